"""What the field methods (nerf.py, surf.py) share literally: the occupancy grid they start from, the optimiser
(base_method.py:60-94), the checkpoint layout (base_method.py:118-264) and full-frame rendering
(base_method.py:366-541).  A subclass sets `models`, `hyper_params`, `occupancy_grid`, `is_training` and
`render_rays`, and `_rebuild_occupancy(iter_nr)` for a checkpoint without its grid."""
import os

import torch

from .background import BoundingSphere
from .volsurfs import OccupancyGrid


def init_occupancy_grid(bounding_primitive, res=256):
    """utils/occupancy_grid.py:6-13."""
    r = bounding_primitive.get_radius()
    grid = OccupancyGrid(res, [r * 2, r * 2, r * 2])
    if isinstance(bounding_primitive, BoundingSphere):
        grid.init_sphere_roi(r, 0.0)
    return grid


class FieldMethod:
    RENDER_KEYS = ("rgb", "rgb_fg", "depth", "weights_sum", "bg_transmittance")   # what render() returns

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    def parameters(self):
        return [p for m in self.models.values() if m is not None for p in m.parameters()]

    # ---- optimisation (base_method.py:60-94)
    def init_optim(self, opt_params=None):
        from .optim import FusedAdam
        from .schedulers import MultiStepLR
        self.optimizer = FusedAdam(opt_params or self.collect_opt_params(), lr=self.hyper_params.lr,
                                   betas=(0.9, 0.99), eps=1e-15, weight_decay=0.0)
        self.scheduler_lr_decay = MultiStepLR(self.optimizer, milestones=self.hyper_params.lr_milestones, gamma=0.3)
        return self.optimizer

    def optim_step(self, overlap=False):
        self.optimizer.step()

    # ---- checkpoints (base_method.py:118-264): <root>/<iter:07d>/models/<model>.pt + the grid
    def save(self, iter_nr):
        if self.save_checkpoints_path is None:
            return None
        path = os.path.join(self.save_checkpoints_path, format(iter_nr, "07d"), "models")
        os.makedirs(path, exist_ok=True)
        for key, model in self.models.items():
            if model is not None:
                torch.save(model.state_dict(), os.path.join(path, f"{key}.pt"))
        if self.occupancy_grid is not None:
            torch.save(self.occupancy_grid.get_grid_values(), os.path.join(path, "grid_values.pt"))
            torch.save(self.occupancy_grid.get_grid_occupancy(), os.path.join(path, "grid_occupancy.pt"))
        if self.optimizer is not None:
            torch.save(self.optimizer.state_dict(), os.path.join(path, "fusedadam.pt"))
        return path

    def load(self, iter_nr):
        if self.load_checkpoints_path is None:
            return None
        path = os.path.join(self.load_checkpoints_path, format(iter_nr, "07d"), "models")
        for key, model in self.models.items():
            f = os.path.join(path, f"{key}.pt")
            if model is not None and os.path.exists(f):
                model.load_state_dict(torch.load(f, map_location="cuda"))
        g = self.occupancy_grid
        if g is not None:
            fv, fo = os.path.join(path, "grid_values.pt"), os.path.join(path, "grid_occupancy.pt")
            if os.path.exists(fv) and os.path.exists(fo):
                g.set_grid_values(torch.load(fv, map_location="cuda"))
                g.set_grid_occupancy(torch.load(fo, map_location="cuda"))
            else:
                self._rebuild_occupancy(iter_nr)
        f = os.path.join(path, "fusedadam.pt")
        if self.optimizer is not None and os.path.exists(f):
            self.optimizer.load_state_dict(torch.load(f, map_location="cuda"))
        return path

    # ---- full frames (base_method.py:366-541)
    RENDER_MODES = ("volumetric",)     # a method with a sphere-traced render adds "sphere_traced"

    @torch.no_grad()
    def render(self, rays_o, rays_d, nr_rays_per_pixel=1, chunk=None, render_mode="volumetric"):
        """`render_mode` picks the entry of render_rays' "renders" (utils/evaluation.py:95's render-mode folders);
        "sphere_traced" sets `render_sphere_traced` for the call."""
        if render_mode not in self.RENDER_MODES:
            raise ValueError(f"{type(self).__name__}: render_mode {render_mode!r} is not one of {self.RENDER_MODES}")
        if render_mode == "sphere_traced" and self.is_training:
            raise ValueError("the sphere-traced render runs outside training only (render_camera sets that)")
        chunk = int(chunk or self.hyper_params.test_rays_batch_size)
        keys = self.RENDER_KEYS
        outs = {k: [] for k in keys}
        was =getattr(self, "render_sphere_traced", False)
        if render_mode == "sphere_traced":
            self.render_sphere_traced = True
        try:
            for a in range(0, rays_o.shape[0], chunk):
                v = self.render_rays(rays_o[a:a + chunk], rays_d[a:a + chunk])["renders"][render_mode]
                for k in keys:
                    outs[k].append(v[k])
        finally:
            if render_mode == "sphere_traced":
                self.render_sphere_traced = was
        full = {k: torch.cat(v, 0) for k, v in outs.items()}
        if nr_rays_per_pixel > 1:
            full = {k: v.reshape(-1, nr_rays_per_pixel, v.shape[-1]).mean(1) for k, v in full.items()}
        return full

    @torch.no_grad()
    def render_camera(self, camera, nr_rays_per_pixel=1, jitter_pixels=False, chunk=None, render_mode="volumetric"):
        """{key: [H, W, C]} of one camera (what evaluation.render_and_eval scores: "rgb")."""
        from .camera import get_camera_rays
        was = self.is_training
        self.is_training = False
        try:
            rays_o, rays_d, _ = get_camera_rays(camera, nr_rays_per_pixel, jitter_pixels)
            full = self.render(rays_o, rays_d, nr_rays_per_pixel, chunk, render_mode)
        finally:
            self.is_training = was
        return {k: v.reshape(camera.height, camera.width, v.shape[-1]) for k, v in full.items()}
