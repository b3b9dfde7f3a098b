"""What the field methods (nerf.py, surf.py, offsets_surfs.py) share: the hyper-parameter base, the foreground
sampler and the two-round SDF importance procedure, the finite-difference stencil of a field, the autograd
wrappers' background handling, and `FieldMethod`: the constructor's common part, the appearance and background
models, the occupancy grid they start from, the optimiser (base_method.py:60-94), the shared loss terms, the
checkpoint layout (base_method.py:118-264) and full-frame rendering (base_method.py:366-541).  A subclass sets
`models`, `render_rays` and `collect_opt_params`, and `_rebuild_occupancy(iter_nr)` for a checkpoint without its
grid."""
import os

import numpy as np
import torch

from . import _lib
from .background import BoundingSphere, render_contracted_bg
from .models import RGB, ColorSH, NerfHash
from .trainer import loss_l1
from .volsurfs import OccupancyGrid, RaySampler, VolumeRendering


class FieldHyperParams:
    """params/hyper_params.py (HyperParams): the keys and values the `nerf` and `surf` configurations have in
    common.  A subclass adds its own in `set_defaults`; keyword arguments override single values, then `validate`
    runs."""

    def __init__(self, **overrides):
        self.set_defaults()
        for k, v in overrides.items():
            if not hasattr(self, k):
                raise KeyError(f"unknown hyper-parameter {k!r}")
            setattr(self, k, v)
        self.validate()

    def set_defaults(self):
        # lr schedule
        self.lr = 1e-3
        self.nr_warmup_iters = 3000
        # rays
        self.training_rays_batch_size = 512
        self.is_nr_training_rays_dynamic = True
        self.target_nr_of_training_samples = 512 * (64 + 16 + 16)
        self.test_rays_batch_size = 16384
        self.nr_training_rays_per_pixel = 1
        self.nr_test_rays_per_pixel = 1
        self.jitter_training_rays = True
        self.jitter_test_rays = False
        # masks
        self.is_training_masked = False
        self.is_testing_masked = False
        self.mask_weight = 0.0
        # appearance
        self.geom_feat_size = 32
        self.rgb_pos_encoder_type = "permutohash"
        self.rgb_dir_encoder_type = "spherical_harmonics"
        self.rgb_mlp_layers_dims = [128, 128, 64]
        self.sh_degree = 3
        self.rgb_view_dep = True
        self.rgb_geom_feat_dep = True
        self.rgb_nr_iters_for_c2f = 0
        # background
        self.bg_pos_encoder_type = "permutohash"
        self.bg_dir_encoder_type = "spherical_harmonics"
        self.bg_nr_iters_for_c2f = 0
        self.nr_samples_bg = 64
        # sampling
        self.use_occupancy_grid = True
        self.do_importance_sampling = True
        self.min_dist_between_samples = 1e-4
        self.min_nr_samples_per_ray = 1
        self.max_nr_samples_per_ray = 64
        self.max_nr_imp_samples_per_ray = 32

    def validate(self):
        # hyper_params.py:173-178: the CDF of importance sampling needs 3 samples per ray
        if self.do_importance_sampling and self.min_nr_samples_per_ray < 3:
            self.min_nr_samples_per_ray = 3


def get_logistic_beta_from_variance(variance):
    """logistic_distribution.py:5-8: clip(exp(10 variance), 1e-6, 1e6) (float64)."""
    return float(np.clip(np.exp(variance * 10.0), 1e-6, 1e6))


# ---- field derivatives and losses (utils/fields_utils.py, utils/losses.py)
FD_EPS = 1e-4


def field_stencil(field_fn, points, iter_nr=None, eps=FD_EPS):
    """The field on [p, p + eps x, p + eps y, p + eps z] as ONE call of 4M rows (fields_utils.py:9-31)."""
    with torch.no_grad():
        px, py, pz = points.clone(), points.clone(), points.clone()
        px[:, 0] += eps
        py[:, 1] += eps
        pz[:, 2] += eps
        full = torch.cat([points, px, py, pz], 0)
    return field_fn(full) if iter_nr is None else field_fn(full, iter_nr)


def stencil_gradients(sdfs_full, eps=FD_EPS):
    """fields_utils.py:33-56: the forward differences of the stencil's first column -> [M, 3]."""
    if sdfs_full.dim() < 2:
        sdfs_full = sdfs_full.unsqueeze(1)
    if sdfs_full.shape[-1] > 1:
        sdfs_full = sdfs_full[:, 0].unsqueeze(1)
    sdf, sx, sy, sz = sdfs_full.chunk(4, dim=0)
    return torch.cat([(sx - sdf) / eps, (sy - sdf) / eps, (sz - sdf) / eps], dim=-1)


def eikonal_loss(sdf_gradients, distance_scale=1.0):
    """utils/losses.py:28-33."""
    return ((torch.linalg.norm(sdf_gradients, ord=2, dim=-1) - distance_scale) ** 2).mean()


# ---- the autograd wrappers of the fused composites: the background argument and its gradient
def bg_arg(rgb_bg, N, composite):
    """-> (fp32 tensor or None, bg_per_ray, the caller's shape): rgb_bg [N,3] is per ray, 3 numbers are one colour.
    `composite` names the caller in the error."""
    if rgb_bg is None:
        return None, 0, None
    if rgb_bg.dim() == 2 and rgb_bg.shape == (N, 3) and N != 1:
        return _lib.check_f32(rgb_bg.contiguous()), 1, rgb_bg.shape
    if rgb_bg.numel() == 3:
        return _lib.check_f32(rgb_bg.reshape(3).contiguous()), 0, rgb_bg.shape
    raise _lib.VolsurfsHipError(f"{composite} composite: rgb_bg must be [N,3] or one colour, got {tuple(rgb_bg.shape)}")


def composite_grad_buffers(pack, g_rgb, bg, bg_needs_grad):
    """Before a composite's backward launch -> (g_rgb contiguous, zeros when autograd passed none; the buffer
    g_bg [N,3] the kernel fills, or None when the background takes no gradient)."""
    N, dev = pack.get_nr_rays(), pack.ray_start_end_idx.device
    g_rgb = torch.zeros(N, 3, device=dev) if g_rgb is None else g_rgb.contiguous()
    return g_rgb, (torch.empty(N, 3, device=dev) if bg is not None and bg_needs_grad else None)


def composite_bg_grad(ctx, g_bg):
    """After the launch: one colour's gradient is the sum over the rays, in the shape it came in (ctx.per_ray,
    ctx.bg_shape of bg_arg)."""
    return g_bg if g_bg is None or ctx.per_ray else g_bg.sum(0).view(ctx.bg_shape)


# ---- foreground samples (utils/nerf_utils.py:100-190, sdf_utils.py:178-281, sdfs_utils.py:435-510)
def get_rays_samples_packed(rays_o, rays_d, t_near, t_far, importance_fn, occupancy_grid, min_dist_between_samples,
                            min_nr_samples_per_ray, max_nr_samples_per_ray, jitter_samples, values_dim):
    """-> (pack with dt, importance pack or None): the samples in the occupied voxels (or uniform ones without a
    grid), merged with `importance_fn(pack)`'s samples when a function is given."""
    with torch.no_grad():
        if occupancy_grid is not None:
            pack = RaySampler.compute_samples_fg_in_grid_occupied_regions(
                rays_o, rays_d, t_near, t_far, min_dist_between_samples, min_nr_samples_per_ray,
                max_nr_samples_per_ray, jitter_samples, occupancy_grid.get_nr_voxels_per_dim(),
                occupancy_grid.get_grid_extent(), occupancy_grid.get_grid_occupancy(), occupancy_grid.get_grid_roi(),
                values_dim)
        else:
            pack = RaySampler.compute_samples_fg(rays_o, rays_d, t_near, t_far, min_dist_between_samples,
                                                 min_nr_samples_per_ray, max_nr_samples_per_ray, jitter_samples,
                                                 values_dim)
        imp = None
        if not pack.is_empty():
            if importance_fn is not None:
                imp = importance_fn(pack)
                pack = VolumeRendering.combine_ray_samples_packets(pack, imp, min_dist_between_samples)
            pack.update_dt(False)
    return pack, imp


@torch.no_grad()
def importance_sampling_sdf_rounds(values_fn, cdf_fn, nr_columns, pack_uniform, nr_samples, logistic_beta_value,
                                   min_dist_between_samples, jitter_samples=False):
    """sdf_utils.py:40-175 / sdfs_utils.py:67-180 -> the two rounds' samples merged: round one on the uniform samples
    with beta / 2, round two on the combined pack (whose samples_values carry the `nr_columns` SDF columns) with
    beta, nr_samples // 2 each.  `values_fn(points)` evaluates the SDF columns, `cdf_fn(pack, values, beta)` is the
    fused coarse CDF of one round."""
    if pack_uniform.is_empty():
        raise _lib.VolsurfsHipError("ray_samples_packed_uniform should not be empty")
    sdf = values_fn(pack_uniform.samples_3d)
    pack_uniform.update_dt(False)
    beta = np.float32(logistic_beta_value)          # torch.ones_like(dt) * logistic_beta_value
    cdf = cdf_fn(pack_uniform, sdf, beta / np.float32(2.0))
    imp_1 = VolumeRendering.importance_sample(pack_uniform, cdf, nr_samples // 2, jitter_samples)
    sdf_1 = values_fn(imp_1.samples_3d)
    pack_uniform.set_samples_values(sdf.reshape(-1, nr_columns))
    imp_1.set_samples_values(sdf_1.reshape(-1, nr_columns))
    combined = VolumeRendering.combine_ray_samples_packets(pack_uniform, imp_1, min_dist_between_samples)
    sdf_c = combined.samples_values
    pack_uniform.remove_samples_values()
    imp_1.remove_samples_values()
    combined.remove_samples_values()         # (so that imp_2 is created without values, like imp_1)
    combined.update_dt(False)
    cdf = cdf_fn(combined, sdf_c, beta)
    imp_2 = VolumeRendering.importance_sample(combined, cdf, nr_samples // 2, jitter_samples)
    return imp_1, imp_2


def init_occupancy_grid(bounding_primitive, res=256):
    """utils/occupancy_grid.py:6-13."""
    r = bounding_primitive.get_radius()
    grid = OccupancyGrid(res, [r * 2, r * 2, r * 2])
    if isinstance(bounding_primitive, BoundingSphere):
        grid.init_sphere_roi(r, 0.0)
    return grid


class FieldMethod:
    RENDER_KEYS = ("rgb", "rgb_fg", "depth", "weights_sum", "bg_transmittance")   # what render() returns
    OCCUPANCY_EVERY = 50                   # update_method_state
    OCCUPANCY_MAX_VARIANCE = 0.8           # the SDF methods' update_occupancy_grid (surf.py:286-299)
    OCCUPANCY_THRESH = 1e-4
    NR_RANDOM_POINTS = 1024                # surf.py:985, offsets_surfs.py:1264
    OFFSURFACE_SCALE = 1e2                 # surf.py:1031

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    # ---- construction: what every method's __init__ starts and ends with
    def _init_common(self, train, hyper_params, load_checkpoints_path, save_checkpoints_path, bounding_primitive,
                     bg_color):
        """-> bb_sides of the models.  The occupancy grid is made here, the models by the subclass, in its order."""
        self.hyper_params = hyper_params
        self.load_checkpoints_path, self.save_checkpoints_path = load_checkpoints_path, save_checkpoints_path
        self.bounding_primitive = bounding_primitive
        self.bg_color = None if bg_color is None else torch.as_tensor(bg_color, dtype=torch.float32).cuda().view(1, 3)
        self.optimizer = self.lr_scheduler = self.scheduler_lr_decay = None
        self.is_training = bool(train)
        self.occupancy_grid = init_occupancy_grid(bounding_primitive) if hyper_params.use_occupancy_grid else None
        self.models = {}
        return bounding_primitive.get_radius() * 2.0

    def _appearance_model(self, out_channels, view_dep, normal_dep, geom_feat_dep, bb):
        hp = self.hyper_params
        if hp.appearance_predict_sh_coeffs:
            return ColorSH(in_channels=3, out_channels=out_channels, mlp_layers_dims=hp.rgb_mlp_layers_dims,
                           pos_encoder_type=hp.rgb_pos_encoder_type, sh_deg=hp.sh_degree, normal_dep=normal_dep,
                           geom_feat_dep=geom_feat_dep, in_geom_feat_size=hp.geom_feat_size,
                           nr_iters_for_c2f=hp.rgb_nr_iters_for_c2f, bb_sides=bb)
        return RGB(in_channels=3, out_channels=out_channels, mlp_layers_dims=hp.rgb_mlp_layers_dims,
                   pos_encoder_type=hp.rgb_pos_encoder_type, dir_encoder_type=hp.rgb_dir_encoder_type,
                   sh_deg=hp.sh_degree, view_dep=view_dep, normal_dep=normal_dep, geom_feat_dep=geom_feat_dep,
                   in_geom_feat_size=hp.geom_feat_size, nr_iters_for_c2f=hp.rgb_nr_iters_for_c2f, bb_sides=bb)

    def _rgb_model(self, bb):
        hp = self.hyper_params
        if hp.appearance_predict_sh_coeffs:
            assert hp.rgb_view_dep, "SH coeffs only implemented for view dependent color"
        return self._appearance_model(3, hp.rgb_view_dep, hp.rgb_normal_dep, hp.rgb_geom_feat_dep, bb)

    def _background_model(self):
        """A NerfHash, or None with a constant bg_color."""
        hp = self.hyper_params
        return NerfHash(in_channels=3, pos_encoder_type=hp.bg_pos_encoder_type, dir_encoder_type=hp.bg_dir_encoder_type,
                        nr_iters_for_c2f=hp.bg_nr_iters_for_c2f) if self.bg_color is None else None

    def _load_and_init_optim(self, train, start_iter_nr):
        if start_iter_nr > 0:
            self.load(start_iter_nr)
        if train:
            self.init_optim()

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

    def _install_warmup(self):
        """nerf.py:437-443, surf.py:843-856: the warm-up in front of the milestone decay, once an optimiser exists."""
        from .schedulers import GradualWarmupScheduler
        if self.hyper_params.nr_warmup_iters > 0:
            self.lr_scheduler = GradualWarmupScheduler(self.optimizer, multiplier=1,
                                                       total_epoch=self.hyper_params.nr_warmup_iters,
                                                       after_scheduler=self.scheduler_lr_decay)
        else:
            self.lr_scheduler = self.scheduler_lr_decay

    # ---- occupancy grid of the SDF methods (surf.py:246-302, offsets_surfs.py:387-418): the full grid, the
    # distance to the nearest surface, beta of min(0.8, variance)
    @torch.no_grad()
    def _update_sdf_occupancy(self, sdf_fn, distance, iter_nr, decay):
        """`distance(sdf_fn's values)` -> [M,1], the unsigned distance the grid stores."""
        g = self.occupancy_grid
        if g is None:
            return
        pts, idx = g.get_grid_samples(False)
        sdf = [sdf_fn(b, iter_nr=iter_nr)[0] for b in torch.split(pts, 256 * 256 * 100, dim=0)]
        sdf = distance(torch.cat(sdf, 0) if len(sdf) > 1 else sdf[0])
        beta = torch.ones_like(sdf) * get_logistic_beta_from_variance(min(self.OCCUPANCY_MAX_VARIANCE, self.variance))
        g.update_grid_values(idx, sdf, decay)
        g.update_grid_occupancy_with_sdf_values(idx, beta, self.OCCUPANCY_THRESH, False)

    def _rebuild_occupancy(self, iter_nr):
        self.update_occupancy_grid(iter_nr=iter_nr)

    # ---- render_rays' background and the render of a pack without samples
    def _render_bg(self, raycast, iter_nr):
        """-> (rgb_bg [N,3], what the composite blends with: the one colour or rgb_bg, the background's median
        depth or None for a constant colour)."""
        if self.models["bg"] is None:
            return self.bg_color.expand(raycast["nr_rays"], 3), self.bg_color.view(3), None
        bg = render_contracted_bg(self.models["bg"], raycast, nr_samples_bg=self.hyper_params.nr_samples_bg,
                                  jitter_samples=self.is_training, iter_nr=iter_nr)
        return bg["pred_rgb"], bg["pred_rgb"], bg["median_depth"]

    @staticmethod
    def _zero_renders(N, dev, rgb_bg, zero_shapes):
        """No foreground: the entries of `zero_shapes` are zeros [N, *shape], bg_transmittance is 1 and rgb is the
        background."""
        r = {k: torch.zeros(N, *shape, device=dev) for k, shape in zero_shapes.items()}
        r["bg_transmittance"] = torch.ones(N, 1, device=dev)
        r["nr_samples"] = torch.zeros(N, 1, dtype=torch.int32, device=dev)
        r["rgb"] = r["rgb_fg"] if rgb_bg is None else r["rgb_fg"] + r["bg_transmittance"] * rgb_bg
        return r

    # ---- loss terms the methods share (nerf.py:445-500, surf.py:960-1100, offsets_surfs.py:1230-1400)
    def _loss_rgb(self, vol, gt_rgb, gt_mask, masked):
        """-> (the L1 colour loss, masked or not, the predicted mask or None), both averaged over a pixel's rays."""
        pred_rgb, pred_mask = vol["rgb"], vol.get("weights_sum")
        R = self.hyper_params.nr_training_rays_per_pixel
        if R > 1:
            pred_rgb = pred_rgb.view(-1, R, 3).mean(dim=1)
            pred_mask = None if pred_mask is None else pred_mask.view(-1, R, 1).mean(dim=1)
        return (loss_l1(gt_rgb, pred_rgb, mask=gt_mask) if masked else loss_l1(gt_rgb, pred_rgb)), pred_mask

    def _loss_mask(self, pred_mask, gt_mask):
        pm = torch.clamp(pred_mask, min=0.0, max=1.0)
        return loss_l1(pm, gt_mask, mask=1 - gt_mask) * self.hyper_params.mask_weight

    def _random_points_stencil(self, sdf_fn, iter_nr):
        """-> (sdf, its finite-difference gradient) at NR_RANDOM_POINTS random points of the bounding primitive,
        from one evaluation of the 4-point stencil."""
        with torch.no_grad():
            pts = self.bounding_primitive.get_random_points_inside(self.NR_RANDOM_POINTS)
        full = field_stencil(sdf_fn, pts, iter_nr)[0]
        return full[:pts.shape[0]], stencil_gradients(full)

    @staticmethod
    def _loss_eikonal(random_grad, samples_grad, weight):
        """The eikonal term at the random points, plus the one at the ray samples when there are any (None: none)."""
        loss = eikonal_loss(random_grad) * weight
        return loss if samples_grad is None else loss + eikonal_loss(samples_grad) * weight

    def _loss_offsurface(self, random_sdf):
        return torch.exp(-self.OFFSURFACE_SCALE * torch.abs(random_sdf)).mean() * self.hyper_params.offsurface_weight

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
        was = getattr(self, "render_sphere_traced", False)
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
