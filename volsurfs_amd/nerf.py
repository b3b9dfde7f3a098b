"""The NeRF method (volsurfs_py/methods/nerf.py, config/nerf/base.cfg, utils/nerf_utils.py): a density field and
a radiance field trained from posed images by volume rendering, the first stage of the baker.  Its two per-ray
chains run as fused HIP kernels (csrc/nerf_render.hip): the foreground composite with the background blend
(`nerf_composite`) and the coarse pass of importance sampling (`nerf_coarse_cdf`); everything else is the
project's existing HIP operators (permutohedral encoder, fused MLP, occupancy grid, packed samplers).
`isosurface.extract_nerf_level_sets` meshes the trained density."""
import torch

from . import _lib
from .background import intersect_bounding_primitive
from .field_method import (FieldHyperParams, FieldMethod, bg_arg, composite_bg_grad, composite_grad_buffers,
                           get_rays_samples_packed)
from .models import Density
from .volsurfs import VolumeRendering


class NeRFHyperParams(FieldHyperParams):
    """params/hyper_params.py (HyperParams, HyperParamsNeRF) with config/nerf/base.cfg applied: the keys and values
    a `nerf` run of the reference trains with.  Keyword arguments override single values."""

    def set_defaults(self):
        super().set_defaults()
        # lr schedule
        self.lr_milestones = [100000, 150000, 180000, 190000]
        self.training_end_iter = 200000
        # density
        self.density_encoding_type = "permutohash"
        self.density_mlp_layers_dims = [32, 32, 32]
        self.density_nr_iters_for_c2f = 1000
        # appearance
        self.appearance_predict_sh_coeffs = False
        self.rgb_normal_dep = False
        # losses
        self.sparsity_weight = 1e-4


# ---- fused per-ray chains (csrc/nerf_render.hip)
class _NerfComposite(torch.autograd.Function):
    """render_fg_volumetric's alpha / transmittance / weights / integrals and render_rays' background blend as one
    launch each way (vsa_nerf_composite_fwd / _bwd).  Differentiable outputs: rgb (blended) and weights_sum; rgb_fg,
    depth and weights are not (the reference integrates the depth without autograd; nerf.py's losses read only rgb
    and weights_sum)."""

    @staticmethod
    def forward(ctx, pack, density, rgb, rgb_bg, want_weights):
        density = _lib.check_f32(density.contiguous())
        rgb = _lib.check_f32(rgb.contiguous())
        S, N = rgb.shape[0], pack.get_nr_rays()
        if density.numel() != S or pack.samples_dt.numel() != S or rgb.shape[1] != 3:
            raise _lib.VolsurfsHipError("nerf composite: rgb [S,3], density [S,1], a pack with S samples and dt")
        rgb_bg, per_ray, bg_shape = bg_arg(rgb_bg, N, "nerf")
        dev = rgb.device
        rgb_fg = torch.empty(N, 3, device=dev)
        rgb_out = torch.empty(N, 3, device=dev)
        wsum = torch.empty(N, 1, device=dev)
        depth = torch.empty(N, 1, device=dev)
        weights = torch.empty(S, 1, device=dev) if want_weights else None
        _lib.call("vsa_nerf_composite_fwd", pack.ray_start_end_idx, density, pack.samples_dt, pack.samples_z, rgb,
                  rgb_bg, per_ray, rgb_fg, rgb_out, wsum, depth, weights, N, _lib.stream_ptr())
        ctx.save_for_backward(density, rgb, rgb_bg, wsum)
        ctx.pack, ctx.per_ray = pack, per_ray
        ctx.bg_shape = bg_shape
        ctx.set_materialize_grads(False)
        nd = [rgb_fg, depth] + ([weights] if weights is not None else [])
        ctx.mark_non_differentiable(*nd)
        return rgb_out, rgb_fg, wsum, depth, weights

    @staticmethod
    def backward(ctx, g_rgb, _g_fg, g_wsum, _g_depth, _g_weights):
        density, rgb, rgb_bg, wsum = ctx.saved_tensors
        pack, ctx.pack = ctx.pack, None
        N = pack.get_nr_rays()
        g_density, g_rgb_s = torch.empty_like(density), torch.empty_like(rgb)
        scratch = torch.empty(2 * rgb.shape[0], device=rgb.device)
        g_rgb, g_bg = composite_grad_buffers(pack, g_rgb, rgb_bg, ctx.needs_input_grad[3])
        _lib.call("vsa_nerf_composite_bwd", pack.ray_start_end_idx, density, pack.samples_dt, rgb, rgb_bg,
                  ctx.per_ray, wsum, g_rgb, None if g_wsum is None else g_wsum.contiguous(), g_density, g_rgb_s, g_bg,
                  scratch, N, bool(VolumeRendering.bug_compat), _lib.stream_ptr())
        return None, g_density, g_rgb_s, composite_bg_grad(ctx, g_bg), None


def nerf_composite(pack, density, rgb, rgb_bg=None, return_weights=False):
    """alpha = 1 - exp(-density dt), T = cumprod((1 - alpha) + 1e-6), w = alpha T (methods/nerf.py:266-287) on a
    compacted pack with dt; rgb_bg [N,3], one colour or None (no blend: rgb = rgb_fg).  Returns a dict: rgb [N,3],
    rgb_fg [N,3], weights_sum [N,1], bg_transmittance [N,1] = 1 - weights_sum, depth [N,1], weights [S,1] (or
    None).  Bit-identical to the chain of CumprodOneMinusAlphaToTransmittanceFunc, IntegrateWithWeights3DFunc and
    SumOverRaysFunc, forward and backward (tests/test_nerf_render.py)."""
    rgb_out, rgb_fg, wsum, depth, weights = _NerfComposite.apply(pack, density.view(-1, 1), rgb, rgb_bg,
                                                                 bool(return_weights))
    return {"rgb": rgb_out, "rgb_fg": rgb_fg, "weights_sum": wsum, "bg_transmittance": 1 - wsum.detach(),
            "depth": depth, "weights": weights}


@torch.no_grad()
def nerf_coarse_cdf(pack, density):
    """importance_sampling_nerf (utils/nerf_utils.py:61-82) from the uniform pass's densities [S,1] to the CDF [S,1]
    in one launch (vsa_nerf_coarse_cdf); bit-identical to the chain of single ops."""
    density = _lib.check_f32(density.contiguous())
    if density.numel() != pack.samples_dt.numel():
        raise _lib.VolsurfsHipError("nerf_coarse_cdf: one density per sample")
    cdf = torch.empty(density.numel(), 1, device=density.device)
    _lib.call("vsa_nerf_coarse_cdf", pack.ray_start_end_idx, density, pack.samples_dt, cdf, pack.get_nr_rays(),
              _lib.stream_ptr())
    return cdf


@torch.no_grad()
def importance_sampling_nerf(density_fn, pack_uniform, iter_nr, nr_samples, jitter_samples=False):
    """utils/nerf_utils.py:9-97: the density of the uniform samples (no autograd), the fused coarse CDF, then
    VolumeRendering.importance_sample."""
    if pack_uniform.is_empty():
        raise _lib.VolsurfsHipError("ray_samples_packed_uniform should not be empty")
    res = density_fn(points=pack_uniform.samples_3d, iter_nr=iter_nr)
    density = res[0] if isinstance(res, tuple) else res
    if density.shape[1] > 1:
        density = density[:, 0:1]
    pack_uniform.update_dt(False)
    cdf = nerf_coarse_cdf(pack_uniform, density)
    return VolumeRendering.importance_sample(pack_uniform, cdf, nr_samples, jitter_samples)


def get_rays_samples_packed_nerf(rays_o, rays_d, t_near, t_far, density_fn, occupancy_grid=None, iter_nr=None,
                                 min_dist_between_samples=1e-4, min_nr_samples_per_ray=1, max_nr_samples_per_ray=64,
                                 max_nr_imp_samples_per_ray=32, jitter_samples=False, importance_sampling=True,
                                 values_dim=1):
    """utils/nerf_utils.py:100-190 -> (pack with dt, importance pack or None)."""
    imp_fn = (lambda pack: importance_sampling_nerf(density_fn, pack, iter_nr, max_nr_imp_samples_per_ray,
                                                    jitter_samples)) if importance_sampling else None
    return get_rays_samples_packed(rays_o, rays_d, t_near, t_far, imp_fn, occupancy_grid, min_dist_between_samples,
                                   min_nr_samples_per_ray, max_nr_samples_per_ray, jitter_samples, values_dim)


class NeRF(FieldMethod):
    """methods/nerf.py:29-507.  models = {"density": Density, "rgb": RGB or ColorSH, "bg": NerfHash or None (with a
    constant bg_color [3])}; the occupancy grid of init_occupancy_grid (256^3, a sphere ROI for a BoundingSphere).
    Trains through trainer.train_step / train (the autograd path): `method(rays_o, rays_d, gt_rgb, gt_mask, iter_nr)`
    returns (losses, info, foreground samples) — the sample count drives the dynamic ray count."""

    method_name = "nerf"
    OCCUPANCY_RANDOM_VOXELS = 256 * 256 * 4   # update_occupancy_grid (nerf.py:194-255); every 50 iterations
    OCCUPANCY_DECAY = 0.8
    SPARSITY_FROM_ITER = 5000              # the sparsity term is on for iter_nr > 5000 (nerf.py:467)
    SPARSITY_NR_POINTS = 1024

    def __init__(self, train, hyper_params, load_checkpoints_path, save_checkpoints_path, bounding_primitive,
                 bg_color=None, start_iter_nr=0):
        hp = hyper_params
        bb = self._init_common(train, hp, load_checkpoints_path, save_checkpoints_path, bounding_primitive, bg_color)
        self.models["density"] = Density(in_channels=3, out_channels=1, geom_feat_size=hp.geom_feat_size,
                                         mlp_layers_dims=hp.density_mlp_layers_dims,
                                         encoding_type=hp.density_encoding_type,
                                         nr_iters_for_c2f=hp.density_nr_iters_for_c2f, bb_sides=bb)
        self.models["rgb"] = self._rgb_model(bb)
        self.models["bg"] = self._background_model()
        self._load_and_init_optim(train, start_iter_nr)
        self.update_method_state(iter_nr=start_iter_nr)
        self.update_occupancy_grid(iter_nr=start_iter_nr, decay=0.0, random_voxels=False, jitter_samples=False)

    # ---- optimisation (base_method.py:60-94, nerf.py:143-192)
    def collect_opt_params(self):
        groups = [{"params": list(self.models["density"].parameters()), "lr": self.hyper_params.lr,
                   "name": "model_density"},
                  {"params": list(self.models["rgb"].parameters()), "lr": self.hyper_params.lr, "name": "model_rgb"}]
        if self.models["bg"] is not None:
            groups.append({"params": list(self.models["bg"].parameters()), "lr": self.hyper_params.lr,
                           "name": "model_bg"})
        return groups

    # ---- occupancy grid (nerf.py:194-255, 414-421)
    @torch.no_grad()
    def update_occupancy_grid(self, iter_nr, decay=OCCUPANCY_DECAY, random_voxels=True, jitter_samples=True):
        g = self.occupancy_grid
        if g is None:
            return
        if random_voxels:
            pts, idx = g.get_random_grid_samples_in_roi(self.OCCUPANCY_RANDOM_VOXELS, jitter_samples)
        else:
            pts, idx = g.get_grid_samples(jitter_samples)
        dens = [self.models["density"](b, iter_nr=iter_nr)[0] for b in torch.split(pts, 256 * 256 * 100, dim=0)]
        dens = torch.cat(dens, 0) if len(dens) > 1 else dens[0]
        g.update_grid_values(idx, dens, decay)
        g.update_grid_occupancy_with_density_values(idx, self.OCCUPANCY_THRESH, False)

    def update_method_state(self, iter_nr):
        if self.is_training and self.hyper_params.use_occupancy_grid and iter_nr % self.OCCUPANCY_EVERY == 0:
            self.update_occupancy_grid(iter_nr=iter_nr)

    # ---- rendering (nerf.py:257-412)
    def render_fg_volumetric(self, pack, iter_nr=None, override=None, rgb_bg=None):
        """-> (renders dict, samples_3d, None).  `rgb_bg` folds render_rays' blend into the same launch."""
        N = pack.get_nr_rays()
        dev = pack.ray_o.device
        if pack.is_empty():
            return self._zero_renders(N, dev, rgb_bg, {"rgb_fg": (3,), "depth": (1,), "weights_sum": (1,)}), None, None
        samples_3d = pack.samples_3d
        density, geom_feat = self.models["density"](points=samples_3d, iter_nr=iter_nr)
        dirs = pack.samples_dirs
        view_dir = (override or {}).get("view_dir")
        if view_dir is not None:
            dirs = torch.as_tensor(view_dir, dtype=torch.float32, device=dev).view(1, 3).expand(dirs.shape[0], 3).contiguous()
        rgb = self.models["rgb"](points=samples_3d, samples_dirs=dirs, iter_nr=iter_nr, geom_feat=geom_feat)
        c = nerf_composite(pack, density, rgb, rgb_bg)
        r = {"rgb": c["rgb"], "rgb_fg": c["rgb_fg"], "depth": c["depth"], "weights_sum": c["weights_sum"],
             "bg_transmittance": c["bg_transmittance"],
             "nr_samples": pack.get_nr_samples_per_ray().view(-1, 1).int()}
        return r, samples_3d, None

    def render_rays(self, rays_o, rays_d, iter_nr=None, override=None, **kwargs):
        """The reference's dict: {"renders": {"volumetric": {rgb, rgb_fg, rgb_bg, depth, weights_sum,
        bg_transmittance, nr_samples[, median_depth_bg]}}, "samples_3d", "samples_grad"}."""
        hp = self.hyper_params
        raycast = intersect_bounding_primitive(self.bounding_primitive, rays_o, rays_d)
        pack, _ = get_rays_samples_packed_nerf(
            rays_o, rays_d, raycast["t_near"], raycast["t_far"], self.models["density"], self.occupancy_grid, iter_nr,
            hp.min_dist_between_samples, hp.min_nr_samples_per_ray, hp.max_nr_samples_per_ray,
            hp.max_nr_imp_samples_per_ray, jitter_samples=self.is_training, importance_sampling=hp.do_importance_sampling)
        rgb_bg, blend_bg, median_bg = self._render_bg(raycast, iter_nr)
        renders, samples_3d, samples_grad = self.render_fg_volumetric(pack, iter_nr=iter_nr, override=override,
                                                                      rgb_bg=blend_bg)
        renders["rgb_bg"] = rgb_bg
        if median_bg is not None:
            renders["median_depth_bg"] = median_bg
        return {"renders": {"volumetric": renders}, "samples_3d": samples_3d, "samples_grad": samples_grad}

    # ---- training (nerf.py:423-507)
    def forward(self, rays_o, rays_d, gt_rgb, gt_mask=None, iter_nr=0, is_first_iter=False, is_training_masked=None,
                **kwargs):
        hp = self.hyper_params
        masked = hp.is_training_masked if is_training_masked is None else is_training_masked
        self.update_method_state(iter_nr)
        if is_first_iter and self.scheduler_lr_decay is not None:           # nerf.py:437-443
            self._install_warmup()
        res = self.render_rays(rays_o, rays_d, iter_nr=iter_nr)
        loss_rgb, pred_mask = self._loss_rgb(res["renders"]["volumetric"], gt_rgb, gt_mask, masked)
        loss = loss_rgb
        loss_sparsity = loss_mask = 0.0
        points = self.bounding_primitive.get_random_points_inside(self.SPARSITY_NR_POINTS)
        if iter_nr > self.SPARSITY_FROM_ITER and hp.sparsity_weight > 0.0:
            dens, _ = self.models["density"](points, iter_nr)
            loss_sparsity = torch.clamp((1 - torch.exp(-dens)).mean(), min=0.0) * hp.sparsity_weight  # losses.py:22-25
            loss = loss + loss_sparsity
        if masked and hp.mask_weight > 0.0:
            loss_mask = self._loss_mask(pred_mask, gt_mask)
            loss = loss + loss_mask
        losses = {"loss": loss, "rgb": loss_rgb, "sparsity": loss_sparsity, "mask": loss_mask}
        return losses, {}, res["samples_3d"]

    def _rebuild_occupancy(self, iter_nr):
        self.update_occupancy_grid(iter_nr=iter_nr, decay=0.0, random_voxels=False, jitter_samples=False)
