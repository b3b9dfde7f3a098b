"""The Surf method (volsurfs_py/methods/surf.py, config/surf/base.cfg, utils/sdf_utils.py, utils/fields_utils.py):
a NeuS signed distance field and a radiance field trained from posed images by volume rendering, the stage whose
`sdf.pt` the later methods start from.  Its two per-ray chains run as fused HIP kernels (csrc/surf_render.hip):
the NeuS foreground composite with the background blend (`neus_composite`) and one round of the coarse CDF of
importance sampling (`sdf_coarse_cdf`); everything else is the project's existing HIP operators (permutohedral
encoder, fused MLP, occupancy grid, packed samplers).  `isosurface.extract_surf_level_sets` meshes the SDF."""
import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .background import intersect_bounding_primitive
from .field_method import (FD_EPS, FieldHyperParams, FieldMethod, bg_arg, composite_bg_grad, composite_grad_buffers,
                           field_stencil, get_logistic_beta_from_variance, get_rays_samples_packed,
                           importance_sampling_sdf_rounds, stencil_gradients)
from .field_method import eikonal_loss  # noqa: F401  (its users import it from here)
from .models import SDF
from .volsurfs import VolumeRendering


class SurfHyperParams(FieldHyperParams):
    """params/hyper_params.py (HyperParams, HyperParamsSuRF) with config/surf/base.cfg applied: the keys and values
    a `surf` run of the reference trains with.  Keyword arguments override single values."""

    def set_defaults(self):
        super().set_defaults()
        # lr schedule
        self.lr_milestones = [80000, 90000]
        self.training_end_iter = 100000
        # phases
        self.init_phase_end_iter = 5000
        self.first_phase_end_iter = 100000
        self.first_phase_variance_start_value = 0.3
        self.first_phase_variance_end_value = 0.7
        self.reduce_curv_start_iter = None
        self.reduce_curv_end_iter = None
        # sdf
        self.sdf_encoding_type = "permutohash"
        self.sdf_mlp_layers_dims = [32, 32, 32]
        self.sdf_mlp_output_dims = 1
        self.sdf_nr_iters_for_c2f = 5000
        # appearance
        self.rgb_mlp_output_dims = 3
        self.appearance_predict_sh_coeffs = True
        self.rgb_normal_dep = True
        self.rgb_use_lipshitz_mlp = False
        self.use_color_calibration = False
        self.use_grad_scaler = False
        # losses
        self.eikonal_weight = 0.04
        self.curvature_weight = 0.65
        self.lipshitz_weight = 0.0
        self.offsurface_weight = 1e-4

    def validate(self):
        if self.rgb_use_lipshitz_mlp or self.lipshitz_weight > 0.0:
            raise NotImplementedError("the Lipschitz MLP and its loss are not implemented")
        if self.use_color_calibration or self.use_grad_scaler:
            raise NotImplementedError("colour calibration and the grad scaler are not implemented")
        super().validate()


# ---- schedule helpers (utils/common.py, utils/logistic_distribution.py)
def map_range_val(input_val, input_start, input_end, output_start, output_end):
    """utils/common.py:94-100."""
    clamped = max(input_start, min(input_end, input_val))
    if input_start >= input_end:
        return output_end
    return output_start + ((output_end - output_start) / (input_end - input_start)) * (clamped - input_start)


def logistic_distribution_stdev(beta=1.0):
    return (1.0 / beta * np.pi) / np.sqrt(3)


def curvature_weight_schedule(iter_nr, reduce_curv_start_iter, reduce_curv_end_iter):
    """surf.py:1042-1060: 1 without a reduction window, else 1 -> 0 over it and 0 after."""
    if reduce_curv_end_iter is None or reduce_curv_start_iter is None:
        return 1.0
    if iter_nr < reduce_curv_end_iter:
        return map_range_val(iter_nr, reduce_curv_start_iter, reduce_curv_end_iter, 1.0, 0.0)
    return 0.0


# ---- field derivatives (utils/fields_utils.py; the stencil itself is field_method.py's)
def get_field_gradients(field_fn, points, iter_nr=None, eps=FD_EPS):
    """fields_utils.py:6-66 (grad_method "finite-diff")."""
    res = field_stencil(field_fn, points, iter_nr, eps)
    return stencil_gradients(res[0] if isinstance(res, tuple) else res, eps)


def get_sdfs_curvature(sdfs_fn, points, sdfs_gradients, rand_directions, iter_nr=None, eps=FD_EPS):
    """fields_utils.py:69-166 for K surfaces with the random directions given: the K shifted point sets
    (points + tangent_k eps) evaluated as ONE stencil call of 4 K M rows, column k of block k -> [M, K, 1]
    ([M] for one surface).  Same rows and values as the reference's K calls."""
    normals = F.normalize(sdfs_gradients, dim=-1)
    K = sdfs_gradients.shape[1] if sdfs_gradients.dim() > 2 else 1
    rand_directions = F.normalize(rand_directions, dim=-1)
    if normals.dim() > 2:
        rand_directions = rand_directions.unsqueeze(1)
    tangent = torch.cross(normals, rand_directions, dim=-1)
    M = points.shape[0]
    if tangent.dim() > 2:
        shifted = torch.cat([points + tangent[:, i] * eps for i in range(K)], 0)
    else:
        shifted = points + tangent * eps
    res = field_stencil(sdfs_fn, shifted, iter_nr)
    grads = stencil_gradients(res[0] if isinstance(res, tuple) else res)       # [K M, K, 3] or [M, 3]
    if normals.dim() > 2:
        shifted_n = torch.stack([F.normalize(grads[i * M:(i + 1) * M, i], dim=-1) if grads.dim() > 2
                                 else F.normalize(grads[i * M:(i + 1) * M], dim=-1) for i in range(K)], 1)
    else:
        shifted_n = F.normalize(grads[:, 0] if grads.dim() > 2 else grads, dim=-1)
    dot = torch.sum(torch.mul(normals, shifted_n), dim=-1, keepdim=True)
    angle = torch.acos(torch.clamp(dot, -1.0 + 1e-6, 1.0 - 1e-6))
    curv = angle / np.pi
    return curv.squeeze(1) if K == 1 else curv


def get_sdf_curvature(sdf_fn, points, sdf_gradients, rand_directions, iter_nr=None, eps=FD_EPS):
    """fields_utils.py:69-166 for one surface, with the random directions given (the method passes
    torch.randn_like(points)): the angle between the normal and the normal a step eps along a random tangent,
    over pi -> [M].  get_sdfs_curvature on gradients [M, 3]."""
    return get_sdfs_curvature(sdf_fn, points, sdf_gradients, rand_directions, iter_nr, eps)


def neus_alphas_torch(samples_dirs, samples_dt, sdf, gradients, cos_anneal_ratio, logistic_beta):
    """VolumeRenderingNeuS.compute_alphas_from_logistic_beta as torch elementwise ops (the restatement that
    csrc/surf_render.hip's prologue follows op by op)."""
    true_cos = (samples_dirs * gradients).sum(-1, keepdim=True)
    iter_cos = -(F.relu(-true_cos * 0.5 + 0.5) * (1.0 - cos_anneal_ratio) + F.relu(-true_cos) * cos_anneal_ratio)
    next_sdf = sdf + iter_cos * samples_dt * 0.5
    prev_sdf = sdf - iter_cos * samples_dt * 0.5
    prev_cdf = torch.sigmoid(prev_sdf * logistic_beta)
    next_cdf = torch.sigmoid(next_sdf * logistic_beta)
    return ((prev_cdf - next_cdf + 1e-6) / (prev_cdf + 1e-6)).clip(0.0, 1.0)


# ---- fused per-ray chains (csrc/surf_render.hip)
class _NeusComposite(torch.autograd.Function):
    """render_fg_volumetric's NeuS alpha / transmittance / weights / integrals and render_rays' background blend as
    one launch each way (vsa_neus_composite_fwd / _bwd).  Differentiable inputs: sdf, sdf_grad, rgb, rgb_bg;
    differentiable outputs: rgb (blended) and weights_sum.  depth, normals and weights carry no gradient (the
    reference integrates them without autograd)."""

    @staticmethod
    def forward(ctx, pack, sdf, sdf_grad, normals, rgb, rgb_bg, cos_anneal_ratio, logistic_beta, want_weights):
        sdf = _lib.check_f32(sdf.contiguous())
        sdf_grad = _lib.check_f32(sdf_grad.contiguous())
        normals = _lib.check_f32(normals.contiguous())
        rgb = _lib.check_f32(rgb.contiguous())
        S, N = rgb.shape[0], pack.get_nr_rays()
        if sdf.numel() != S or sdf_grad.shape != (S, 3) or normals.shape != (S, 3) or rgb.shape[1] != 3 or \
                pack.samples_dt.numel() != S:
            raise _lib.VolsurfsHipError("neus composite: sdf [S,1], sdf_grad / normals / rgb [S,3], a pack with dt")
        bg, per_ray, bg_shape = bg_arg(rgb_bg, N, "neus")
        dev = rgb.device
        rgb_fg, rgb_out, nrm = torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)
        wsum, depth = torch.empty(N, 1, device=dev), torch.empty(N, 1, device=dev)
        weights = torch.empty(S, 1, device=dev) if want_weights else None
        alpha = torch.empty(S, 1, device=dev) if want_weights else None
        dirs = pack.samples_dirs.contiguous()
        _lib.call("vsa_neus_composite_fwd", pack.ray_start_end_idx, sdf, sdf_grad, dirs, pack.samples_dt,
                  pack.samples_z, normals, rgb, bg, per_ray, float(cos_anneal_ratio), float(logistic_beta), rgb_fg,
                  rgb_out, wsum, depth, nrm, weights, alpha, N, _lib.stream_ptr())
        ctx.save_for_backward(sdf, sdf_grad, dirs, rgb, bg, wsum)
        ctx.pack, ctx.per_ray, ctx.bg_shape = pack, per_ray, bg_shape
        ctx.car, ctx.beta = float(cos_anneal_ratio), float(logistic_beta)
        ctx.set_materialize_grads(False)
        nd = [rgb_fg, depth, nrm] + ([weights, alpha] if want_weights else [])
        ctx.mark_non_differentiable(*nd)
        return rgb_out, rgb_fg, wsum, depth, nrm, weights, alpha

    @staticmethod
    def backward(ctx, g_rgb, _g_fg, g_wsum, _g_depth, _g_nrm, _g_w, _g_a):
        sdf, sdf_grad, dirs, rgb, bg, wsum = ctx.saved_tensors
        pack, ctx.pack = ctx.pack, None
        N = pack.get_nr_rays()
        g_sdf, g_grad, g_rgb_s = torch.empty_like(sdf), torch.empty_like(sdf_grad), torch.empty_like(rgb)
        scratch = torch.empty(2 * rgb.shape[0], device=rgb.device)
        g_rgb, g_bg = composite_grad_buffers(pack, g_rgb, bg, ctx.needs_input_grad[5])
        _lib.call("vsa_neus_composite_bwd", pack.ray_start_end_idx, sdf, sdf_grad, dirs, pack.samples_dt, rgb, bg,
                  ctx.per_ray, ctx.car, ctx.beta, wsum, g_rgb, None if g_wsum is None else g_wsum.contiguous(), g_sdf,
                  g_grad, g_rgb_s, g_bg, scratch, N, bool(VolumeRendering.bug_compat), _lib.stream_ptr())
        return None, g_sdf, g_grad, None, g_rgb_s, composite_bg_grad(ctx, g_bg), None, None, None


def neus_composite(pack, sdf, sdf_grad, normals, rgb, rgb_bg=None, cos_anneal_ratio=1.0, logistic_beta=2048.0,
                   return_weights=False):
    """render_fg_volumetric (surf.py:357-433) from the samples' sdf [S,1], sdf_grad [S,3], normals [S,3] and rgb
    [S,3] on a compacted pack with dt, and render_rays' blend with rgb_bg [N,3], one colour or None (rgb = rgb_fg).
    Returns a dict: rgb, rgb_fg, normals [N,3], weights_sum, bg_transmittance = 1 - weights_sum, depth [N,1];
    weights and alpha [S,1] (or None).  Downstream of alpha bit-identical to the chain of
    CumprodOneMinusAlphaToTransmittanceFunc, SumOverRaysFunc and IntegrateWithWeights*Func
    (tests/test_surf_render.py)."""
    out = _NeusComposite.apply(pack, sdf.reshape(-1, 1), sdf_grad, normals, rgb, rgb_bg, cos_anneal_ratio,
                               logistic_beta, bool(return_weights))
    rgb_out, rgb_fg, wsum, depth, nrm, weights, alpha = out
    return {"rgb": rgb_out, "rgb_fg": rgb_fg, "weights_sum": wsum, "bg_transmittance": 1 - wsum.detach(),
            "depth": depth, "normals": nrm, "weights": weights, "alpha": alpha}


@torch.no_grad()
def sdf_coarse_cdf(pack, sdf, logistic_beta):
    """One round of importance_sampling_sdf (sdf_utils.py:87-109) from the pack's SDF [S,1] to the CDF [S,1] in one
    launch (vsa_sdf_coarse_cdf); `logistic_beta` is the fp32 value the chain multiplies by.  Bit-identical to the
    chain of single ops."""
    sdf = _lib.check_f32(sdf.contiguous())
    if sdf.numel() != pack.samples_dt.numel():
        raise _lib.VolsurfsHipError("sdf_coarse_cdf: one sdf per sample")
    cdf = torch.empty(sdf.numel(), 1, device=sdf.device)
    _lib.call("vsa_sdf_coarse_cdf", pack.ray_start_end_idx, sdf, pack.samples_dt, float(logistic_beta), cdf,
              pack.get_nr_rays(), _lib.stream_ptr())
    return cdf


def _sdf_column(res):
    sdf = res[0] if isinstance(res, tuple) else res
    return sdf[:, 0:1] if sdf.shape[1] > 1 else sdf


def importance_sampling_sdf(sdf_fn, pack_uniform, iter_nr, nr_samples, logistic_beta_value, min_dist_between_samples,
                            jitter_samples=False):
    """sdf_utils.py:40-175 -> (imp_1, imp_2): importance_sampling_sdf_rounds on the one SDF column, the coarse CDF
    of each round the fused kernel."""
    values_fn = lambda p: _sdf_column(sdf_fn(p) if iter_nr is None else sdf_fn(p, iter_nr))
    return importance_sampling_sdf_rounds(values_fn, sdf_coarse_cdf, 1, pack_uniform, nr_samples, logistic_beta_value,
                                          min_dist_between_samples, jitter_samples)


def get_rays_samples_packed_sdf(rays_o, rays_d, t_near, t_far, sdf_fn, logistic_beta_value, occupancy_grid=None,
                                iter_nr=None, min_dist_between_samples=1e-4, min_nr_samples_per_ray=1,
                                max_nr_samples_per_ray=64, max_nr_imp_samples_per_ray=32, jitter_samples=False,
                                importance_sampling=True, values_dim=1):
    """sdf_utils.py:178-281 -> (pack with dt, importance pack or None)."""
    imp_fn = (lambda pack: VolumeRendering.combine_ray_samples_packets(
        *importance_sampling_sdf(sdf_fn, pack, iter_nr, max_nr_imp_samples_per_ray, logistic_beta_value,
                                 min_dist_between_samples, jitter_samples),
        min_dist_between_samples)) if importance_sampling else None
    return get_rays_samples_packed(rays_o, rays_d, t_near, t_far, imp_fn, occupancy_grid, min_dist_between_samples,
                                   min_nr_samples_per_ray, max_nr_samples_per_ray, jitter_samples, values_dim)


class Surf(FieldMethod):
    """methods/surf.py:34-1128 (volumetric rendering, and the sphere-traced render of the zero level set when
    `render_sphere_traced` is set; the Lipschitz MLP, colour calibration and train_appearance_only are not
    implemented).  models = {"sdf": SDF, "rgb": ColorSH or RGB,
    "bg": NerfHash or None (with a constant bg_color [3])}; the occupancy grid of init_occupancy_grid.  Trains
    through trainer.train_step / train: `method(rays_o, rays_d, gt_rgb, gt_mask, iter_nr)` returns (losses, info,
    foreground samples or None during the sphere init)."""

    method_name = "surf"
    RENDER_KEYS = FieldMethod.RENDER_KEYS + ("normals",)
    RENDER_MODES = ("volumetric", "sphere_traced")
    render_sphere_traced = False           # render_rays adds renders["sphere_traced"] outside training
    SPHERE_TRACED_MAX_STEPS, SPHERE_TRACED_THRESH = 100, 1e-3    # render_rays' call (surf.py:735-741)
    SPHERE_INIT_NR_POINTS = 30000          # surf.py:905
    SPHERE_INIT_EIKONAL_WEIGHT = 1e-3      # surf.py:927

    def __init__(self, train, hyper_params, load_checkpoints_path, save_checkpoints_path, bounding_primitive,
                 bg_color=None, start_iter_nr=0, init_sphere_radius=None):
        hp = hyper_params
        if (start_iter_nr == 0 or start_iter_nr < hp.init_phase_end_iter) and init_sphere_radius is None:
            raise ValueError("init_sphere_radius must be given when training starts in the sphere-init phase "
                             f"(start_iter_nr {start_iter_nr} < init_phase_end_iter {hp.init_phase_end_iter})")
        bb = self._init_common(train, hp, load_checkpoints_path, save_checkpoints_path, bounding_primitive, bg_color)
        self.variance = hp.first_phase_variance_end_value
        self.cos_anneal_ratio = 1.0
        self.in_process_of_sphere_init = False
        self.just_started_first_phase = False
        self.init_sphere_radius = init_sphere_radius
        self.models["sdf"] = SDF(in_channels=3, geom_feat_size=hp.geom_feat_size, mlp_layers_dims=hp.sdf_mlp_layers_dims,
                                 encoding_type=hp.sdf_encoding_type, nr_iters_for_c2f=hp.sdf_nr_iters_for_c2f,
                                 bb_sides=bb)
        self.models["rgb"] = self._rgb_model(bb)
        self.models["bg"] = self._background_model()
        self._load_and_init_optim(train, start_iter_nr)
        self.update_method_state(iter_nr=start_iter_nr)
        self.update_occupancy_grid(iter_nr=start_iter_nr)

    # ---- optimisation (surf.py:178-244)
    def collect_opt_params(self):
        lr, m = self.hyper_params.lr, self.models
        groups = [{"params": list(m["sdf"].pos_encoder.parameters()), "weight_decay": 0.0, "lr": lr,
                   "name": "sdf_pos_encoder"},
                  {"params": list(m["sdf"].mlp_sdf.parameters()), "weight_decay": 0.0, "lr": lr, "name": "sdf_mlp_sdf"},
                  {"params": list(m["rgb"].pos_encoder.parameters()), "weight_decay": 0.0, "lr": lr,
                   "name": "rgb_pos_encoder"},
                  {"params": list(m["rgb"].mlp.parameters()), "weight_decay": 0.0, "lr": lr, "name": "rgb_mlp"}]
        if m["bg"] is not None:
            groups.append({"params": list(m["bg"].parameters()), "weight_decay": 0.0, "lr": lr, "name": "bg"})
        return [g for g in groups if g["params"]]

    # ---- occupancy grid (surf.py:246-302): |sdf|, decay 0
    def update_occupancy_grid(self, iter_nr=None, decay=0.0):
        self._update_sdf_occupancy(self.models["sdf"].main_sdf, torch.abs, iter_nr, decay)

    # ---- phases (surf.py:789-864)
    def update_method_state(self, iter_nr):
        hp = self.hyper_params
        start, end = hp.init_phase_end_iter, hp.first_phase_end_iter
        self.in_process_of_sphere_init = iter_nr < start
        self.just_started_first_phase = iter_nr == start
        if self.is_training and hp.use_occupancy_grid and iter_nr % self.OCCUPANCY_EVERY == 0:
            self.update_occupancy_grid(iter_nr=iter_nr)
        if self.in_process_of_sphere_init:
            return
        self.cos_anneal_ratio = map_range_val(iter_nr, start, end, 0.0, 1.0)
        self.variance = map_range_val(iter_nr, start, end, hp.first_phase_variance_start_value,
                                      hp.first_phase_variance_end_value)
        if self.just_started_first_phase:
            self.update_occupancy_grid(iter_nr)
            if self.is_training and self.lr_scheduler is None and self.scheduler_lr_decay is not None:
                self._install_warmup()

    # ---- rendering (surf.py:305-787)
    def render_fg_volumetric(self, pack, logistic_beta_value=2048.0, cos_anneal_ratio=1.0, iter_nr=None,
                             override=None, rgb_bg=None):
        """-> (renders dict, samples_3d, samples_sdf_grad).  The SDF, its features and its finite-difference
        gradient come from ONE evaluation of the 4-point stencil; `rgb_bg` folds render_rays' blend into the
        composite launch."""
        N = pack.get_nr_rays()
        dev = pack.ray_o.device
        if pack.is_empty():
            r = self._zero_renders(N, dev, rgb_bg, {"rgb_fg": (3,), "depth_fg": (1,), "weights_sum": (1,),
                                                     "normals": (3,)})
            return r, None, torch.zeros(N, 3, device=dev)
        samples_3d = pack.samples_3d
        S = samples_3d.shape[0]
        sdf_full, feat_full = field_stencil(self.models["sdf"].forward, samples_3d, iter_nr)
        sdf, geom_feat = sdf_full[:S], None if feat_full is None else feat_full[:S]
        sdf_grad = stencil_gradients(sdf_full)
        normals = F.normalize(sdf_grad, dim=1)
        dirs = pack.samples_dirs
        view_dir = (override or {}).get("view_dir")
        if view_dir is not None:
            dirs = torch.as_tensor(view_dir, dtype=torch.float32, device=dev).view(1, 3).expand(S, 3).contiguous()
        rgb = self.models["rgb"](points=samples_3d, samples_dirs=dirs, normals=normals, iter_nr=iter_nr,
                                 geom_feat=geom_feat)
        c = neus_composite(pack, sdf, sdf_grad, normals.detach(), rgb, rgb_bg, cos_anneal_ratio, logistic_beta_value)
        r = {"rgb": c["rgb"], "rgb_fg": c["rgb_fg"], "depth_fg": c["depth"], "weights_sum": c["weights_sum"],
             "bg_transmittance": c["bg_transmittance"], "normals": c["normals"],
             "nr_samples": pack.get_nr_samples_per_ray().view(-1, 1).int()}
        return r, samples_3d, sdf_grad

    @torch.no_grad()
    def render_fg_sphere_traced(self, raycast, max_st_steps, converged_dist_tresh, iter_nr=None):
        """surf.py:551-645 -> (renders, points of the hits [H,3] or None, samples_sdf_grad [N,3]); renders = rgb_fg,
        depth_fg, weights_sum (1 on a hit), bg_transmittance, normals.  The zero level set is found by
        sphere_trace's rounds; the hits' features and finite-difference gradient come from ONE evaluation of the
        4-point stencil, their colour from models["rgb"] with the ray direction, the normal and the feature."""
        from .sphere_trace import _trace, scatter_rows
        N, rays_d = raycast["nr_rays"], raycast["rays_d"]
        res = _trace(self.models["sdf"].main_sdf, raycast["rays_o"], rays_d, raycast["points_near"],
                     self.bounding_primitive, [None], max_st_steps, converged_dist_tresh, 1.0, iter_nr, False)
        H = res.hits_per_slot()[0]
        hit = res.hit[0]
        weights_sum = hit.float().unsqueeze(1)
        dev = rays_d.device
        zeros = lambda c: torch.zeros(N, c, device=dev)
        points, normals, grads, depth, rgb_fg = None, zeros(3), zeros(3), zeros(1), zeros(3)
        if H > 0:
            items = res.hit_items[:H].long()
            points = res.points[0].index_select(0, items)
            sdf_full, feat_full = field_stencil(self.models["sdf"].main_sdf, points, iter_nr)
            grad_hit = stencil_gradients(sdf_full)
            normals_hit = F.normalize(grad_hit, dim=1)
            rgb_hit = self.models["rgb"](points=points, samples_dirs=rays_d.index_select(0, items),
                                         normals=normals_hit, iter_nr=iter_nr,
                                         geom_feat=None if feat_full is None else feat_full[:H])
            sc = lambda rows: scatter_rows(res.hit_items, H, rows, N)
            normals, grads, rgb_fg = sc(normals_hit), sc(grad_hit), sc(rgb_hit)
            depth = sc(res.z[0].index_select(0, items).unsqueeze(1))
        renders = {"rgb_fg": rgb_fg, "depth_fg": depth, "weights_sum": weights_sum,
                   "bg_transmittance": 1 - weights_sum, "normals": normals}
        return renders, points, grads

    def render_rays(self, rays_o, rays_d, iter_nr=None, override=None, **kwargs):
        """The reference's dict: {"renders": {"volumetric": {rgb, rgb_fg, rgb_bg, depth_fg, depth_bg, depth,
        weights_sum, bg_transmittance, normals, nr_samples}}, "samples_3d", "samples_grad"}.  `override` takes
        "variance", "cos_anneal_ratio" and "view_dir".  With `render_sphere_traced` set and outside training,
        "renders" also holds "sphere_traced": render_fg_sphere_traced's entries (100 rounds, 1e-3) with rgb_bg,
        depth_bg and rgb = rgb_fg + bg_transmittance rgb_bg, depth composed as the volumetric entry's (the
        reference computes this render and has the blend commented out, which leaves it without an `rgb`)."""
        hp = self.hyper_params
        override = override or {}
        raycast = intersect_bounding_primitive(self.bounding_primitive, rays_o, rays_d)
        variance = override.get("variance")
        beta = get_logistic_beta_from_variance(self.variance if variance is None else variance)
        pack, _ = get_rays_samples_packed_sdf(
            rays_o, rays_d, raycast["t_near"], raycast["t_far"], self.models["sdf"], beta, self.occupancy_grid,
            iter_nr, hp.min_dist_between_samples, hp.min_nr_samples_per_ray, hp.max_nr_samples_per_ray,
            hp.max_nr_imp_samples_per_ray, jitter_samples=self.is_training, importance_sampling=hp.do_importance_sampling)
        car = override.get("cos_anneal_ratio")
        car = self.cos_anneal_ratio if car is None else car
        rgb_bg, blend_bg, depth_bg = self._render_bg(raycast, iter_nr)
        if depth_bg is None:
            depth_bg = raycast["t_far"]
        renders, samples_3d, samples_grad = self.render_fg_volumetric(pack, beta, car, iter_nr, override, blend_bg)
        renders["rgb_bg"] = rgb_bg
        renders["depth_bg"] = depth_bg
        renders["depth"] = renders["depth_fg"] * renders["weights_sum"] + depth_bg * renders["bg_transmittance"]
        all_renders = {"volumetric": renders}
        if self.render_sphere_traced and not self.is_training:
            st, _, _ = self.render_fg_sphere_traced(raycast, self.SPHERE_TRACED_MAX_STEPS, self.SPHERE_TRACED_THRESH,
                                                    iter_nr)
            st["rgb_bg"], st["depth_bg"] = rgb_bg, depth_bg
            st["rgb"] = st["rgb_fg"] + st["bg_transmittance"] * rgb_bg
            st["depth"] = st["depth_fg"] * st["weights_sum"] + depth_bg * st["bg_transmittance"]
            all_renders["sphere_traced"] = st
        return {"renders": all_renders, "samples_3d": samples_3d, "samples_grad": samples_grad}

    # ---- training (surf.py:866-1128)
    def _sphere_init_losses(self):
        r = self.init_sphere_radius
        with torch.no_grad():
            points = self.bounding_primitive.get_random_points_inside(self.SPHERE_INIT_NR_POINTS)
            sdf_gt = (points.norm(dim=-1) - r).unsqueeze(-1)
        # main_sdf(points) and get_field_gradients(main_sdf, points) of surf.py:912-921 share one stencil call
        sdf_full = field_stencil(self.models["sdf"].main_sdf, points)[0]
        sdf_pred, sdf_grad = sdf_full[:points.shape[0]], stencil_gradients(sdf_full)
        loss_sdf = ((sdf_pred - sdf_gt) ** 2).mean()
        loss_eikonal = ((sdf_grad.norm(dim=-1) - 1) ** 2).mean()
        return loss_sdf + loss_eikonal * self.SPHERE_INIT_EIKONAL_WEIGHT, loss_sdf, loss_eikonal

    def forward(self, rays_o, rays_d, gt_rgb, gt_mask=None, iter_nr=0, is_first_iter=False, is_training_masked=None,
                **kwargs):
        hp = self.hyper_params
        masked = hp.is_training_masked if is_training_masked is None else is_training_masked
        loss_sdf = loss_eikonal = loss_rgb = loss_curvature = loss_offsurface = loss_mask = 0.0
        self.update_method_state(iter_nr)
        samples_3d = None
        if self.in_process_of_sphere_init:
            loss, loss_sdf, loss_eikonal = self._sphere_init_losses()
        else:
            res = self.render_rays(rays_o, rays_d, iter_nr=iter_nr)
            samples_3d, samples_grad = res["samples_3d"], res["samples_grad"]
            loss_rgb, pred_mask = self._loss_rgb(res["renders"]["volumetric"], gt_rgb, gt_mask, masked)
            loss = loss_rgb
            r_sdf, r_grad = self._random_points_stencil(self.models["sdf"].main_sdf, iter_nr)
            has_samples = samples_3d is not None and samples_3d.shape[0] > 0
            if hp.eikonal_weight > 0.0:
                loss_eikonal = self._loss_eikonal(r_grad, samples_grad if has_samples else None, hp.eikonal_weight)
                loss = loss + loss_eikonal
            if hp.offsurface_weight > 0.0:
                loss_offsurface = self._loss_offsurface(r_sdf)
                loss = loss + loss_offsurface
            w_curv = curvature_weight_schedule(iter_nr, hp.reduce_curv_start_iter, hp.reduce_curv_end_iter)
            if hp.curvature_weight > 0.0 and w_curv > 0.0 and has_samples:
                curv = get_sdf_curvature(self.models["sdf"].main_sdf, samples_3d, samples_grad,
                                         torch.randn_like(samples_3d), iter_nr=iter_nr)
                loss_curvature = curv.mean() * hp.curvature_weight * w_curv
                loss = loss + loss_curvature
            if masked and hp.mask_weight > 0.0:
                loss_mask = self._loss_mask(pred_mask, gt_mask)
                loss = loss + loss_mask
        losses = {"loss": loss, "sdf": loss_sdf, "eikonal": loss_eikonal, "rgb": loss_rgb,
                  "curvature": loss_curvature, "lipshitz": 0.0, "offsurface_high_sdf": loss_offsurface,
                  "mask": loss_mask}
        info = {"stdev": logistic_distribution_stdev(get_logistic_beta_from_variance(self.variance))}
        return losses, info, samples_3d
