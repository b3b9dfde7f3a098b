"""The OffsetsSurfs method (volsurfs_py/methods/offsets_surfs.py, config/offsets_surfs/base_5.cfg,
models/offsets_sdf.py, utils/offsets_utils.py, utils/sdfs_utils.py): K nested surfaces, the zero levels of a main
SDF shifted by learned, spatially varying offsets, each with its own colour and transparency, trained from posed
images starting from a `surf` run's `sdf.pt`.  Its meshes (`isosurface.extract_offsets_surfs_meshes`) are the shells
the VolSurfs stages take.

The per-ray chains run as fused HIP kernels (csrc/offsets_render.hip): the K NeuS composites with the dense blend
of the shells and the background (`offsets_composite`) and one importance round over K CDFs (`sdfs_coarse_cdf`).
The rest is the project's existing HIP operators and the Surf method's helpers."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .background import intersect_bounding_primitive
from .field_method import (FieldMethod, bg_arg, composite_bg_grad, composite_grad_buffers, eikonal_loss,
                           field_stencil, get_logistic_beta_from_variance, get_rays_samples_packed,
                           importance_sampling_sdf_rounds, stencil_gradients)
from .models import OffsetsSDF
from .surf import SurfHyperParams, get_sdfs_curvature, logistic_distribution_stdev, map_range_val
from .volsurfs import VolumeRendering

MAX_SURFS = 16          # csrc/offsets_render.hip OR_MAX_SURFS


class OffsetsSurfsHyperParams(SurfHyperParams):
    """params/hyper_params.py (HyperParamsOffsetsSuRFs) with config/offsets_surfs/base_5.cfg applied.  Keyword
    arguments override single values; what Surf does not implement raises here too."""

    def set_defaults(self):
        super().set_defaults()
        # base_5.cfg
        self.init_phase_end_iter = 2000
        self.color_init_phase_end_iter = 3000
        self.nr_warmup_iters = 1000
        self.lr_milestones = [40000, 45000, 47500]
        self.nr_inner_surfs = 4
        self.nr_outer_surfs = 0
        self.delta_surfs_multiplier = 1.0
        self.training_end_iter = 50000
        self.first_phase_end_iter = 45000
        self.first_phase_stop_main_surf = False
        self.first_phase_variance_start_value = 0.7
        self.first_phase_variance_end_value = 1.0
        self.sdf_nr_iters_for_c2f = 0
        self.rgb_nr_iters_for_c2f = 0
        self.appearance_predict_sh_coeffs = False
        self.min_nr_samples_per_ray = 1
        # HyperParamsOffsetsSuRFs
        self.are_surfs_colors_indep = False
        self.are_surfs_transparency_indep = False
        self.is_inner_surf_solid = False
        self.transp_view_dep = True
        self.transp_normal_dep = True
        self.transp_geom_feat_dep = True
        self.offsets_weight = 0.0
        self.support_surfs_eikonal_weight = 0.04
        self.with_alpha_decay = True

    def validate(self):
        super().validate()
        if self.nr_inner_surfs + self.nr_outer_surfs + 1 > MAX_SURFS:
            raise _lib.VolsurfsHipError(f"at most {MAX_SURFS} surfaces")


def get_offsets_gt(nr_outer_surfs, nr_inner_surfs, delta_surfs, main_surf_shift=0.0):
    """utils/offsets_utils.py:4-21: [inner offsets, largest first, then outer ones] (float64, as the reference's
    tensor of numpy float64 values; an empty float32 tensor for K = 1)."""
    outer, cur = [], main_surf_shift
    for _ in range(nr_outer_surfs):
        cur -= delta_surfs
        outer.append(cur)
    inner, cur = [], main_surf_shift
    for _ in range(nr_inner_surfs):
        cur += delta_surfs
        inner.append(cur)
    vals = inner[::-1] + outer
    return (torch.tensor(vals, dtype=torch.float64) if vals else torch.tensor([])) - main_surf_shift


# ---- fused per-ray chains (csrc/offsets_render.hip)
class _OffsetsComposite(torch.autograd.Function):
    """render_fg_volumetric's K NeuS chains and the blend, and render_rays' background, as one launch each way
    (vsa_offsets_composite_fwd / _bwd).  Differentiable inputs: sdfs, sdfs_grad, rgb, transparency, rgb_bg;
    differentiable output: rgb.  The other outputs carry no gradient."""

    @staticmethod
    def forward(ctx, pack, sdfs, sdfs_grad, normals, rgb, transparency, rgb_bg, car, beta, decay, want_alpha):
        sdfs = _lib.check_f32(sdfs.contiguous())
        S, K = sdfs.shape
        N = pack.get_nr_rays()
        if K < 1 or K > MAX_SURFS:
            raise _lib.VolsurfsHipError(f"offsets composite: 1 <= K <= {MAX_SURFS} surfaces, got {K}")
        sdfs_grad = _lib.check_f32(sdfs_grad.contiguous())
        normals = _lib.check_f32(normals.contiguous())
        rgb = _lib.check_f32(rgb.contiguous())
        ctx.tr_shape = transparency.shape
        transparency = _lib.check_f32(transparency.reshape(S, K).contiguous())
        if sdfs_grad.shape != (S, K, 3) or normals.shape != (S, K, 3) or rgb.shape != (S, K, 3) or \
                pack.samples_dt.numel() != S:
            raise _lib.VolsurfsHipError("offsets composite: sdfs [S,K], sdfs_grad / normals / rgb [S,K,3], "
                                        "transparency [S,K], a pack with dt")
        bg, per_ray, bg_shape = bg_arg(rgb_bg, N, "neus")
        dev = sdfs.device
        e = lambda *s: torch.empty(*s, device=dev)
        s_rgb, s_nrm, s_depth, s_ws = e(N, K, 3), e(N, K, 3), e(N, K, 1), e(N, K, 1)
        s_alpha, s_T, s_bw = e(N, K, 1), e(N, K, 1), e(N, K, 1)
        rgb_fg, bgT, rgb_out = e(N, 3), e(N, 1), e(N, 3)
        alpha = e(S, K) if want_alpha else None
        dirs = pack.samples_dirs.contiguous()
        with_decay = decay is not None
        _lib.call("vsa_offsets_composite_fwd", pack.ray_start_end_idx, K, sdfs, sdfs_grad, normals, rgb,
                  transparency, dirs, pack.samples_dt, pack.samples_z, bg, per_ray, float(car), float(beta),
                  int(with_decay), float(decay) if with_decay else 0.0, s_rgb, s_nrm, s_depth, s_ws, s_alpha, s_T,
                  s_bw, rgb_fg, bgT, rgb_out, alpha, N, _lib.stream_ptr())
        ctx.save_for_backward(sdfs, sdfs_grad, normals, rgb, transparency, dirs, bg, s_rgb, s_alpha, s_T, bgT)
        ctx.pack, ctx.per_ray, ctx.bg_shape = pack, per_ray, bg_shape
        ctx.car, ctx.beta, ctx.decay = float(car), float(beta), decay
        ctx.set_materialize_grads(False)
        nd = [rgb_fg, bgT, s_rgb, s_nrm, s_depth, s_ws, s_alpha, s_T, s_bw] + ([alpha] if want_alpha else [])
        ctx.mark_non_differentiable(*nd)
        return (rgb_out, *nd, *([] if want_alpha else [None]))

    @staticmethod
    def backward(ctx, g_rgb, *_):
        sdfs, sdfs_grad, normals, rgb, transparency, dirs, bg, s_rgb, s_alpha, s_T, bgT = ctx.saved_tensors
        pack, ctx.pack = ctx.pack, None
        N = pack.get_nr_rays()
        S, K = sdfs.shape
        g_sdfs, g_grad, g_rgb_s = torch.empty_like(sdfs), torch.empty_like(sdfs_grad), torch.empty_like(rgb)
        g_t = torch.empty_like(transparency)
        scratch = torch.empty(2 * S * K, device=sdfs.device)
        d = ctx.decay
        g_rgb, g_bg = composite_grad_buffers(pack, g_rgb, bg, ctx.needs_input_grad[6])
        _lib.call("vsa_offsets_composite_bwd", pack.ray_start_end_idx, K, sdfs, sdfs_grad, normals, rgb,
                  transparency, dirs, pack.samples_dt, bg, ctx.per_ray, ctx.car, ctx.beta, int(d is not None),
                  float(d) if d is not None else 0.0, s_rgb, s_alpha, s_T, bgT, g_rgb, g_sdfs, g_grad, g_rgb_s, g_t, g_bg,
                  scratch, N, bool(VolumeRendering.bug_compat), _lib.stream_ptr())
        return (None, g_sdfs, g_grad, None, g_rgb_s, g_t.view(ctx.tr_shape), composite_bg_grad(ctx, g_bg), None, None,
                None, None)


def offsets_composite(pack, sdfs, sdfs_grad, normals, rgb, transparency, rgb_bg=None, cos_anneal_ratio=1.0,
                      logistic_beta=2048.0, alpha_decay_factor=None, return_alpha=False):
    """render_fg_volumetric (offsets_surfs.py:420-713) and render_rays' blend (:983-1005) from the samples' sdfs
    [S,K(,1)], sdfs_grad [S,K,3], normals [S,K,3] (no gradient), rgb [S,K,3] and transparency [S,K(,1)] on a
    compacted pack with dt; rgb_bg [N,3], one colour or None; alpha_decay_factor None = no decay.  Returns the
    reference's buffers inner to outer: surfs_rgb / surfs_normals [N,K,3], surfs_depths / surfs_weight_sum /
    surfs_alpha / surfs_transmittance / surfs_blending_weights [N,K,1], and rgb_fg [N,3], bg_transmittance [N,1],
    rgb [N,3]; with return_alpha the per-sample NeuS alpha [S,K] too.  Per surface bit-identical downstream of
    alpha to the packed ops (tests/test_offsets_surfs_render.py)."""
    S = sdfs.shape[0]
    out = _OffsetsComposite.apply(pack, sdfs.reshape(S, sdfs.shape[1]), sdfs_grad, normals, rgb, transparency, rgb_bg,
                                  cos_anneal_ratio, logistic_beta, alpha_decay_factor, bool(return_alpha))
    rgb_out, rgb_fg, bgT, s_rgb, s_nrm, s_depth, s_ws, s_alpha, s_T, s_bw, alpha = out
    return {"alpha": alpha, "rgb": rgb_out, "rgb_fg": rgb_fg, "bg_transmittance": bgT, "surfs_rgb": s_rgb, "surfs_normals": s_nrm,
            "surfs_depths": s_depth, "surfs_weight_sum": s_ws, "surfs_alpha": s_alpha, "surfs_transmittance": s_T,
            "surfs_blending_weights": s_bw}


@torch.no_grad()
def sdfs_coarse_cdf(pack, sdfs, logistic_beta):
    """One round of importance_sampling_sdfs_iter (sdfs_utils.py:12-64) from the pack's sdfs [S,K(,1)] to the CDF
    [S,1] in one launch (vsa_sdfs_coarse_cdf); `logistic_beta` is the fp32 value the chain multiplies by.
    Bit-identical to the chain of single ops."""
    S = sdfs.shape[0]
    sdfs = _lib.check_f32(sdfs.reshape(S, sdfs.shape[1]).contiguous())
    K = sdfs.shape[1]
    if K < 1 or K > MAX_SURFS:
        raise _lib.VolsurfsHipError(f"sdfs_coarse_cdf: 1 <= K <= {MAX_SURFS} surfaces, got {K}")
    if S != pack.samples_dt.numel():
        raise _lib.VolsurfsHipError("sdfs_coarse_cdf: one row of sdfs per sample")
    cdf = torch.empty(S, 1, device=sdfs.device)
    _lib.call("vsa_sdfs_coarse_cdf", pack.ray_start_end_idx, K, sdfs, pack.samples_dt, float(logistic_beta), cdf,
              pack.get_nr_rays(), _lib.stream_ptr())
    return cdf


def _sdfs_columns(res):
    sdfs = res[0] if isinstance(res, tuple) else res
    return sdfs[..., 0:1] if sdfs.shape[2] > 1 else sdfs


def importance_sampling_sdfs(sdfs_fn, nr_surfs, pack_uniform, iter_nr, nr_imp_samples, logistic_beta_value,
                             min_dist_between_samples, jitter_samples=False):
    """sdfs_utils.py:67-180 -> (imp_1, imp_2): importance_sampling_sdf_rounds on the K SDF columns, each round's CDF
    the fused kernel."""
    values_fn = lambda p: _sdfs_columns(sdfs_fn(p) if iter_nr is None else sdfs_fn(p, iter_nr))
    return importance_sampling_sdf_rounds(values_fn, sdfs_coarse_cdf, nr_surfs, pack_uniform, nr_imp_samples,
                                          logistic_beta_value, min_dist_between_samples, jitter_samples)


def get_rays_samples_packed_sdfs(rays_o, rays_d, t_near, t_far, sdfs_fn, nr_surfs, logistic_beta_value,
                                 occupancy_grid=None, iter_nr=None, min_dist_between_samples=1e-4,
                                 min_nr_samples_per_ray=1, max_nr_samples_per_ray=64, max_nr_imp_samples_per_ray=32,
                                 jitter_samples=False, importance_sampling=True, values_dim=1):
    """sdfs_utils.py:435-510 -> (pack with dt, importance pack or None)."""
    imp_fn = (lambda pack: VolumeRendering.combine_ray_samples_packets(
        *importance_sampling_sdfs(sdfs_fn, nr_surfs, pack, iter_nr, max_nr_imp_samples_per_ray, logistic_beta_value,
                                  min_dist_between_samples, jitter_samples),
        min_dist_between_samples)) if importance_sampling else None
    return get_rays_samples_packed(rays_o, rays_d, t_near, t_far, imp_fn, occupancy_grid, min_dist_between_samples,
                                   min_nr_samples_per_ray, max_nr_samples_per_ray, jitter_samples, values_dim)


def appearance_rows(model, points, dirs, normals, geom_feat, iter_nr=None):
    """One appearance model evaluated ONCE over K S rows (surface-major: the points, directions and features
    repeated, the K surfaces' normals [S,K,3] stacked) -> [S, K, C]: row for row what the reference's K calls
    model(points, dirs, normals[:, k], geom_feat) give."""
    S, K = normals.shape[0], normals.shape[1]
    rep = lambda t: None if t is None else t.repeat(K, 1)
    out = model(points=rep(points), samples_dirs=rep(dirs), normals=normals.transpose(0, 1).reshape(K * S, 3),
                iter_nr=iter_nr, geom_feat=rep(geom_feat))
    return out.reshape(K, S, -1).transpose(0, 1)


class OffsetsSurfs(FieldMethod):
    """methods/offsets_surfs.py:32-1449 (volumetric rendering, and the sphere-traced render of the K surfaces when
    `render_sphere_traced` is set; the debug-ray plot and colour calibration are not implemented).  models = {"sdfs": OffsetsSDF, "rgb" or "rgb_<i>": RGB / ColorSH (3 channels),
    "alpha" or "alpha_<i>": RGB / ColorSH (1 channel) or None for a solid inner shell, "bg": NerfHash or None}.
    Trains through trainer.train_step / train: `method(rays_o, rays_d, gt_rgb, gt_mask, iter_nr)` returns (losses,
    info, foreground samples or None during the offsets init)."""

    method_name = "offsets_surfs"
    RENDER_KEYS = ("rgb", "rgb_fg", "bg_transmittance")
    RENDER_MODES = ("volumetric", "sphere_traced")
    render_sphere_traced = False           # render_rays adds renders["sphere_traced"] outside training
    SPHERE_TRACED_MAX_STEPS, SPHERE_TRACED_THRESH = 100, 1e-3    # render_rays' call (offsets_surfs.py:955-961)
    OFFSETS_INIT_NR_POINTS = 30000         # offsets_surfs.py:1175
    DECAY_START, DECAY_END = 1000.0, 10.0  # alpha_decay_factor over the first phase

    def __init__(self, train, hyper_params, load_checkpoints_path, save_checkpoints_path, bounding_primitive,
                 models_path, bg_color=None, start_iter_nr=0):
        hp = hyper_params
        if models_path is None and start_iter_nr == 0:
            raise ValueError("models_path must be a folder holding the surf method's sdf.pt")
        bb = self._init_common(train, hp, load_checkpoints_path, save_checkpoints_path, bounding_primitive, bg_color)
        stdev = logistic_distribution_stdev(get_logistic_beta_from_variance(hp.first_phase_variance_start_value))
        self.delta_surfs = stdev * hp.delta_surfs_multiplier
        self.offsets_gt = get_offsets_gt(hp.nr_outer_surfs, hp.nr_inner_surfs, self.delta_surfs)
        sdfs = OffsetsSDF(in_channels=3, mlp_layers_dims=hp.sdf_mlp_layers_dims, encoding_type=hp.sdf_encoding_type,
                          nr_inner_surfs=hp.nr_inner_surfs, nr_outer_surfs=hp.nr_outer_surfs,
                          geom_feat_size=hp.geom_feat_size, nr_iters_for_c2f=0, bb_sides=bb)
        self.models["sdfs"] = sdfs
        self.nr_surfs, self.main_surf_idx = sdfs.nr_surfs, sdfs.main_surf_idx
        self.nr_inner_surfs, self.nr_outer_surfs = sdfs.nr_inner_surfs, sdfs.nr_outer_surfs
        self.in_offsets_init = self.in_color_init = self.in_first_phase = self.in_second_phase = False
        self.just_started_offsets_init = self.just_started_color_init = True
        self.just_started_first_phase = self.just_started_second_phase = True
        self.variance = 1.0
        self.cos_anneal_ratio = 1.0
        self.with_alpha_decay = hp.with_alpha_decay
        self.alpha_decay_factor = self.DECAY_START
        for i in range(self.nr_surfs):
            m = self._appearance_model(3, hp.rgb_view_dep, hp.rgb_normal_dep, hp.rgb_geom_feat_dep, bb)
            if hp.are_surfs_colors_indep:
                self.models[f"rgb_{i}"] = m
            else:
                self.models["rgb"] = m
                break
        for i in range(self.nr_surfs):
            m = None if (hp.is_inner_surf_solid and i == 0) else \
                self._appearance_model(1, hp.transp_view_dep, hp.transp_normal_dep, hp.transp_geom_feat_dep, bb)
            if hp.are_surfs_transparency_indep:
                self.models[f"alpha_{i}"] = m
            else:
                self.models["alpha"] = m
                break
        self.models["bg"] = self._background_model()
        self._load_and_init_optim(train, start_iter_nr)
        if models_path is not None and start_iter_nr == 0:
            ckpt = os.path.join(models_path, "sdf.pt")
            if not os.path.exists(ckpt):
                raise FileNotFoundError(f"checkpoint {ckpt} does not exist")
            sdfs.load_main_sdf_ckpt(ckpt)
            if self.models["bg"] is not None:
                ckpt = os.path.join(models_path, "bg.pt")
                if not os.path.exists(ckpt):
                    raise FileNotFoundError(f"checkpoint {ckpt} does not exist")
                self.models["bg"].load_state_dict(torch.load(ckpt, map_location="cuda"))
        self.update_method_state(start_iter_nr)
        self.update_occupancy_grid(iter_nr=start_iter_nr)

    def parameters(self):
        return super().parameters() + self.models["sdfs"].heads_parameters()

    # ---- optimisation (offsets_surfs.py:325-385)
    def collect_opt_params(self):
        lr, m = self.hyper_params.lr, self.models
        s = m["sdfs"]
        groups = [{"params": list(s.pos_encoder.parameters()), "weight_decay": 0.0, "lr": lr, "name": "sdfs_pos_encoder"},
                  {"params": list(s.mlp_sdf.parameters()), "weight_decay": 0.0, "lr": lr, "name": "sdfs_mlp_sdf"}]
        for i, h in enumerate(s.mlps_eps):
            groups.append({"params": list(h.parameters()), "weight_decay": 0.0, "lr": lr, "name": f"sdfs_mlp_eps_{i}"})
        for key, model in m.items():
            if ("rgb" in key or "alpha" in key or "bg" in key) and model is not None:
                groups.append({"params": list(model.parameters()), "weight_decay": 0.0, "lr": lr, "name": key})
        return [g for g in groups if g["params"]]

    # ---- checkpoints: the reference's sdfs.pt (main surface only) plus sdfs_eps_<i>.pt per head
    def save(self, iter_nr):
        path = super().save(iter_nr)
        if path is not None:
            for i, sd in enumerate(self.models["sdfs"].heads_state_dicts()):
                torch.save(sd, os.path.join(path, f"sdfs_eps_{i}.pt"))
        return path

    def load(self, iter_nr):
        path = super().load(iter_nr)
        if path is not None:
            s = self.models["sdfs"]
            files = [os.path.join(path, f"sdfs_eps_{i}.pt") for i in range(len(s.mlps_eps))]
            missing = [f for f in files if not os.path.exists(f)]
            if missing:
                raise FileNotFoundError(f"offset head checkpoint(s) {missing} do not exist")
            s.load_heads_state_dicts([torch.load(f, map_location="cuda") for f in files])
        return path

    # ---- occupancy grid (offsets_surfs.py:387-418): min_k |sdf_k|, decay 0
    def update_occupancy_grid(self, iter_nr=None, decay=0.0):
        self._update_sdf_occupancy(self.models["sdfs"],
                                   lambda sdfs: torch.min(torch.abs(sdfs.squeeze(-1)), dim=-1, keepdim=True)[0],
                                   iter_nr, decay)

    # ---- phases (offsets_surfs.py:1011-1128)
    def update_method_state(self, iter_nr):
        hp = self.hyper_params
        s = self.models["sdfs"]
        off_end, col_end, first_end = hp.init_phase_end_iter, hp.color_init_phase_end_iter, hp.first_phase_end_iter
        self.in_offsets_init = iter_nr < off_end
        self.in_color_init = off_end <= iter_nr < col_end
        self.in_first_phase = col_end <= iter_nr < first_end
        self.in_second_phase = iter_nr >= first_end
        if self.is_training and not self.in_color_init and hp.use_occupancy_grid and \
                iter_nr % self.OCCUPANCY_EVERY == 0:
            self.update_occupancy_grid(iter_nr=iter_nr)
        if self.in_offsets_init and self.is_training and self.just_started_offsets_init:
            s.freeze_main_surf()
            self.cos_anneal_ratio, self.alpha_decay_factor = 1.0, self.DECAY_START
            self.variance = hp.first_phase_variance_start_value
            self.update_occupancy_grid(iter_nr)
            self.just_started_offsets_init = False
        if self.in_color_init and self.is_training and self.just_started_color_init:
            s.freeze_main_surf()
            s.freeze_offsets()
            self.cos_anneal_ratio, self.alpha_decay_factor = 1.0, self.DECAY_START
            self.variance = hp.first_phase_variance_start_value
            self.update_occupancy_grid(iter_nr)
            self.just_started_color_init = False
        if self.in_first_phase:
            if self.is_training and self.just_started_first_phase:
                s.unfreeze_main_surf()
                s.unfreeze_offsets()
                self.update_occupancy_grid(iter_nr)
                if self.lr_scheduler is None and self.scheduler_lr_decay is not None:
                    self._install_warmup()
                self.just_started_first_phase = False
            self.cos_anneal_ratio = 1.0
            self.variance = map_range_val(iter_nr, col_end, first_end, hp.first_phase_variance_start_value,
                                          hp.first_phase_variance_end_value)
            self.alpha_decay_factor = map_range_val(iter_nr, col_end, first_end, self.DECAY_START, self.DECAY_END)
        if self.in_second_phase and self.is_training and self.just_started_second_phase:
            s.unfreeze_main_surf()
            s.unfreeze_offsets()
            self.update_occupancy_grid(iter_nr)
            self.just_started_second_phase = False
            self.cos_anneal_ratio = 1.0
            self.variance = hp.first_phase_variance_end_value
            self.alpha_decay_factor = self.DECAY_END

    # ---- rendering (offsets_surfs.py:420-1009)
    def render_appearance(self, samples_3d, dirs, normals, geom_feat, iter_nr=None):
        """-> (rgb [S,K,3], transparency [S,K,1]): a shared model evaluated once over K S rows, independent models
        once per surface; a solid inner shell's transparency is 1."""
        hp = self.hyper_params
        S, K = samples_3d.shape[0], self.nr_surfs
        out = []
        for kind, C, indep in (("rgb", 3, hp.are_surfs_colors_indep), ("alpha", 1, hp.are_surfs_transparency_indep)):
            ones = lambda: torch.ones(S, C, device=samples_3d.device)
            if not indep:
                m = self.models[kind]
                out.append(appearance_rows(m, samples_3d, dirs, normals, geom_feat, iter_nr) if m is not None
                           else ones().unsqueeze(1).expand(S, K, C))
                continue
            cols = []
            for i in range(K):
                m = self.models[f"{kind}_{i}"]
                cols.append(ones() if m is None else m(points=samples_3d, samples_dirs=dirs, normals=normals[:, i],
                                                       iter_nr=iter_nr, geom_feat=geom_feat))
            out.append(torch.stack(cols, 1))
        return out[0], out[1]

    def _empty_renders(self, N, dev, rgb_bg):
        K = self.nr_surfs
        r = self._zero_renders(N, dev, rgb_bg, {
            "surfs_rgb": (K, 3), "surfs_normals": (K, 3), "surfs_depths": (K, 1), "surfs_weight_sum": (K, 1),
            "surfs_alpha": (K, 1), "surfs_blending_weights": (K, 1), "rgb_fg": (3,)})
        r["surfs_transmittance"] = torch.ones(N, K, 1, device=dev)
        return r

    def render_fg_volumetric(self, pack, logistic_beta_value=2048.0, cos_anneal_ratio=1.0, iter_nr=None,
                             rgb_bg=None):
        """-> (renders dict, samples_3d, samples_sdfs_grad [S,K,3]).  The sdfs, their features and their
        finite-difference gradients come from ONE evaluation of the 4-point stencil; `rgb_bg` folds render_rays'
        blend into the composite launch."""
        N = pack.get_nr_rays()
        dev = pack.ray_o.device
        if pack.is_empty():
            return self._empty_renders(N, dev, rgb_bg), None, None
        samples_3d = pack.samples_3d
        S = samples_3d.shape[0]
        sdfs_full, _, feat_full = field_stencil(self.models["sdfs"].forward, samples_3d, iter_nr)
        sdfs, geom_feat = sdfs_full[:S], None if feat_full is None else feat_full[:S]
        sdfs_grad = stencil_gradients(sdfs_full)                         # [S, K, 3]
        normals = F.normalize(sdfs_grad, dim=-1)
        dirs = pack.samples_dirs
        rgb, transp = self.render_appearance(samples_3d, dirs, normals, geom_feat, iter_nr)
        decay = float(self.alpha_decay_factor) if self.with_alpha_decay else None
        r = offsets_composite(pack, sdfs, sdfs_grad, normals.detach(), rgb, transp, rgb_bg, cos_anneal_ratio,
                              logistic_beta_value, decay)
        r.pop("alpha")
        r["nr_samples"] = pack.get_nr_samples_per_ray().view(-1, 1).int()
        return r, samples_3d, sdfs_grad

    def _surface_model(self, kind, indep, i):
        return self.models[f"{kind}_{i}"] if indep else self.models[kind]

    @torch.no_grad()
    def render_fg_sphere_traced(self, raycast, max_st_steps, converged_dist_tresh, iter_nr=None):
        """offsets_surfs.py:687-890 -> (renders, samples_3d, samples_sdf, samples_sdf_grad); renders = surfs_rgb
        [N,K,3], surfs_alpha, surfs_depths [N,K,1], surfs_normals [N,K,3], surfs_transmittance,
        surfs_blending_weights [N,K,1] (surfaces inner to outer), rgb_fg [N,3], bg_transmittance [N,1].  The K
        surfaces are traced as one batch of N K items (sphere_trace_columns' loop: an int surf_idx of the reference
        read as that column); the hits of all surfaces share one stencil evaluation, a shared appearance model one
        call; the blend is one launch.  The samples are the hits surface after surface, inner first."""
        from .sphere_trace import _trace, blend_surfaces, scatter_rows
        hp = self.hyper_params
        N, K, rays_d = raycast["nr_rays"], self.nr_surfs, raycast["rays_d"]
        dev = rays_d.device
        res = _trace(self.models["sdfs"], raycast["rays_o"], rays_d, raycast["points_near"],
                     self.bounding_primitive, list(range(K)), max_st_steps, converged_dist_tresh, 1.0, iter_nr, False)
        per_slot = res.hits_per_slot()
        H = sum(per_slot)
        z = lambda c: torch.zeros(N, K, c, device=dev)
        surfs_rgb, surfs_alpha, surfs_depths, surfs_normals = z(3), z(1), z(1), z(3)
        samples_3d = samples_sdf = samples_grad = None
        if H > 0:
            items = res.hit_items[:H].long()
            slot, ray = items // N, items % N
            samples_3d = res.points.reshape(N * K, 3).index_select(0, items)
            dirs = rays_d.index_select(0, ray)
            sdfs_full, _, feat_full = field_stencil(self.models["sdfs"].forward, samples_3d, iter_nr)
            samples_sdf = sdfs_full[:H]
            feat = None if feat_full is None else feat_full[:H]
            grads_all = stencil_gradients(sdfs_full).reshape(H, K, 3)
            samples_grad = grads_all[torch.arange(H, device=dev), slot]
            normals = F.normalize(samples_grad, dim=1)
            ends = np.cumsum([0] + per_slot)
            rows = {}
            for kind, C, indep in (("rgb", 3, hp.are_surfs_colors_indep), ("alpha", 1, hp.are_surfs_transparency_indep)):
                spans = [(ends[i], ends[i + 1], i) for i in range(K)] if indep else [(0, H, 0)]
                out = torch.ones(H, C, device=dev)
                for a, b, i in spans:
                    m = self._surface_model(kind, indep, i)
                    if m is not None and b > a:
                        out[a:b] = m(points=samples_3d[a:b], samples_dirs=dirs[a:b], normals=normals[a:b],
                                     iter_nr=iter_nr, geom_feat=None if feat is None else feat[a:b])
                rows[kind] = out
            sc = lambda r: scatter_rows(res.hit_items, H, r, N, K).reshape(N, K, -1)
            surfs_rgb, surfs_alpha, surfs_normals = sc(rows["rgb"]), sc(rows["alpha"]), sc(normals)
            surfs_depths = sc(res.z.reshape(N * K).index_select(0, items).unsqueeze(1))
        T, w, rgb_fg, bg_T = blend_surfaces(surfs_rgb, surfs_alpha)
        renders = {"surfs_rgb": surfs_rgb, "surfs_alpha": surfs_alpha, "surfs_depths": surfs_depths,
                   "surfs_normals": surfs_normals, "surfs_transmittance": T, "surfs_blending_weights": w,
                   "rgb_fg": rgb_fg, "bg_transmittance": bg_T}
        return renders, samples_3d, samples_sdf, samples_grad

    def render_rays(self, rays_o, rays_d, iter_nr=None, override=None, **kwargs):
        """The reference's dict: {"renders": {"volumetric": {surfs_rgb, surfs_normals, surfs_depths,
        surfs_weight_sum, surfs_alpha, surfs_transmittance, surfs_blending_weights, nr_samples, rgb_fg,
        bg_transmittance, rgb_bg, rgb}}, "samples_3d", "samples_grad"}.  `override` takes "variance" and
        "cos_anneal_ratio".  With `render_sphere_traced` set and outside training, "renders" also holds
        "sphere_traced": render_fg_sphere_traced's entries (100 rounds, 1e-3) with rgb_bg and rgb = rgb_fg +
        bg_transmittance rgb_bg (the reference has this blend commented out, which leaves the entry without `rgb`)."""
        hp = self.hyper_params
        override = override or {}
        raycast = intersect_bounding_primitive(self.bounding_primitive, rays_o, rays_d)
        variance = override.get("variance")
        beta = get_logistic_beta_from_variance(self.variance if variance is None else variance)
        car = override.get("cos_anneal_ratio")
        car = self.cos_anneal_ratio if car is None else car
        pack, _ = get_rays_samples_packed_sdfs(
            rays_o, rays_d, raycast["t_near"], raycast["t_far"], self.models["sdfs"], self.nr_surfs, beta,
            self.occupancy_grid, iter_nr, hp.min_dist_between_samples, hp.min_nr_samples_per_ray,
            hp.max_nr_samples_per_ray, hp.max_nr_imp_samples_per_ray, jitter_samples=self.is_training,
            importance_sampling=hp.do_importance_sampling)
        rgb_bg, blend_bg, _ = self._render_bg(raycast, iter_nr)
        renders, samples_3d, samples_grad = self.render_fg_volumetric(pack, beta, car, iter_nr, blend_bg)
        renders["rgb_bg"] = rgb_bg
        all_renders = {"volumetric": renders}
        if self.render_sphere_traced and not self.is_training:
            st = self.render_fg_sphere_traced(raycast, self.SPHERE_TRACED_MAX_STEPS, self.SPHERE_TRACED_THRESH,
                                              iter_nr)[0]
            st["rgb_bg"] = rgb_bg
            st["rgb"] = st["rgb_fg"] + st["bg_transmittance"] * rgb_bg
            all_renders["sphere_traced"] = st
        return {"renders": all_renders, "samples_3d": samples_3d, "samples_grad": samples_grad}

    # ---- training (offsets_surfs.py:1130-1449)
    def _support(self, grads):
        return torch.cat((grads[:, :self.main_surf_idx], grads[:, self.main_surf_idx + 1:]), dim=1)

    def _offsets_init_losses(self, iter_nr):
        s = self.models["sdfs"]
        with torch.no_grad():
            pts = self.bounding_primitive.get_random_points_inside(self.OFFSETS_INIT_NR_POINTS)
        # main_sdf(points) and get_field_gradients(forward, points) share one stencil call (same rows)
        full_sdfs, _, full_feat = field_stencil(s.forward, pts, iter_nr)
        grads = stencil_gradients(full_sdfs)
        feats = full_feat[:pts.shape[0]]
        off_pos, off_neg, _, _ = s.get_offsets(feats)
        offsets = torch.cat((off_pos, off_neg), dim=1)
        gt = self.offsets_gt.to(offsets.device).unsqueeze(0).expand(pts.shape[0], self.nr_surfs - 1)
        loss_offsets = torch.abs(offsets - gt).mean()
        loss_supp = eikonal_loss(self._support(grads)) * self.hyper_params.support_surfs_eikonal_weight
        return loss_offsets + loss_supp, loss_supp

    def forward(self, rays_o, rays_d, gt_rgb, gt_mask=None, iter_nr=0, is_first_iter=False, is_training_masked=None,
                **kwargs):
        hp = self.hyper_params
        masked = hp.is_training_masked if is_training_masked is None else is_training_masked
        s = self.models["sdfs"]
        loss = torch.zeros((), device="cuda", requires_grad=True)
        loss_curv = loss_eik_main = loss_eik_supp = loss_offsurface = loss_rgb = loss_mask = 0.0
        self.update_method_state(iter_nr)
        samples_3d = None
        if self.in_offsets_init:
            if self.nr_surfs > 1 and s.is_training_offsets:
                loss, loss_eik_supp = self._offsets_init_losses(iter_nr)
        else:
            res = self.render_rays(rays_o, rays_d, iter_nr=iter_nr)
            samples_3d, s_grad = res["samples_3d"], res["samples_grad"]
            loss_rgb, _ = self._loss_rgb(res["renders"]["volumetric"], gt_rgb, gt_mask, masked)
            loss = loss_rgb
            r_sdfs, r_grad = self._random_points_stencil(s.forward, iter_nr)
            has_samples = samples_3d is not None and samples_3d.shape[0] > 0
            main = self.main_surf_idx
            if hp.eikonal_weight > 0.0 and s.is_training_main_surf:
                loss_eik_main = self._loss_eikonal(r_grad[:, main], s_grad[:, main] if has_samples else None,
                                                   hp.eikonal_weight)
                loss = loss + loss_eik_main
            if hp.eikonal_weight > 0.0 and hp.support_surfs_eikonal_weight > 0.0 and s.is_training_offsets and \
                    self.nr_surfs > 1:
                loss_eik_supp = self._loss_eikonal(self._support(r_grad), self._support(s_grad) if has_samples else None,
                                                   hp.support_surfs_eikonal_weight)
                loss = loss + loss_eik_supp
            if hp.offsurface_weight > 0.0:
                loss_offsurface = self._loss_offsurface(r_sdfs[:, main])
                loss = loss + loss_offsurface
            if hp.curvature_weight > 0.0 and has_samples:
                curv = get_sdfs_curvature(s, samples_3d, s_grad, torch.randn_like(samples_3d), iter_nr=iter_nr)
                loss_curv = curv.mean() * hp.curvature_weight
                loss = loss + loss_curv
        losses = {"loss": loss, "curvature": loss_curv, "eikonal_main": loss_eik_main, "eikonal_supp": loss_eik_supp,
                  "loss_offsurface_high_sdf": loss_offsurface, "rgb": loss_rgb, "mask": loss_mask}
        info = {"stdev": logistic_distribution_stdev(get_logistic_beta_from_variance(self.variance))}
        return losses, info, samples_3d
