"""Baked textures refitted to target views: Adam on the 8-bit texel rows themselves, on the device (csrc/texel_fit.hip;
the rule in include/volsurfs_hip.h "Texture fit").  The reference has no such stage: the rule is this
library's own, restated in tests/texture_fit_restated.py and unpinned.

`texture_transfer.make_lod` resamples appearance; it cannot make up for moved geometry, another atlas's seams or halved
texel density.  Here the lighter scene's textures are optimised against renders of the source, through the kernels of
the training path: trace -> a `ShadedFrame` of the baked bank (per-hit uv, shade) -> fused composite + L1 -> the frame's
shade backward into this fit's gradient rows -> `vsa_texel_fit_step`.

* `TextureFit` — a copy of a baked scene with gradient rows and Adam state; `accumulate` views, then `step`.
* `fit_textures` — the loop over cameras, with a report.
* `refit_lod` — `fit_textures` of a LOD against renders of its source from hemisphere cameras.

NOT promised: two fits of the same scene to the same views need not give the same bytes (the shade backward adds f16
atomically; the step itself is deterministic).  hits="trace" only, L1 only, no regulariser, no mip chain: the fit
renders and differentiates the bilinear fetch of level 0 only, and its results (`TextureFit.scene`, `fit_textures`,
`refit_to`) carry no `texture_mip.MipChain`.  A fitted scene needs `build_mips` again before `filter="mip"`; a chain
built before a `step()` is stale and refused.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

DEFAULT_LR = 1e-3            # the best, and the lowest, of the sweep {1e-3, 3e-3, 1e-2, 3e-2} on DESIGN §41's LOD scenes
STAT_WORDS = 4               # quads updated, non-finite gradient elements, bytes changed, elements clamped

FitReport = collections.namedtuple(
    "FitReport", "loss_before loss_after steps losses texels_touched quads_updated bytes_changed nonfinite clamped")
FitReport.__doc__ = """What `fit_textures` did.  loss_before / loss_after: the mean L1 over ALL views before the first
step and with the final bytes; steps; losses: the mean L1 of the last view accumulated before each step;
texels_touched: {(shell, degree): interior texels that ever received a gradient}; quads_updated, bytes_changed,
clamped: sums of the steps' counters; nonfinite: gradient elements that were not finite and were taken as zero (0 in a
healthy fit)."""


class TextureFit:
    """Adam on the texel rows of a copy of `scene` (a `BakedScene`, or a `VolSurfs` after `bake()`; never mutated).
    `.scene` is the scene being fitted: it renders at any time through `render_baked*`.  `.loss`: the mean L1 of the
    last `accumulate`, a device scalar.  lr / betas / eps: Adam's, on parameters in units of q / 255."""

    def __init__(self, scene, lr=DEFAULT_LR, betas=(0.9, 0.99), eps=1e-15, builder="device"):
        from .texture_export import baked_bank_of, export_planes
        from .texture_transfer import scene_like
        src_bank = baked_bank_of(scene, "TextureFit")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        if not (self.lr >= 0.0 and self.eps >= 0.0 and all(0.0 <= b < 1.0 for b in self.betas)):
            raise _lib.VolsurfsHipError(f"TextureFit: lr {lr}, betas {betas}, eps {eps} out of range")
        # a new BakedScene with the bytes of `scene` (the apron clamped)
        self.scene = scene_like(scene, scene.tensor_meshes, export_planes(src_bank), builder)
        bank = self.scene.baked
        n = _lib.workspace_bytes("vsa_texel_fit_state_bytes", ctypes.byref(bank.plan)) // 4
        dev = bank.texels.device
        self.grad_rows = torch.zeros(n, dtype=torch.float16, device=dev)
        self.p, self.m, self.v = (torch.zeros(n, device=dev) for _ in range(3))
        self.totals = torch.zeros(STAT_WORDS, dtype=torch.int64, device=dev)
        self.steps, self.loss, self._scale = 0, None, None
        _lib.call("vsa_texel_fit_init", ctypes.byref(bank.plan), bank.slot_of, bank.seg_start, bank.texels, self.p,
                  self.m, self.v, _lib.stream_ptr())

    def accumulate(self, rays_o, rays_d, target_rgb, loss_weight=1.0, chunk=1 << 20):
        """Adds the gradient of loss_weight * mean |target_rgb - rgb| over these rays to the gradient rows.  May be
        called for several views before one `step()`."""
        from .composite import composite_fwd_bwd_l1_raw, l1_mean
        from .neural_textures import chain_scale
        scene, bank = self.scene, self.scene.baked
        N = int(rays_o.shape[0])
        if N < 1 or tuple(target_rgb.shape) != (N, 3):
            raise _lib.VolsurfsHipError(f"accumulate: {N} rays with targets of shape {tuple(target_rgb.shape)}")
        loss_scale = float(loss_weight) / (3.0 * N)
        if self._scale is None:                  # one scale for everything that meets in the rows before a step
            self._scale = chain_scale(loss_scale=loss_scale)
        tris, losses = scene.raytracer.tris, []
        for a in range(0, N, chunk):
            o, d = rays_o[a:a + chunk].contiguous(), rays_d[a:a + chunk].contiguous()
            gt = target_rgb[a:a + chunk].contiguous().float()
            _, hit_slot, hit_uv = scene._trace_now(o, d)
            frame = bank.frame(hit_slot, hit_uv, scene.face_uvs)
            rgb_k, alpha_k, _ = frame.forward(d, tris, differentiable=True)
            rgb, g_c, g_a = composite_fwd_bwd_l1_raw(rgb_k, alpha_k, scene.bg_color, gt, loss_scale)
            frame.backward(g_c, g_a, self._scale, grad_rows=self.grad_rows)
            losses.append((l1_mean(rgb, gt), int(o.shape[0])))
        self.loss = losses[0][0] if len(losses) == 1 else sum(l * (n / N) for l, n in losses)
        return self.loss

    def step(self):
        """One Adam step on what `accumulate` gathered; the gradient rows are zero again afterwards.  Returns the
        step's counters, int64 [4] on the device (quads updated, non-finite gradient elements, bytes changed, elements
        clamped): nothing is read back here."""
        if self._scale is None:
            raise _lib.VolsurfsHipError("TextureFit.step: nothing accumulated since the last step")
        bank = self.scene.baked
        self.steps += 1
        stats = torch.empty(STAT_WORDS, dtype=torch.int64, device=self.p.device)
        _lib.call("vsa_texel_fit_step", ctypes.byref(bank.plan), bank.slot_of, bank.seg_start, self.grad_rows,
                  1.0 / self._scale, self.p, self.m, self.v, bank.texels, self.lr, self.betas[0], self.betas[1],
                  self.eps, self.steps, stats, _lib.stream_ptr())
        bank.texels_version += 1                     # a mip chain of these bytes is stale now
        self._scale = None
        self.totals += stats
        return stats

    def texels_touched(self):
        """{(shell, degree): interior texels with a non-zero second moment} as device scalars."""
        from .neural_textures import MAX_DEG, ROW_QUADS
        bank, out = self.scene.baked, {}
        for s in range(bank.K):
            for d in range(bank.D):
                sd, W = s * MAX_DEG + d, bank.tex_res[d] + 2
                r0 = int(bank.plan.row_base[sd]) * 4
                rows = self.v[r0:r0 + W * W * ROW_QUADS[d] * 4].view(W * W, -1)
                out[(s, d)] = (rows != 0).any(1).sum()
        return out


def _targets_of(teacher, cameras, supersample):
    return [teacher.render_baked_camera(c, supersample=supersample)["rgb"].float().contiguous() for c in cameras]


@torch.no_grad()
def fit_textures(scene, cameras, targets=None, teacher=None, iterations=100, views_per_step=1, supersample=1,
                 lr=DEFAULT_LR, seed=0, betas=(0.9, 0.99), eps=1e-15, builder="device"):
    """(fitted scene, FitReport): a copy of `scene` whose textures were fitted for `iterations` Adam steps to the
    targets of `cameras`.  targets: a device stack [V, H * W, 3] in float, or teacher: anything with
    `render_baked_camera(camera)`, whose "rgb" (rendered once per camera, with `supersample`, kept on the device) is
    the target.  Each step accumulates `views_per_step` views; the views are visited in a permutation drawn from `seed`,
    again and again.  supersample = s > 1: s^2 jittered rays per pixel, each against the pixel's target."""
    from .camera import get_camera_rays
    from .composite import l1_mean
    cameras = list(cameras)
    if (targets is None) == (teacher is None):
        raise _lib.VolsurfsHipError("fit_textures: give targets or a teacher (one of them)")
    s = int(supersample)
    if not cameras or not 1 <= s <= 8 or int(iterations) < 0 or int(views_per_step) < 1:
        raise _lib.VolsurfsHipError("fit_textures: needs cameras, supersample in 1..8, iterations >= 0 and "
                                    "views_per_step >= 1")
    if targets is None:
        targets = _targets_of(teacher, cameras, s)
    if len(targets) != len(cameras):
        raise _lib.VolsurfsHipError(f"fit_textures: {len(targets)} targets for {len(cameras)} cameras")
    fit = TextureFit(scene, lr, betas, eps, builder)

    def loss_over_all_views():
        each = [l1_mean(fit.scene.render_baked_camera(c)["rgb"].float(), t.float()) for c, t in zip(cameras, targets)]
        return torch.stack(each).mean()

    before = loss_over_all_views()
    order = np.random.RandomState(int(seed)).permutation(len(cameras))
    losses, visit = [], 0
    for _ in range(int(iterations)):
        for _ in range(int(views_per_step)):
            i = int(order[visit % len(order)])
            visit += 1
            rays_o, rays_d, _ = get_camera_rays(cameras[i], s * s, s > 1)
            t = targets[i].float()
            fit.accumulate(rays_o, rays_d, t if s == 1 else t.repeat_interleave(s * s, 0))
        losses.append(fit.loss)
        fit.step()
    after = loss_over_all_views()
    touched = fit.texels_touched()
    words = torch.cat([torch.stack([before, after] + losses).double(),              # the one blocking read
                       fit.totals.double(), torch.stack(list(touched.values())).double()]).cpu().tolist()
    n = 2 + len(losses)
    totals = [int(w) for w in words[n:n + STAT_WORDS]]
    report = FitReport(words[0], words[1], fit.steps, words[2:n],
                       {k: int(w) for k, w in zip(touched, words[n + STAT_WORDS:])}, totals[0], totals[2], totals[1],
                       totals[3])
    return fit.scene, report


@torch.no_grad()
def refit_lod(src, lod, cameras=None, nr_cameras=16, radius=None, resolution=(256, 256), focal=None, **fit):
    """(fitted scene, FitReport): `fit_textures(lod, cameras, teacher=src, **fit)`.  cameras: default `nr_cameras` from
    `sample_cameras_on_hemisphere` of `radius` (default: three times the largest vertex distance from the origin)
    on the +z hemisphere and the rest on the -z one (a stream of their own: the same cameras every call), `resolution`
    = (W, H) pixels, `focal` (default: the shells fill most of the image)."""
    if cameras is None:
        from .camera import sample_cameras_on_hemisphere
        from .volsurfs import _Pcg32State
        W, H = (int(x) for x in resolution)
        if radius is None:
            radius = 3.0 * max(float(m.vertices.norm(dim=1).max()) for m in src.tensor_meshes)
        if focal is None:
            focal = 1.2 * min(W, H)
        K = torch.tensor([[focal, 0.0, 0.5 * W], [0.0, focal, 0.5 * H], [0.0, 0.0, 1.0]])
        rng, n_up = _Pcg32State(), (int(nr_cameras) + 1) // 2
        cameras = (sample_cameras_on_hemisphere(K, W, H, float(radius), n_up, up_sign=1, rng=rng) +
                   sample_cameras_on_hemisphere(K, W, H, float(radius), int(nr_cameras) - n_up, up_sign=-1, rng=rng))
    return fit_textures(lod, cameras, teacher=src, **fit)


__all__ = ["TextureFit", "FitReport", "fit_textures", "refit_lod", "DEFAULT_LR"]
