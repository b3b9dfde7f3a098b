"""Times the OffsetsSurfs method's fused kernels against the op chains they replace, at the reference's batch (512
rays, 64 + 32 samples per ray), for K = 5 and 9 surfaces (median of three rounds, K alternating); the row-batched
appearance against the per-surface calls; and training iterations per second in each phase with the base_5
hyper-parameters.

    python tools/offsets_surfs_bench.py [--rays 512] [--iters 100] [--train-iters 50]

Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from surf_bench import _pack, _timed  # noqa: E402


def _composite_and_cdf(out, N, K, iters):
    from volsurfs_amd import volsurfs as V
    from volsurfs_amd.offsets_surfs import offsets_composite, sdfs_coarse_cdf
    from volsurfs_amd.surf import neus_alphas_torch
    car, beta, decay = 1.0, float(torch.exp(torch.tensor(7.0, dtype=torch.float64))), 500.0
    p = _pack(N, 96)
    S = N * 96
    p.samples_dirs = torch.nn.functional.normalize(torch.randn(S, 3, device="cuda"), dim=1)
    shifts = torch.linspace(0.03, -0.03, K, device="cuda").view(1, K)
    sdfs = (0.2 - p.samples_z.remainder(0.4) + shifts).contiguous()
    grads = torch.randn(S, K, 3, device="cuda")
    nrm = torch.nn.functional.normalize(grads, dim=-1)
    rgb, tr = torch.rand(S, K, 3, device="cuda"), torch.rand(S, K, 1, device="cuda")
    bg, g = torch.rand(N, 3, device="cuda"), torch.randn(N, 3, device="cuda")
    leaves = lambda: [x.clone().requires_grad_(True) for x in (sdfs, grads, rgb, tr)]

    def fused():
        s, gr, c, t = leaves()
        o = offsets_composite(p, s, gr, nrm, c, t, bg, car, beta, decay)
        (o["rgb"] * g).sum().backward()

    def chain():
        s, gr, c, t = leaves()
        sr, sa = [], []
        for k in range(K):
            a = neus_alphas_torch(p.samples_dirs, p.samples_dt, s[:, k:k + 1], gr[:, k], car, beta)
            T = V.CumprodOneMinusAlphaToTransmittanceFunc.apply(p, 1 - a + 1e-6)[0]
            w = a * T
            with torch.no_grad():
                dot = torch.sum(-p.samples_dirs * nrm[:, k], dim=1, keepdim=True).clamp(0.0, 1.0)
                dec = torch.sigmoid(decay * dot) * 2.0 - 1.0
            sr.append(V.IntegrateWithWeights3DFunc.apply(p, c[:, k].contiguous(), w))
            sa.append(V.IntegrateWithWeights1DFunc.apply(p, t[:, k] * dec, w))
            with torch.no_grad():
                V.VolumeRendering.integrate_with_weights_1d(p, p.samples_z, w)
                V.VolumeRendering.sum_over_rays(p, w)
                V.VolumeRendering.integrate_with_weights_3d(p, nrm[:, k].contiguous(), w)
        sr, sa = torch.stack(sr, 1).flip(1), torch.stack(sa, 1).flip(1)
        trans = torch.cumprod(1 - sa, dim=1)
        sT = torch.cat([torch.ones_like(trans[:, -1:]), trans[:, :-1]], dim=1)
        fg = (sr * sT * sa).sum(dim=1)
        ((fg + bg * trans[:, -1]) * g).sum().backward()

    out[f"K{K}_composite_fused_ms"] = _timed(fused, iters)
    out[f"K{K}_composite_chain_ms"] = _timed(chain, iters)
    pu = _pack(N, 64)
    su = (0.2 - pu.samples_z.remainder(0.4) + shifts).contiguous()

    def cdf_chain():
        lb = torch.ones_like(pu.samples_dt) * beta / 2.0
        agg = torch.zeros_like(pu.samples_dt)
        for k in range(K):
            alpha = V.VolumeRendering.sdf2alpha(pu, su[:, k:k + 1].contiguous(), lb)
            T = V.VolumeRendering.cumprod_one_minus_alpha_to_transmittance(pu, 1 - alpha + 1e-6)[0].clip(0.0, 1.0)
            w = alpha * T
            _, ws = V.VolumeRendering.sum_over_rays(pu, w)
            w /= torch.clip(ws, min=1e-6)
            agg += V.VolumeRendering.compute_cdf(pu, w)
        return agg / K

    half = float(torch.tensor(beta, dtype=torch.float32) / 2)
    out[f"K{K}_coarse_cdf_fused_ms"] = _timed(lambda: sdfs_coarse_cdf(pu, su, half), iters)
    out[f"K{K}_coarse_cdf_chain_ms"] = _timed(cdf_chain, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--train-iters", type=int, default=50)
    a = ap.parse_args()
    N = a.rays
    out = {"rays": N}
    # three rounds, the order of K alternating, so that neither K always runs first on a cold device; the median
    # of the three goes out, the spread alongside
    runs = []
    for order in ((5, 9), (9, 5), (5, 9)):
        r = {}
        for K in order:
            _composite_and_cdf(r, N, K, a.iters)
        runs.append(r)
    for k in runs[0]:
        v = sorted(r[k] for r in runs)
        out[k] = v[1]
        out[k + "_spread"] = v[2] - v[0]
    from volsurfs_amd.background import BoundingSphere
    from volsurfs_amd.offsets_surfs import OffsetsSurfs, OffsetsSurfsHyperParams, appearance_rows
    from volsurfs_amd.surf import Surf, SurfHyperParams
    from volsurfs_amd.trainer import train_step
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        # (no coarse-to-fine: OffsetsSDF runs every encoder level, as after a full surf run)
        s = Surf(True, SurfHyperParams(sdf_nr_iters_for_c2f=0), None, tmp, BoundingSphere(0.5),
                 bg_color=(0.0, 0.0, 0.0), init_sphere_radius=0.3)
        o = torch.nn.functional.normalize(torch.randn(N, 3, device="cuda"), dim=1) * 1.5
        d = torch.nn.functional.normalize(torch.rand(N, 3, device="cuda") * 0.4 - 0.2 - o, dim=1)
        gt = torch.rand(N, 3, device="cuda")
        for it in range(200):
            train_step(s, o, d, gt, None, iter_nr=it, is_first_iter=it == 0)
        path = s.save(200)
        hp = OffsetsSurfsHyperParams()
        m = OffsetsSurfs(True, hp, None, None, BoundingSphere(0.5), path, bg_color=(0.0, 0.0, 0.0))
    # training iterations per second in each phase, each entered from its start by update_method_state (the freeze
    # state it sets is recorded next to the figure)
    phases = {"offsets_init": 0, "color_init": hp.init_phase_end_iter, "first_phase": hp.color_init_phase_end_iter,
              "second_phase": hp.first_phase_end_iter}
    sdfs = m.models["sdfs"]
    for name, start in phases.items():
        for it in range(start, start + 5):
            train_step(m, o, d, gt, None, iter_nr=it, is_first_iter=it == 0)
        out[f"train_{name}_trains_main_surf"] = sdfs.is_training_main_surf
        out[f"train_{name}_trains_offsets"] = sdfs.is_training_offsets
        torch.cuda.synchronize()
        t = time.time()
        for it in range(start + 5, start + 5 + a.train_iters):
            train_step(m, o, d, gt, None, iter_nr=it)
        torch.cuda.synchronize()
        out[f"train_{name}_it_per_s"] = a.train_iters / (time.time() - t)
    # the row-batched shared appearance against the reference's K calls, on a render's samples (after the phase
    # loop: rendering needs a phase past the offsets init, and entering one out of order would skip its freezes)
    res = m.render_rays(o, d, iter_nr=hp.first_phase_end_iter)
    pts = res["samples_3d"].detach()
    S, K = pts.shape[0], m.nr_surfs
    dirs = torch.nn.functional.normalize(torch.randn_like(pts), dim=-1)
    nrm = torch.nn.functional.normalize(torch.randn(S, K, 3, device="cuda"), dim=-1)
    feat = torch.randn(S, hp.geom_feat_size, device="cuda", requires_grad=True)
    gr = torch.randn(S, K, 3, device="cuda")

    def rows():
        appearance_rows(m.models["rgb"], pts, dirs, nrm, feat).mul(gr).sum().backward()

    def per_surface():
        sum(m.models["rgb"](points=pts, samples_dirs=dirs, normals=nrm[:, k], geom_feat=feat).mul(gr[:, k]).sum()
            for k in range(K)).backward()

    out["appearance_samples"] = S
    out["appearance_rows_ms"] = _timed(rows, a.iters)
    out["appearance_per_surface_ms"] = _timed(per_surface, a.iters)
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
