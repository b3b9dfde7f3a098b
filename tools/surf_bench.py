"""Times the Surf method's fused kernels against the op chains they replace, at the reference's batch (512 rays,
max_nr_samples_per_ray 64 + 32 importance samples), and one training iteration of the method.

    python tools/surf_bench.py [--rays 512] [--iters 200] [--train-iters 200]

Prints one JSON line: ms per call of the fused NeuS composite (forward + backward) and of one coarse-CDF round
(the uniform pack, 64 samples per ray), the same for their chains of single ops, and training iterations per second
of the first phase with the reference's hyper-parameters."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _pack(N, n, device="cuda"):
    from volsurfs_amd.volsurfs import RaySamplesPacked
    S = N * n
    p = RaySamplesPacked(N, S, 0, 0)
    i = torch.arange(N, dtype=torch.int32, device=device) * n
    p.ray_start_end_idx = torch.stack([i, i + n], 1).contiguous()
    p.is_compacted = p.has_dt = True
    p.samples_dt = torch.rand(S, 1, device=device) * 0.02 + 1e-3
    p.samples_z = torch.cumsum(p.samples_dt, 0)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--train-iters", type=int, default=200)
    a = ap.parse_args()
    from volsurfs_amd import volsurfs as V
    from volsurfs_amd.surf import neus_alphas_torch, neus_composite, sdf_coarse_cdf
    N = a.rays
    out = {"rays": N}
    car, beta = 0.5, float(torch.exp(torch.tensor(5.0, dtype=torch.float64)))
    # the composite runs on the combined pack (64 + 32 samples), the coarse CDF on the uniform one (64)
    p = _pack(N, 96)
    S = N * 96
    p.samples_dirs = torch.nn.functional.normalize(torch.randn(S, 3, device="cuda"), dim=1)
    sdf = 0.2 - p.samples_z.remainder(0.4)
    grad = torch.randn(S, 3, device="cuda")
    nrm = torch.nn.functional.normalize(grad, dim=1)
    col = torch.rand(S, 3, device="cuda")
    bg = torch.rand(N, 3, device="cuda")
    g = torch.randn(N, 3, device="cuda")

    def fused():
        s, gr, c = sdf.clone().requires_grad_(True), grad.clone().requires_grad_(True), col.clone().requires_grad_(True)
        o = neus_composite(p, s, gr, nrm, c, bg, car, beta)
        (o["rgb"] * g).sum().backward()

    def chain():
        s, gr, c = sdf.clone().requires_grad_(True), grad.clone().requires_grad_(True), col.clone().requires_grad_(True)
        alpha = neus_alphas_torch(p.samples_dirs, p.samples_dt, s, gr, car, beta)
        T, _ = V.CumprodOneMinusAlphaToTransmittanceFunc.apply(p, 1 - alpha + 1e-6)
        w = alpha * T
        ws, _ = V.SumOverRaysFunc.apply(p, w)
        fg = V.IntegrateWithWeights3DFunc.apply(p, c, w)
        V.VolumeRendering.integrate_with_weights_1d(p, p.samples_z, w.detach())
        V.VolumeRendering.integrate_with_weights_3d(p, nrm, w.detach())
        ((fg + (1 - ws) * bg) * g).sum().backward()

    out["composite_fused_ms"] = _timed(fused, a.iters)
    out["composite_chain_ms"] = _timed(chain, a.iters)
    pu = _pack(N, 64)
    su = 0.2 - pu.samples_z.remainder(0.4)

    def cdf_chain():
        alpha = V.VolumeRendering.sdf2alpha(pu, su, torch.ones_like(pu.samples_dt) * beta / 2.0)
        T, _ = V.VolumeRendering.cumprod_one_minus_alpha_to_transmittance(pu, 1 - alpha + 1e-6)
        w = alpha * T
        _, ws = V.VolumeRendering.sum_over_rays(pu, w)
        w /= torch.clip(ws, min=1e-6)
        V.VolumeRendering.compute_cdf(pu, w)

    half = float(torch.tensor(beta, dtype=torch.float32) / 2)
    out["coarse_cdf_fused_ms"] = _timed(lambda: sdf_coarse_cdf(pu, su, half), a.iters)
    out["coarse_cdf_chain_ms"] = _timed(cdf_chain, a.iters)
    # training iterations of the first phase (reference hyper-parameters, constant background) after a short
    # sphere init, so that the occupancy grid holds a surface
    from volsurfs_amd.background import BoundingSphere
    from volsurfs_amd.surf import Surf, SurfHyperParams
    from volsurfs_amd.trainer import train_step
    torch.manual_seed(0)
    hp = SurfHyperParams()
    m = Surf(True, hp, None, None, BoundingSphere(0.5), bg_color=(0.0, 0.0, 0.0), init_sphere_radius=0.3)
    o = torch.nn.functional.normalize(torch.randn(N, 3, device="cuda"), dim=1) * 1.5
    d = torch.nn.functional.normalize(torch.rand(N, 3, device="cuda") * 0.4 - 0.2 - o, dim=1)
    gt = torch.rand(N, 3, device="cuda")
    for it in range(200):
        train_step(m, o, d, gt, None, iter_nr=it, is_first_iter=it == 0)
    start = hp.init_phase_end_iter
    for it in range(start, start + 10):
        train_step(m, o, d, gt, None, iter_nr=it)
    torch.cuda.synchronize()
    t = time.time()
    for it in range(start + 10, start + 10 + a.train_iters):
        train_step(m, o, d, gt, None, iter_nr=it)
    torch.cuda.synchronize()
    out["train_it_per_s"] = a.train_iters / (time.time() - t)
    out["train_samples_per_it"] = int(m.last_nr_samples)
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
