"""Times the NeRF method's fused kernels against the op chains they replace, at the reference's batch (512 rays,
max_nr_samples_per_ray 64 + 32 importance samples), and one training iteration of the method.

    python tools/nerf_bench.py [--rays 512] [--iters 200] [--train-iters 200]

Prints one JSON line: ms per call of the fused composite (forward + backward) and coarse CDF, the same for their
single-op chains, and training iterations per second."""
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
    from volsurfs_amd.nerf import nerf_coarse_cdf, nerf_composite
    N = a.rays
    out = {"rays": N}
    # the composite runs on the combined pack (64 + 32 samples), the coarse CDF on the uniform one (64)
    p = _pack(N, 96)
    S = N * 96
    dens = torch.rand(S, 1, device="cuda") * 20
    col = torch.rand(S, 3, device="cuda")
    bg = torch.rand(N, 3, device="cuda")
    g = torch.randn(N, 3, device="cuda")

    def fused():
        d, c = dens.clone().requires_grad_(True), col.clone().requires_grad_(True)
        o = nerf_composite(p, d, c, bg)
        (o["rgb"] * g).sum().backward()

    def chain():
        d, c = dens.clone().requires_grad_(True), col.clone().requires_grad_(True)
        alpha = 1.0 - torch.exp(-d * p.samples_dt)
        T, _ = V.CumprodOneMinusAlphaToTransmittanceFunc.apply(p, 1 - alpha + 1e-6)
        w = alpha * T
        ws, _ = V.SumOverRaysFunc.apply(p, w)
        fg = V.IntegrateWithWeights3DFunc.apply(p, c, w)
        V.VolumeRendering.integrate_with_weights_1d(p, p.samples_z, w.detach())
        ((fg + (1 - ws) * bg) * g).sum().backward()

    out["composite_fused_ms"] = _timed(fused, a.iters)
    out["composite_chain_ms"] = _timed(chain, a.iters)
    pu = _pack(N, 64)
    du = torch.rand(N * 64, 1, device="cuda") * 20

    def cdf_chain():
        alpha = torch.clamp(1.0 - torch.exp(-du * pu.samples_dt), min=0.0, max=1.0)
        T, _ = V.VolumeRendering.cumprod_one_minus_alpha_to_transmittance(pu, 1 - alpha + 1e-6)
        w = alpha * T
        _, ws = V.VolumeRendering.sum_over_rays(pu, w)
        w /= torch.clamp(ws, min=1e-6)
        V.VolumeRendering.compute_cdf(pu, w)

    out["coarse_cdf_fused_ms"] = _timed(lambda: nerf_coarse_cdf(pu, du), a.iters)
    out["coarse_cdf_chain_ms"] = _timed(cdf_chain, a.iters)
    # one training iteration of the method (reference hyper-parameters, constant background)
    from volsurfs_amd.background import BoundingSphere
    from volsurfs_amd.nerf import NeRF, NeRFHyperParams
    from volsurfs_amd.trainer import train_step
    torch.manual_seed(0)
    m = NeRF(True, NeRFHyperParams(), None, None, BoundingSphere(0.5), bg_color=(0.0, 0.0, 0.0))
    o = torch.nn.functional.normalize(torch.randn(N, 3, device="cuda"), dim=1) * 1.5
    d = torch.nn.functional.normalize(torch.rand(N, 3, device="cuda") * 0.4 - 0.2 - o, dim=1)
    gt = torch.rand(N, 3, device="cuda")
    for it in range(10):
        train_step(m, o, d, gt, None, iter_nr=it, is_first_iter=it == 0)
    torch.cuda.synchronize()
    t = time.time()
    for it in range(10, 10 + a.train_iters):
        train_step(m, o, d, gt, None, iter_nr=it)
    torch.cuda.synchronize()
    out["train_it_per_s"] = a.train_iters / (time.time() - t)
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
