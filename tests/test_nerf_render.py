"""The NeRF method's fused per-ray kernels (csrc/nerf_render.hip) against the chains of single ops they replace:
bit-identical forward and backward, deterministic, and close to a float64 CPU restatement."""
import numpy as np
import pytest
import torch


def _start_end(counts):
    counts = np.asarray(counts, np.int64)
    ends = np.cumsum(counts)
    return np.stack([ends - counts, ends], 1).astype(np.int32), int(ends[-1]) if len(ends) else 0


def _counts(seed, n_rays=600):
    """Empty rays, 1-sample rays and the chunk edges 31 / 32 / 33 plus a 200-sample ray, among random lengths."""
    g = np.random.default_rng(seed)
    c = g.integers(0, 97, n_rays)
    c[:8] = [0, 1, 31, 32, 33, 200, 0, 1]
    return c


def _pack(se, S, seed):
    from volsurfs_amd.volsurfs import RaySamplesPacked
    g = np.random.default_rng(seed)
    N = se.shape[0]
    p = RaySamplesPacked(N, S, 0, 0)
    p.ray_start_end_idx = torch.from_numpy(se).cuda()
    p.is_compacted = True
    dt = g.uniform(1e-3, 0.05, (S, 1)).astype(np.float32)
    z = np.zeros((S, 1), np.float32)
    for a, b in se:
        z[a:b, 0] = 0.1 + np.cumsum(dt[a:b, 0])
    p.samples_dt = torch.from_numpy(dt).cuda()
    p.samples_z = torch.from_numpy(z).cuda()
    p.has_dt = True
    return p


class _Blend(torch.autograd.Function):
    """rgb = rgb_fg + bgT * rgb_bg with the per-ray background gradient summed in the order the kernel states:
    g_bgT = (g_0 bg_0 + g_1 bg_1) + g_2 bg_2."""

    @staticmethod
    def forward(ctx, rgb_fg, bgT, rgb_bg):
        ctx.save_for_backward(bgT, rgb_bg)
        return rgb_fg + bgT * rgb_bg

    @staticmethod
    def backward(ctx, g):
        bgT, rgb_bg = ctx.saved_tensors
        b = rgb_bg.expand(g.shape[0], 3)
        g_bgT = g[:, 0:1] * b[:, 0:1]
        g_bgT = g_bgT + g[:, 1:2] * b[:, 1:2]
        g_bgT = g_bgT + g[:, 2:3] * b[:, 2:3]
        g_bg = g * bgT
        if rgb_bg.shape[0] != g.shape[0]:
            g_bg = g_bg.sum(0, keepdim=True)
        return g, g_bgT, g_bg


def _chain(p, density, rgb, rgb_bg):
    """methods/nerf.py:266-302 and the blend of render_rays on this project's single ops."""
    from volsurfs_amd import volsurfs as V
    alpha = 1.0 - torch.exp(-density * p.samples_dt)
    T, _ = V.CumprodOneMinusAlphaToTransmittanceFunc.apply(p, 1 - alpha + 1e-6)
    w = alpha * T
    wsum, _ = V.SumOverRaysFunc.apply(p, w)
    bgT = 1 - wsum
    rgb_fg = V.IntegrateWithWeights3DFunc.apply(p, rgb, w)
    depth = V.VolumeRendering.integrate_with_weights_1d(p, p.samples_z, w.detach())
    rgb_out = _Blend.apply(rgb_fg, bgT, rgb_bg) if rgb_bg is not None else rgb_fg
    return {"rgb": rgb_out, "rgb_fg": rgb_fg, "weights_sum": wsum, "depth": depth, "weights": w}


def _cpu_restatement(se, density, dt, z, rgb, rgb_bg, g_rgb, g_ws, bug_compat):
    """float64 torch autograd over the maths, per ray (the :1021 slip of bug_compat restated as the gradient w
    receives from the colour integral)."""
    density = density.double().requires_grad_(True)
    rgb = rgb.double().requires_grad_(True)
    bg = None if rgb_bg is None else rgb_bg.double().requires_grad_(True)
    dt, z = dt.double(), z.double()
    rgb_bug = rgb.detach()[:, [0, 1, 1]] if bug_compat else rgb.detach()
    outs = {"rgb": [], "weights_sum": [], "depth": []}
    for r, (a, b) in enumerate(se):
        alpha = 1 - torch.exp(-density[a:b] * dt[a:b])
        a1 = (1 - alpha) + 1e-6
        T = torch.cat([torch.ones(1, 1, dtype=torch.float64), torch.cumprod(a1, 0)[:-1]], 0)[: b - a]
        w = alpha * T
        fg = (w.detach() * rgb[a:b]).sum(0) + (w * rgb_bug[a:b]).sum(0) - (w * rgb_bug[a:b]).sum(0).detach()
        ws = w.sum(0)
        out = fg if bg is None else fg + (1 - ws) * bg[r if bg.shape[0] > 1 else 0]
        outs["rgb"].append(out)
        outs["weights_sum"].append(ws.view(1))
        outs["depth"].append((w * z[a:b]).sum(0).detach())
    res = {k: torch.stack(v) for k, v in outs.items()}
    loss = (res["rgb"] * g_rgb.double()).sum()
    if g_ws is not None:
        loss = loss + (res["weights_sum"] * g_ws.double()).sum()
    loss.backward()
    return res, density.grad, rgb.grad, None if bg is None else bg.grad


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("bug_compat", [True, False])
@pytest.mark.parametrize("bg", ["per_ray", "constant"])
@pytest.mark.parametrize("with_gws", [False, True])
def test_nerf_composite_equals_the_op_chain(bug_compat, bg, with_gws):
    from volsurfs_amd import volsurfs as V
    from volsurfs_amd.nerf import nerf_composite
    se, S = _start_end(_counts(3))
    p = _pack(se, S, 4)
    N = se.shape[0]
    g = np.random.default_rng(5)
    dens = torch.from_numpy(g.uniform(0.0, 40.0, (S, 1)).astype(np.float32)).cuda()
    col = torch.from_numpy(g.uniform(0, 1, (S, 3)).astype(np.float32)).cuda()
    bgc = torch.from_numpy(g.uniform(0, 1, (N, 3) if bg == "per_ray" else (1, 3)).astype(np.float32)).cuda()
    g_rgb = torch.from_numpy(g.standard_normal((N, 3)).astype(np.float32)).cuda()
    g_ws = torch.from_numpy(g.standard_normal((N, 1)).astype(np.float32)).cuda() if with_gws else None
    V.VolumeRendering.bug_compat = bug_compat
    try:
        runs = []
        for fused in (False, True, True):
            d = dens.clone().requires_grad_(True)
            c = col.clone().requires_grad_(True)
            b = bgc.clone().requires_grad_(True)
            out = nerf_composite(p, d, c, b, return_weights=True) if fused else _chain(p, d, c, b)
            loss = (out["rgb"] * g_rgb).sum()
            if with_gws:
                loss = loss + (out["weights_sum"] * g_ws).sum()
            loss.backward()
            runs.append([out["rgb"].detach(), out["rgb_fg"].detach(), out["weights_sum"].detach(),
                         out["depth"].detach(), out["weights"].detach(), d.grad, c.grad, b.grad])
        names = ("rgb", "rgb_fg", "weights_sum", "depth", "weights", "g_density", "g_rgb", "g_rgb_bg")
        for k, name in enumerate(names):
            if name == "g_rgb_bg" and bg == "constant":
                # the constant colour's gradient is a torch reduction over the rays on both sides
                torch.testing.assert_close(runs[1][k], runs[0][k], rtol=1e-5, atol=1e-5)
            else:
                assert torch.equal(runs[1][k], runs[0][k]), (name, float((runs[1][k] - runs[0][k]).abs().max()))
            assert torch.equal(runs[1][k], runs[2][k]), ("not deterministic", name)
        # the empty rays: no foreground, the background shows through
        assert torch.equal(runs[1][2][0], torch.zeros(1, device="cuda"))
        ref, gd, gc, gb = _cpu_restatement(se, dens.cpu(), p.samples_dt.cpu(), p.samples_z.cpu(), col.cpu(),
                                           bgc.cpu(), g_rgb.cpu(), None if g_ws is None else g_ws.cpu(), bug_compat)
        for got, want, name in ((runs[1][0], ref["rgb"], "rgb"), (runs[1][2], ref["weights_sum"], "weights_sum"),
                                (runs[1][3], ref["depth"], "depth"), (runs[1][5], gd, "g_density"),
                                (runs[1][6], gc, "g_rgb"), (runs[1][7], gb, "g_rgb_bg")):
            assert _rel(got, want) < 1e-6, (name, _rel(got, want))
    finally:
        V.VolumeRendering.bug_compat = True


@pytest.mark.gpu
def test_nerf_composite_without_background_and_zero_rays():
    from volsurfs_amd.nerf import nerf_composite
    se, S = _start_end([0, 0, 5, 40])
    p = _pack(se, S, 1)
    d = torch.rand(S, 1, device="cuda").requires_grad_(True)
    c = torch.rand(S, 3, device="cuda").requires_grad_(True)
    out = nerf_composite(p, d, c, None)
    ch = _chain(p, d, c, None)
    assert torch.equal(out["rgb"], ch["rgb"].detach()) and torch.equal(out["rgb_fg"], ch["rgb_fg"].detach())
    assert torch.equal(out["bg_transmittance"][:2], torch.ones(2, 1, device="cuda"))
    from volsurfs_amd.volsurfs import RaySamplesPacked
    e = RaySamplesPacked(0, 0, 0, 0)
    e.ray_start_end_idx = torch.zeros(0, 2, dtype=torch.int32, device="cuda")
    e.is_compacted, e.has_dt = True, True
    e.samples_dt = e.samples_z = torch.zeros(0, 1, device="cuda")
    out = nerf_composite(e, torch.zeros(0, 1, device="cuda"), torch.zeros(0, 3, device="cuda"))
    assert out["rgb"].shape == (0, 3)


@pytest.mark.gpu
def test_nerf_coarse_cdf_equals_the_op_chain():
    from volsurfs_amd import volsurfs as V
    from volsurfs_amd.nerf import nerf_coarse_cdf
    for seed, lo, hi in ((7, 0.0, 40.0), (8, 0.0, 1e-3), (9, 50.0, 500.0)):
        se, S = _start_end(_counts(seed))
        p = _pack(se, S, seed + 1)
        g = np.random.default_rng(seed + 2)
        dens = torch.from_numpy(g.uniform(lo, hi, (S, 1)).astype(np.float32)).cuda()
        # utils/nerf_utils.py:61-82
        alpha = torch.clamp(1.0 - torch.exp(-dens * p.samples_dt), min=0.0, max=1.0)
        T, _ = V.VolumeRendering.cumprod_one_minus_alpha_to_transmittance(p, 1 - alpha + 1e-6)
        w = alpha * T
        _, ws = V.VolumeRendering.sum_over_rays(p, w)
        ws = torch.clamp(ws, min=1e-6)
        w /= ws
        want = V.VolumeRendering.compute_cdf(p, w)
        got = nerf_coarse_cdf(p, dens)
        assert torch.equal(got, want), (seed, float((got - want).abs().max()))
        assert torch.equal(got, nerf_coarse_cdf(p, dens))
        # rays of fewer than 2 samples have a zero CDF
        assert float(got[int(se[1, 0])]) == 0.0
