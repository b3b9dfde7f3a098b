"""The Surf method's fused per-ray kernels (csrc/surf_render.hip) against the chains of single ops they replace: the
NeuS prologue against its torch elementwise restatement, everything downstream of alpha bit-identical to this
project's packed ops, deterministic; the coarse CDF bit-identical to its chain for both beta scales."""
import numpy as np
import pytest
import torch


def _start_end(counts):
    counts = np.asarray(counts, np.int64)
    ends = np.cumsum(counts)
    return np.stack([ends - counts, ends], 1).astype(np.int32), int(ends[-1]) if len(ends) else 0


def _counts(seed, n_rays=512):
    """Empty rays, 1-sample rays and the chunk edges 31 / 32 / 33 plus a 96-sample ray, among random lengths."""
    g = np.random.default_rng(seed)
    c = g.integers(0, 97, n_rays)
    c[:8] = [0, 1, 31, 32, 33, 96, 0, 1]
    return c


def _pack(se, S, seed):
    """A compacted pack with dt, z and unit directions; an SDF falling through zero along every ray."""
    from volsurfs_amd.volsurfs import RaySamplesPacked
    g = np.random.default_rng(seed)
    N = se.shape[0]
    p = RaySamplesPacked(N, S, 0, 0)
    p.ray_start_end_idx = torch.from_numpy(se).cuda()
    p.is_compacted = True
    dt = g.uniform(1e-3, 0.05, (S, 1)).astype(np.float32)
    z = np.zeros((S, 1), np.float32)
    sdf = np.zeros((S, 1), np.float32)
    for a, b in se:
        z[a:b, 0] = 0.1 + np.cumsum(dt[a:b, 0])
        sdf[a:b, 0] = g.uniform(0.05, 0.3) - (z[a:b, 0] - 0.1) * g.uniform(0.5, 1.5) + g.normal(0, 0.01, b - a)
    dirs = g.standard_normal((S, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    p.samples_dt = torch.from_numpy(dt).cuda()
    p.samples_z = torch.from_numpy(z).cuda()
    p.samples_dirs = torch.from_numpy(dirs).cuda()
    p.has_dt = True
    return p, torch.from_numpy(sdf).cuda()


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


class _Substitute(torch.autograd.Function):
    """Forward: the value `b`; backward: the gradient goes to `a` (feeds the chain the kernel's alpha while the
    torch prologue still receives the chain's gradient)."""

    @staticmethod
    def forward(ctx, a, b):
        return b.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _chain(p, sdf, grad, normals, rgb, rgb_bg, car, beta, alpha_override=None):
    """surf.py render_fg_volumetric (VolumeRenderingNeuS) and the blend of render_rays on torch elementwise ops
    and this project's packed ops."""
    from volsurfs_amd import volsurfs as V
    from volsurfs_amd.surf import neus_alphas_torch
    alpha = neus_alphas_torch(p.samples_dirs, p.samples_dt, sdf, grad, car, beta)
    if alpha_override is not None:
        alpha = _Substitute.apply(alpha, alpha_override)
    T, _ = V.CumprodOneMinusAlphaToTransmittanceFunc.apply(p, 1 - alpha + 1e-6)
    w = alpha * T
    wsum, _ = V.SumOverRaysFunc.apply(p, w)
    bgT = 1 - wsum
    rgb_fg = V.IntegrateWithWeights3DFunc.apply(p, rgb, w)
    depth = V.VolumeRendering.integrate_with_weights_1d(p, p.samples_z, w.detach())
    nrm = V.VolumeRendering.integrate_with_weights_3d(p, normals, w.detach())
    rgb_out = _Blend.apply(rgb_fg, bgT, rgb_bg) if rgb_bg is not None else rgb_fg
    return {"rgb": rgb_out, "rgb_fg": rgb_fg, "weights_sum": wsum, "depth": depth, "normals": nrm, "weights": w,
            "alpha": alpha}


def _ulp(a, b):
    """Largest distance in units in the last place between two fp32 tensors (0 for +0 / -0)."""
    def key(t):
        i = t.detach().contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max()) if a.numel() else 0


def _rel_max(a, b):
    """max |a - b| over max |b|."""
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30)) if a.numel() else 0.0


# Measured on MI355X over this sweep: the kernel's alpha against the torch restatement (max abs
# difference; torch.sigmoid is not 1 / (1 + expf(-x)) to the last bit, and (pc - nc) + 1e-6 magnifies an ulp of
# either sigmoid) and the prologue's gradients (through the torch prologue fed the same downstream gradient, as a
# fraction of the largest entry).  The asserts allow twice that.
ALPHA_ABS_MEASURED = 2.5e-6
G_SDF_REL_MEASURED = 9.4e-7
G_GRAD_REL_MEASURED = 1.1e-6

BETAS = (float(np.exp(3.0)), float(np.exp(7.0)))


@pytest.mark.gpu
@pytest.mark.parametrize("bug_compat", [True, False])
@pytest.mark.parametrize("bg", [None, "per_ray", "constant"])
@pytest.mark.parametrize("car", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("beta", BETAS)
def test_neus_composite_equals_the_op_chain(bug_compat, bg, car, beta):
    from volsurfs_amd import volsurfs as V
    from volsurfs_amd.surf import neus_composite
    se, S = _start_end(_counts(3))
    p, sdf0 = _pack(se, S, 4)
    N = se.shape[0]
    g = np.random.default_rng(5)
    grad0 = torch.from_numpy(g.standard_normal((S, 3)).astype(np.float32) * 0.7).cuda()
    nrm = torch.nn.functional.normalize(grad0, dim=1)
    col = torch.from_numpy(g.uniform(0, 1, (S, 3)).astype(np.float32)).cuda()
    bgc = None if bg is None else torch.from_numpy(
        g.uniform(0, 1, (N, 3) if bg == "per_ray" else (1, 3)).astype(np.float32)).cuda()
    g_rgb = torch.from_numpy(g.standard_normal((N, 3)).astype(np.float32)).cuda()
    g_ws = torch.from_numpy(g.standard_normal((N, 1)).astype(np.float32)).cuda()
    V.VolumeRendering.bug_compat = bug_compat
    try:
        runs = {}
        for name in ("fused", "fused2", "chain", "chain_kalpha"):
            s = sdf0.clone().requires_grad_(True)
            gr = grad0.clone().requires_grad_(True)
            c = col.clone().requires_grad_(True)
            b = None if bgc is None else bgc.clone().requires_grad_(True)
            if name.startswith("fused"):
                out = neus_composite(p, s, gr, nrm, c, b, car, beta, return_weights=True)
            else:
                out = _chain(p, s, gr, nrm, c, b, car, beta,
                             runs["fused"]["alpha"] if name == "chain_kalpha" else None)
            loss = (out["rgb"] * g_rgb).sum() + (out["weights_sum"] * g_ws).sum()
            loss.backward()
            runs[name] = {k: out[k].detach() for k in ("rgb", "rgb_fg", "weights_sum", "depth", "normals", "weights",
                                                        "alpha")}
            runs[name].update(g_sdf=s.grad, g_grad=gr.grad, g_rgb=c.grad, g_bg=None if b is None else b.grad)
        f, f2, ch, chk = runs["fused"], runs["fused2"], runs["chain"], runs["chain_kalpha"]
        for k, v in f.items():
            if v is not None:
                assert torch.equal(v, f2[k]), ("not deterministic", k)
        # downstream of alpha: bit-identical to the packed ops fed the kernel's alpha
        for k in ("rgb", "rgb_fg", "weights_sum", "depth", "normals", "weights", "g_rgb"):
            assert torch.equal(f[k], chk[k]), (k, float((f[k] - chk[k]).abs().max()))
        if bg == "per_ray":
            assert torch.equal(f["g_bg"], chk["g_bg"])
        elif bg == "constant":
            # the constant colour's gradient is a torch reduction over the rays on both sides
            torch.testing.assert_close(f["g_bg"], chk["g_bg"], rtol=1e-5, atol=1e-5)
        # the prologue against its torch restatement
        a_abs = float((f["alpha"] - ch["alpha"]).abs().max())
        rs, rg = _rel_max(f["g_sdf"], chk["g_sdf"]), _rel_max(f["g_grad"], chk["g_grad"])
        print(f"neus prologue bug_compat={bug_compat} bg={bg} car={car} beta={beta:.1f}: alpha {a_abs:.3e} "
              f"({_ulp(f['alpha'], ch['alpha'])} ulp), g_sdf {rs:.3e}, g_sdf_grad {rg:.3e} of the largest entry")
        assert a_abs <= 2 * ALPHA_ABS_MEASURED
        assert rs <= 2 * G_SDF_REL_MEASURED and rg <= 2 * G_GRAD_REL_MEASURED
        # the empty rays: no foreground
        assert float(f["weights_sum"][0]) == 0.0 and float(f["weights_sum"][6]) == 0.0
    finally:
        V.VolumeRendering.bug_compat = True


@pytest.mark.gpu
def test_neus_composite_without_samples():
    from volsurfs_amd.surf import neus_composite
    from volsurfs_amd.volsurfs import RaySamplesPacked
    e = RaySamplesPacked(3, 0, 0, 0)
    e.ray_start_end_idx = torch.zeros(3, 2, dtype=torch.int32, device="cuda")
    e.is_compacted, e.has_dt = True, True
    e.samples_dt = e.samples_z = torch.zeros(0, 1, device="cuda")
    e.samples_dirs = torch.zeros(0, 3, device="cuda")
    z3 = torch.zeros(0, 3, device="cuda")
    bg = torch.tensor([0.2, 0.4, 0.6], device="cuda")
    out = neus_composite(e, torch.zeros(0, 1, device="cuda"), z3, z3, z3, bg, 0.5, 100.0)
    assert torch.equal(out["rgb"], bg.view(1, 3).expand(3, 3)) and torch.equal(out["weights_sum"],
                                                                               torch.zeros(3, 1, device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("beta", BETAS)
def test_sdf_coarse_cdf_equals_the_op_chain(beta):
    from volsurfs_amd import volsurfs as V
    from volsurfs_amd.surf import sdf_coarse_cdf
    for seed in (7, 8):
        se, S = _start_end(_counts(seed))
        p, sdf = _pack(se, S, seed + 1)
        for scale in ("half", "full"):
            # utils/sdf_utils.py:87-109 (beta / 2) and :153-175 (beta)
            lb = torch.ones_like(p.samples_dt) * beta
            if scale == "half":
                lb = lb / 2.0
            alpha = V.VolumeRendering.sdf2alpha(p, sdf, lb)
            T, _ = V.VolumeRendering.cumprod_one_minus_alpha_to_transmittance(p, 1 - alpha + 1e-6)
            w = alpha * T
            _, ws = V.VolumeRendering.sum_over_rays(p, w)
            ws = torch.clip(ws, min=1e-6)
            w /= ws
            want = V.VolumeRendering.compute_cdf(p, w)
            b32 = np.float32(beta) / np.float32(2.0) if scale == "half" else np.float32(beta)
            got = sdf_coarse_cdf(p, sdf, b32)
            assert torch.equal(got, want), (seed, scale, float((got - want).abs().max()))
            assert torch.equal(got, sdf_coarse_cdf(p, sdf, b32))
            assert float(got[int(se[1, 0])]) == 0.0     # a 1-sample ray has a zero CDF
