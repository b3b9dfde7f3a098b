"""The OffsetsSurfs method's fused per-ray kernels (csrc/offsets_render.hip) against the chains of single ops they
replace: per surface, everything downstream of alpha bit-identical to this project's packed ops, alpha itself within
the bound of the Surf kernel, the K-shell blend and all gradients within measured bounds of torch; deterministic; the
coarse CDF over K surfaces bit-identical to its chain at both beta scales."""
import numpy as np
import pytest
import torch

from test_surf_render import ALPHA_ABS_MEASURED, _counts, _pack, _start_end, _Substitute


def _inputs(K, seed, n_rays=256):
    """A pack, K sdfs falling through zero along every ray (spread by a per-surface shift), gradients, normals,
    colours and transparencies."""
    se, S = _start_end(_counts(seed, n_rays))
    p, sdf0 = _pack(se, S, seed + 1)
    g = np.random.default_rng(seed + 2)
    shifts = torch.from_numpy(np.linspace(0.04, -0.04, K).astype(np.float32)).cuda()
    sdfs = (sdf0 + shifts.view(1, K)).contiguous()
    grads = torch.from_numpy(g.standard_normal((S, K, 3)).astype(np.float32) * 0.7).cuda()
    nrm = torch.nn.functional.normalize(grads, dim=-1)
    rgb = torch.from_numpy(g.uniform(0, 1, (S, K, 3)).astype(np.float32)).cuda()
    tr = torch.from_numpy(g.uniform(0, 1, (S, K, 1)).astype(np.float32)).cuda()
    return se, p, sdfs, grads, nrm, rgb, tr


def _chain(p, sdfs, grads, nrm, rgb, tr, rgb_bg, car, beta, decay, alphas=None):
    """offsets_surfs.py render_fg_volumetric (VolumeRenderingNeuS per surface) and render_rays' blend on torch ops
    and this project's packed ops; `alphas` [S,K] substitutes the kernel's alpha downstream."""
    from volsurfs_amd import volsurfs as V
    from volsurfs_amd.surf import neus_alphas_torch
    K = sdfs.shape[1]
    s_rgb, s_alpha, s_depth, s_ws, s_nrm, a_all = [], [], [], [], [], []
    for k in range(K):
        a = neus_alphas_torch(p.samples_dirs, p.samples_dt, sdfs[:, k:k + 1], grads[:, k], car, beta)
        a_all.append(a)
        if alphas is not None:
            a = _Substitute.apply(a, alphas[:, k:k + 1].contiguous())
        T = V.CumprodOneMinusAlphaToTransmittanceFunc.apply(p, 1 - a + 1e-6)[0]
        w = a * T
        t = tr[:, k]
        dec = torch.ones_like(t)
        if decay is not None:
            with torch.no_grad():
                dot = torch.sum(-p.samples_dirs * nrm[:, k], dim=1, keepdim=True).clamp(0.0, 1.0)
                dec = torch.sigmoid(decay * dot) * 2.0 - 1.0
        t = t * dec
        s_rgb.append(V.IntegrateWithWeights3DFunc.apply(p, rgb[:, k].contiguous(), w))
        s_alpha.append(V.IntegrateWithWeights1DFunc.apply(p, t, w))
        with torch.no_grad():
            s_depth.append(V.VolumeRendering.integrate_with_weights_1d(p, p.samples_z, w))
            s_ws.append(V.VolumeRendering.sum_over_rays(p, w)[0])
            s_nrm.append(V.VolumeRendering.integrate_with_weights_3d(p, nrm[:, k].contiguous(), w))
    surfs_rgb, surfs_alpha = torch.stack(s_rgb, 1), torch.stack(s_alpha, 1)
    sr, sa = surfs_rgb.flip(1), surfs_alpha.flip(1)
    trans = torch.cumprod(1 - sa, dim=1)
    if K == 1:
        sT, bgT = torch.ones_like(trans), trans.squeeze(-1)
    else:
        sT = torch.cat([torch.ones_like(trans[:, -1:]), trans[:, :-1]], dim=1)
        bgT = trans[:, -1:].squeeze(-1)
    bw = sT * sa
    rgb_fg = (sr * bw).sum(dim=1)
    N = rgb_fg.shape[0]
    out = rgb_fg if rgb_bg is None else rgb_fg + rgb_bg.expand(N, 3) * bgT
    return {"rgb": out, "rgb_fg": rgb_fg, "bg_transmittance": bgT, "surfs_rgb": surfs_rgb, "surfs_alpha": surfs_alpha,
            "surfs_depths": torch.stack(s_depth, 1), "surfs_weight_sum": torch.stack(s_ws, 1),
            "surfs_normals": torch.stack(s_nrm, 1), "surfs_transmittance": sT.flip(1),
            "surfs_blending_weights": bw.flip(1), "alpha": torch.cat(a_all, 1)}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30)) if a.numel() else 0.0


PER_SURFACE = ("surfs_rgb", "surfs_depths", "surfs_weight_sum", "surfs_normals")
BLEND = ("rgb", "rgb_fg", "bg_transmittance", "surfs_transmittance", "surfs_blending_weights")
# Measured on MI355X over this sweep, as the largest difference over the largest entry; the asserts
# allow twice that.  blend: the K-shell cumprod / sum of torch against the kernel's sequential loop;
# decay: the transparency integral with the decay on (torch.sigmoid against 1 / (1 + expf(-x)));
# grads: every input gradient against the chain fed the kernel's alpha (the torch prologue for g_sdfs / g_grads).
BLEND_REL_MEASURED = 6.6e-7
DECAY_REL_MEASURED = 2.2e-6
GRAD_REL_MEASURED = 3.9e-5

BETAS = (float(np.exp(7.0)), float(np.exp(10.0)))
CARS = (0.0, 0.5, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 5, 9])
@pytest.mark.parametrize("bug_compat", [True, False])
@pytest.mark.parametrize("bg", [None, "per_ray", "constant"])
@pytest.mark.parametrize("decay", [None, 300.0])
def test_offsets_composite_equals_the_op_chain(K, bug_compat, bg, decay):
    from volsurfs_amd import volsurfs as V
    from volsurfs_amd.offsets_surfs import offsets_composite
    se, p, sdfs0, grads0, nrm, rgb0, tr0 = _inputs(K, 3 + K)
    N = se.shape[0]
    g = np.random.default_rng(11)
    bgc = None if bg is None else torch.from_numpy(
        g.uniform(0, 1, (N, 3) if bg == "per_ray" else (1, 3)).astype(np.float32)).cuda()
    g_rgb = torch.from_numpy(g.standard_normal((N, 3)).astype(np.float32)).cuda()
    V.VolumeRendering.bug_compat = bug_compat
    worst = {"blend": 0.0, "decay": 0.0, "grad": 0.0, "alpha": 0.0}
    try:
        for car in CARS:
            for beta in BETAS:
                runs = {}
                for name in ("fused", "fused2", "chain", "chain_kalpha"):
                    s = sdfs0.clone().requires_grad_(True)
                    gr = grads0.clone().requires_grad_(True)
                    c = rgb0.clone().requires_grad_(True)
                    t = tr0.clone().requires_grad_(True)
                    b = None if bgc is None else bgc.clone().requires_grad_(True)
                    if name.startswith("fused"):
                        out = offsets_composite(p, s, gr, nrm, c, t, b, car, beta, decay, return_alpha=True)
                    else:
                        out = _chain(p, s, gr, nrm, c, t, b, car, beta, decay,
                                     runs["fused"]["alpha"] if name == "chain_kalpha" else None)
                    (out["rgb"] * g_rgb).sum().backward()
                    r = {k: out[k].detach() for k in PER_SURFACE + BLEND + ("surfs_alpha", "alpha")}
                    r.update(g_sdfs=s.grad, g_grads=gr.grad, g_rgb=c.grad, g_tr=t.grad,
                             g_bg=None if b is None else b.grad)
                    runs[name] = r
                f, f2, ch, chk = runs["fused"], runs["fused2"], runs["chain"], runs["chain_kalpha"]
                for k, v in f.items():
                    if v is not None:
                        assert torch.equal(v, f2[k]), ("not deterministic", k)
                # per surface, downstream of alpha: the packed ops' bits
                for k in PER_SURFACE + (() if decay else ("surfs_alpha",)):
                    assert torch.equal(f[k].reshape(chk[k].shape), chk[k]), (k, float((f[k] - chk[k]).abs().max()))
                if decay:
                    worst["decay"] = max(worst["decay"], _rel(f["surfs_alpha"], chk["surfs_alpha"]))
                for k in BLEND:
                    worst["blend"] = max(worst["blend"], _rel(f[k].reshape(chk[k].shape), chk[k]))
                for k in ("g_rgb", "g_tr", "g_bg"):
                    if f[k] is not None:
                        worst["grad"] = max(worst["grad"], _rel(f[k], chk[k]))
                for k in ("g_sdfs", "g_grads"):
                    worst["grad"] = max(worst["grad"], _rel(f[k], chk[k]))
                worst["alpha"] = max(worst["alpha"], float((f["alpha"] - ch["alpha"]).abs().max()))
                # the empty rays: no foreground, full background
                assert float(f["bg_transmittance"][0]) == 1.0 and float(f["bg_transmittance"][6]) == 1.0
        print(f"offsets composite K={K} bug_compat={bug_compat} bg={bg} decay={decay}: alpha {worst['alpha']:.3e}, "
              f"blend {worst['blend']:.3e}, decay {worst['decay']:.3e}, grads {worst['grad']:.3e} of the largest entry")
        assert worst["alpha"] <= 2 * ALPHA_ABS_MEASURED
        assert worst["blend"] <= 2 * BLEND_REL_MEASURED
        assert worst["decay"] <= 2 * DECAY_REL_MEASURED
        assert worst["grad"] <= 2 * GRAD_REL_MEASURED
    finally:
        V.VolumeRendering.bug_compat = True


@pytest.mark.gpu
def test_offsets_composite_without_samples_and_too_many_surfaces():
    from volsurfs_amd._lib import VolsurfsHipError
    from volsurfs_amd.offsets_surfs import offsets_composite, sdfs_coarse_cdf
    from volsurfs_amd.volsurfs import RaySamplesPacked
    e = RaySamplesPacked(3, 0, 0, 0)
    e.ray_start_end_idx = torch.zeros(3, 2, dtype=torch.int32, device="cuda")
    e.is_compacted, e.has_dt = True, True
    e.samples_dt = e.samples_z = torch.zeros(0, 1, device="cuda")
    e.samples_dirs = torch.zeros(0, 3, device="cuda")
    z = lambda *s: torch.zeros(*s, device="cuda")
    bg = torch.tensor([0.2, 0.4, 0.6], device="cuda")
    out = offsets_composite(e, z(0, 3), z(0, 3, 3), z(0, 3, 3), z(0, 3, 3), z(0, 3, 1), bg, 0.5, 100.0, 50.0)
    assert torch.equal(out["rgb"], bg.view(1, 3).expand(3, 3))
    assert torch.equal(out["surfs_transmittance"], torch.ones(3, 3, 1, device="cuda"))
    se, p, sdfs, grads, nrm, rgb, tr = _inputs(3, 5, 64)
    S = sdfs.shape[0]
    with pytest.raises(VolsurfsHipError):
        offsets_composite(p, z(S, 17), z(S, 17, 3), z(S, 17, 3), z(S, 17, 3), z(S, 17, 1))
    with pytest.raises(VolsurfsHipError):
        sdfs_coarse_cdf(p, z(S, 17), 100.0)
    # the C ABI refuses K outside 1..16 itself (VSA_ERR_UNSUPPORTED = -2), before any launch; the buffers are sized
    # for the K asked, so nothing would be out of bounds even without the check
    from volsurfs_amd import _lib
    N = p.get_nr_rays()
    st = _lib.stream_ptr()
    for K in (0, 17):
        Kb = max(K, 1)
        with pytest.raises(VolsurfsHipError, match="status -2"):
            _lib.call("vsa_sdfs_coarse_cdf", p.ray_start_end_idx, K, z(S, Kb), p.samples_dt, 100.0, z(S, 1), N, st)
        with pytest.raises(VolsurfsHipError, match="status -2"):
            _lib.call("vsa_offsets_composite_fwd", p.ray_start_end_idx, K, z(S, Kb), z(S, Kb, 3), z(S, Kb, 3),
                      z(S, Kb, 3), z(S, Kb), p.samples_dirs, p.samples_dt, p.samples_z, None, 0, 1.0, 100.0, 0, 0.0,
                      z(N, Kb, 3), z(N, Kb, 3), z(N, Kb), z(N, Kb), z(N, Kb), z(N, Kb), z(N, Kb), z(N, 3), z(N, 1),
                      z(N, 3), None, N, st)
        with pytest.raises(VolsurfsHipError, match="status -2"):
            _lib.call("vsa_offsets_composite_bwd", p.ray_start_end_idx, K, z(S, Kb), z(S, Kb, 3), z(S, Kb, 3),
                      z(S, Kb, 3), z(S, Kb), p.samples_dirs, p.samples_dt, None, 0, 1.0, 100.0, 0, 0.0, z(N, Kb, 3),
                      z(N, Kb), z(N, Kb), z(N, 1), z(N, 3), z(S, Kb), z(S, Kb, 3), z(S, Kb, 3), z(S, Kb), None,
                      z(2 * S * Kb), N, 1, st)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 5, 9])
def test_sdfs_coarse_cdf_equals_the_op_chain(K):
    from volsurfs_amd import volsurfs as V
    from volsurfs_amd.offsets_surfs import sdfs_coarse_cdf
    for beta in BETAS:
        se, p, sdfs, *_ = _inputs(K, 20 + K, 512)
        for scale in ("half", "full"):
            # utils/sdfs_utils.py:12-64 with beta / 2 and beta
            value = beta / 2.0 if scale == "half" else beta
            lb = torch.ones_like(p.samples_dt) * value
            agg = torch.zeros_like(p.samples_dt)
            for k in range(K):
                alpha = V.VolumeRendering.sdf2alpha(p, sdfs[:, k:k + 1].contiguous(), lb)
                T, _ = V.VolumeRendering.cumprod_one_minus_alpha_to_transmittance(p, 1 - alpha + 1e-6)
                T = T.clip(0.0, 1.0)
                w = alpha * T
                _, ws = V.VolumeRendering.sum_over_rays(p, w)
                w /= torch.clip(ws, min=1e-6)
                agg += V.VolumeRendering.compute_cdf(p, w)
            want = agg / K
            b32 = np.float32(beta) / np.float32(2.0) if scale == "half" else np.float32(beta)
            got = sdfs_coarse_cdf(p, sdfs.unsqueeze(-1), b32)
            assert torch.equal(got, want), (K, scale, float((got - want).abs().max()))
            assert torch.equal(got, sdfs_coarse_cdf(p, sdfs, b32))
            assert float(got[int(se[1, 0])]) == 0.0     # a 1-sample ray has a zero CDF
