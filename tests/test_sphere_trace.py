"""Sphere tracing (volsurfs_amd/sphere_trace.py, csrc/sphere_trace.hip) and the sphere-traced render of Surf and
OffsetsSurfs: the restatement of the reference's masked loop against the fixture recorded from the reference's own
loop (tools/make_sphere_trace_golden.py), the device loop against the fixture and against the restatement, the batched
columns, the blend kernel, and the two methods' renders on a sphere-initialised field."""
import math
import os

import numpy as np
import pytest
import torch

import sphere_trace_restated as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "sphere_trace.npz")
CASES = [f"{f}_{s}" for s in R.FIXTURE_SETTINGS for f in R.FIXTURE_FIELDS]

# Bounds of the fixture test.  The reference's own float32 / float64 gap on these cases (make_sphere_trace_golden.py
# --check64): 0 flipped flags of 2304 in all ten cases, points within 6.2e-7 on hits and within 9.0e-5 on the other
# rays (rays that graze the bounding sphere, whose near point is ill-conditioned).
MAX_FLIPS = 12                  # 0.5 % of the rays of a case: a condition, the reference flips none
HIT_POINT_TOL = 1e-5            # rays both sides flag as hits: 1 % of the convergence threshold
OTHER_POINT_TOL = 1e-4          # rays that left the sphere or ran out of rounds: one long step, no render reads them


def _case(name):
    f, s = name.rsplit("_", 1)
    fn, surf_idx = R.FIXTURE_FIELDS[f]
    rounds, thresh = R.FIXTURE_SETTINGS[s]
    return fn, surf_idx, rounds, thresh


# ---- CPU

@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_fixture_on_cpu(case):
    """The masked loop restated in torch gives the bytes the reference's own loop gave (float32, same torch ops)."""
    d = np.load(GOLDEN)
    o, dirs = torch.from_numpy(d["rays_o"]), torch.from_numpy(d["rays_d"])
    o2, d2 = R.fixture_rays()
    assert torch.equal(o, o2) and torch.equal(dirs, d2)
    fn, surf_idx, rounds, thresh = _case(case)
    prim = R.TorchBoundingSphere(float(d["radius"]))
    for uah, key in ((False, "_hit"), (True, "_hit_unconverged")):
        stats = {}
        p, z, hit = R.sphere_trace_restated(fn, o, dirs, prim, rounds, thresh, surf_idx=surf_idx,
                                            unconverged_are_hits=uah, stats=stats)
        assert torch.equal(p, torch.from_numpy(d[case + "_points"]))
        assert torch.equal(z, torch.from_numpy(d[case + "_z"]))
        assert torch.equal(hit, torch.from_numpy(d[case + key]))
        assert 0 < stats["rounds"] <= rounds and stats["masked_ops"] >= 9 * stats["rounds"]
    if surf_idx is not None:        # an int index means that column kept as [M, 1]
        p2, _, hit2 = R.sphere_trace_restated(fn, o, dirs, prim, rounds, thresh, surf_idx=surf_idx[0])
        assert torch.equal(p2, torch.from_numpy(d[case + "_points"])) and \
            torch.equal(hit2, torch.from_numpy(d[case + "_hit"]))


def _blend_inputs(N, K, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(N, K, 3, generator=g)
    alpha = torch.rand(N, K, 1, generator=g)
    pick = torch.rand(N, K, 1, generator=g)
    alpha = torch.where(pick < 0.15, torch.zeros_like(alpha), torch.where(pick > 0.85, torch.ones_like(alpha), alpha))
    return rgb.to(device), alpha.to(device)


def test_header_declares_the_sphere_trace_entry_points():
    import ctypes
    from volsurfs_amd import _lib
    names = ["vsa_st_begin", "vsa_st_step", "vsa_st_finish", "vsa_st_scatter", "vsa_st_blend"]
    declared, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    for n in names:
        assert n in declared and n in protos and protos[n][0] is ctypes.c_int
    assert len(protos["vsa_st_step"][1]) == 21 and protos["vsa_st_step"][1][7] is ctypes.c_float
    assert protos["vsa_st_scatter"][1][1] is ctypes.c_longlong
    assert len(protos["vsa_st_blend"][1]) == 9


# ---- GPU: the loop

def _fixture_on_device():
    from volsurfs_amd.background import BoundingSphere
    d = np.load(GOLDEN)
    return d, torch.from_numpy(d["rays_o"]).cuda(), torch.from_numpy(d["rays_d"]).cuda(), \
        BoundingSphere(float(d["radius"]))


@pytest.mark.gpu
def test_fixture_cases_on_the_device():
    """sphere_trace with the fixture's fields evaluated by torch on the device against the reference's recorded
    results.  Measured on MI355X: 0 flipped flags in all twenty runs, points within 1.6e-7 on hits and
    9.8e-6 on the other rays, samples_z within 2.4e-7 and 1.1e-5."""
    from volsurfs_amd.sphere_trace import sphere_trace
    d, o, dirs, prim = _fixture_on_device()
    worst = {"flips": 0, "hit": 0.0, "other": 0.0, "z_hit": 0.0, "z_other": 0.0}
    failures = []
    for case in CASES:
        fn, surf_idx, rounds, thresh = _case(case)
        for uah, key in ((False, "_hit"), (True, "_hit_unconverged")):
            pack, hit = sphere_trace(fn, o, dirs, prim, nr_sphere_traces=rounds, sdf_converged_tresh=thresh,
                                     surf_idx=surf_idx, unconverged_are_hits=uah)
            assert pack.samples_3d.shape == (o.shape[0], 3) and pack.samples_z.shape == (o.shape[0], 1)
            assert hit.dtype == torch.bool and hit.shape == (o.shape[0],)
            ref_hit = torch.from_numpy(d[case + key]).cuda()
            ref_p, ref_z = torch.from_numpy(d[case + "_points"]).cuda(), torch.from_numpy(d[case + "_z"]).cuda()
            same = hit == ref_hit
            flips = int((~same).sum())
            worst["flips"] = max(worst["flips"], flips)
            if uah:     # the same points; only the flags of the rays that ran out of rounds change
                print(f"sphere_trace fixture {case} unconverged_are_hits: {int(hit.sum())} hits, {flips} flips")
                if flips > MAX_FLIPS:
                    failures.append((case, uah, flips))
                continue
            both, other = same & hit, same & ~hit
            gap = (pack.samples_3d - ref_p).abs().amax(-1)
            zgap = (pack.samples_z - ref_z).abs()[:, 0]
            mx = lambda t, m: float(t[m].max()) if bool(m.any()) else 0.0
            g = (mx(gap, both), mx(gap, other), mx(zgap, both), mx(zgap, other))
            print(f"sphere_trace fixture {case}: {int(hit.sum())} hits, {flips} flips, max point gap {g[0]:.2e} on "
                  f"hits / {g[1]:.2e} elsewhere, z gap {g[2]:.2e} / {g[3]:.2e}")
            for k, v in zip(("hit", "other", "z_hit", "z_other"), g):
                worst[k] = max(worst[k], v)
            if flips > MAX_FLIPS or g[0] > HIT_POINT_TOL or g[1] > OTHER_POINT_TOL or g[2] > HIT_POINT_TOL or \
                    g[3] > OTHER_POINT_TOL:
                failures.append((case, uah, flips, g))
    print("sphere_trace fixture worst:", worst)
    assert not failures, failures


def _assert_same_as_restatement(sdf_fn, o, dirs, prim, rounds, thresh, surf_idx=None, uah=False, iter_nr=None):
    from volsurfs_amd.sphere_trace import sphere_trace
    pack, hit = sphere_trace(sdf_fn, o, dirs, prim, nr_sphere_traces=rounds, sdf_converged_tresh=thresh,
                             surf_idx=surf_idx, unconverged_are_hits=uah, iter_nr=iter_nr)
    p, z, h = R.sphere_trace_restated(sdf_fn, o, dirs, prim, rounds, thresh, iter_nr=iter_nr, surf_idx=surf_idx,
                                      unconverged_are_hits=uah)
    assert torch.equal(hit, h), f"{int((hit != h).sum())} flags differ"
    assert torch.equal(pack.samples_3d, p), f"max point gap {float((pack.samples_3d - p).abs().max()):.3e}"
    # z: torch's norm kernel and the trace's sqrt of the ordered sum of squares may round differently: 2 ulp of a
    # distance below 2
    assert float((pack.samples_z - z).abs().max()) <= 2 * 2.0 ** -22
    return pack, hit


@pytest.mark.gpu
def test_analytic_fields_match_the_restatement_on_the_device_bit_for_bit():
    _, o, dirs, prim = _fixture_on_device()
    for case in CASES:
        fn, surf_idx, rounds, thresh = _case(case)
        for uah in (False, True):
            _, hit = _assert_same_as_restatement(fn, o, dirs, prim, rounds, thresh, surf_idx, uah)
        assert int(hit.sum()) > 0
    # a cube as the bounding primitive (kind 0)
    from volsurfs_amd.background import BoundingBox
    _assert_same_as_restatement(R.sdf_torus, o, dirs, BoundingBox(0.9), 100, 1e-3)


SPHERE_R = 0.3


@pytest.fixture(scope="module")
def sphere_surf(tmp_path_factory):
    """A Surf method whose SDF went through 300 sphere-init iterations to radius 0.3 (as test_offsets_surfs_method's
    _surf_ckpt trains it), saved; -> (method, its models folder)."""
    from test_surf_method import _cameras, _gt_images, _method as surf_method
    from volsurfs_amd.camera import TensorReel
    from volsurfs_amd.trainer import train
    torch.manual_seed(0)
    tmp = tmp_path_factory.mktemp("sphere_surf")
    iters = 300
    m = surf_method(bg_color=(0.0, 0.0, 0.0), init_sphere_radius=SPHERE_R, save=str(tmp / "surf"),
                    hp={"lr": 3e-3, "init_phase_end_iter": iters + 1, "sdf_nr_iters_for_c2f": 0})
    cams = _cameras(4)
    train(TensorReel(cams, _gt_images(cams)), m, 0, iters, nr_training_rays=512)
    m.is_training = False
    return m, m.save(iters)


def _row_is_batch_independent(fn):
    """1000 points evaluated alone and inside a batch of 100 000: the same bytes?"""
    g = torch.Generator("cuda").manual_seed(5)
    big = (torch.rand(100000, 3, device="cuda", generator=g) - 0.5) * 0.8
    a = 40000
    with torch.no_grad():
        alone, inside = fn(big[a:a + 1000].contiguous()), fn(big)[a:a + 1000]
    return torch.equal(alone, inside)


def _view_rays(H=64, eye=(0.0, 0.0, 1.5), focal=70.0):
    from volsurfs_amd.camera import Camera, get_camera_rays
    cam = Camera.look_at(eye, focal=focal, height=H, width=H)
    o, d, _ = get_camera_rays(cam)
    return cam, o, d


@pytest.mark.gpu
def test_sdf_model_matches_the_restatement_on_the_device(sphere_surf):
    """models.SDF (permutohedral encoder + fused MLP) after the sphere init: the loop evaluates the SDF in launches
    of other row counts than the restatement (padding, lagged bounds), so first the premise — a row's output does not
    depend on the batch it is in — then bit identity."""
    m, _ = sphere_surf
    sdf = m.models["sdf"]
    assert _row_is_batch_independent(lambda p: sdf.main_sdf(p)[0])
    _, o, dirs = _view_rays()
    for rounds, thresh, uah in ((100, 1e-3, False), (8, 1e-4, True)):
        _, hit = _assert_same_as_restatement(sdf.main_sdf, o, dirs, m.bounding_primitive, rounds, thresh, uah=uah)
        assert 0 < int(hit.sum()) < hit.numel()


def _offsets_sdf(ckpt_folder, nr_inner, nr_outer, head_bias=-4.0):
    """An OffsetsSDF on the sphere-initialised main surface whose heads give offsets of about softplus(head_bias)."""
    from volsurfs_amd.models import OffsetsSDF
    s = OffsetsSDF(in_channels=3, mlp_layers_dims=[32, 32, 32], encoding_type="permutohash", nr_inner_surfs=nr_inner,
                   nr_outer_surfs=nr_outer, geom_feat_size=32, nr_iters_for_c2f=0, bb_sides=1.0)
    s.load_main_sdf_ckpt(os.path.join(ckpt_folder, "sdf.pt"))
    with torch.no_grad():
        for h in s.mlps_eps:
            list(h.parameters())[-1].fill_(head_bias)
    return s


@pytest.mark.gpu
def test_offsets_sdf_columns_match_the_restatement_and_separate_calls(sphere_surf):
    """OffsetsSDF with K = 5: every column against the restatement, and sphere_trace_columns against K separate
    sphere_trace calls, bit for bit; two runs give the same bytes."""
    from volsurfs_amd.sphere_trace import sphere_trace, sphere_trace_columns
    m, folder = sphere_surf
    s = _offsets_sdf(folder, 2, 2)
    assert _row_is_batch_independent(lambda p: s(p)[0])
    prim = m.bounding_primitive
    _, o, dirs = _view_rays()
    single = []
    for k in range(5):
        pack, hit = _assert_same_as_restatement(s, o, dirs, prim, 100, 1e-3, surf_idx=k)
        pack_l, hit_l = sphere_trace(s, o, dirs, prim, nr_sphere_traces=100, sdf_converged_tresh=1e-3, surf_idx=[k])
        assert torch.equal(pack_l.samples_3d, pack.samples_3d) and torch.equal(hit_l, hit)
        single.append((pack, hit))
    counts = [int(h.sum()) for _, h in single]
    assert counts[0] > 0 and all(a <= b for a, b in zip(counts, counts[1:])) and counts[0] < counts[-1]
    for run in range(2):
        batched = sphere_trace_columns(s, o, dirs, prim, list(range(5)), nr_sphere_traces=100,
                                       sdf_converged_tresh=1e-3)
        for (pa, ha), (pb, hb) in zip(single, batched):
            assert torch.equal(ha, hb)
            assert torch.equal(pa.samples_3d, pb.samples_3d) and torch.equal(pa.samples_z, pb.samples_z)
    # a subset in another order
    sub = sphere_trace_columns(s, o, dirs, prim, [3, 1], nr_sphere_traces=100, sdf_converged_tresh=1e-3)
    assert torch.equal(sub[0][0].samples_3d, single[3][0].samples_3d) and torch.equal(sub[1][1], single[1][1])


@pytest.mark.gpu
def test_edge_sizes_misses_and_one_round():
    from volsurfs_amd.background import BoundingSphere
    from volsurfs_amd.sphere_trace import sphere_trace, sphere_trace_columns, stats_summary
    _, o, dirs, prim = _fixture_on_device()
    for n in (0, 1, 65):
        pack, hit = sphere_trace(R.sdf_torus, o[:n].contiguous(), dirs[:n].contiguous(), prim, 100, 1e-3)
        assert pack.samples_3d.shape == (n, 3) and pack.samples_z.shape == (n, 1) and hit.shape == (n,)
        if n:
            _assert_same_as_restatement(R.sdf_torus, o[:n].contiguous(), dirs[:n].contiguous(), prim, 100, 1e-3)
    assert sphere_trace_columns(R.sdf_three_columns, o[:0], dirs[:0], prim, [0, 1])[1][1].shape == (0,)
    # the first rows of the fixture view with a sphere they all miss: every ray starts at its origin, takes one step and
    # is done (outside); no hits
    far = BoundingSphere(0.05)
    oo, dd = o[:200].contiguous(), dirs[:200].contiguous()
    assert not bool(far.intersect(oo, dd)[0].any())
    pack, hit = _assert_same_as_restatement(R.sdf_torus, oo, dd, far, 100, 1e-3)
    assert not bool(hit.any())
    s = stats_summary()
    assert s["live"][0] == 200 and sum(s["live"][1:]) == 0 and s["rounds"] <= 1 + 2
    assert torch.equal(pack.samples_3d, oo + dd * R.sdf_torus(oo))
    # one round
    for uah in (False, True):
        _assert_same_as_restatement(R.sdf_two_balls, o, dirs, prim, 1, 1e-3, uah=uah)
    # 65 rays x 3 columns
    b = sphere_trace_columns(R.sdf_three_columns, o[1000:1065].contiguous(), dirs[1000:1065].contiguous(), prim,
                             [0, 1, 2], 100, 1e-3)
    for k in range(3):
        pk, hk = sphere_trace(R.sdf_three_columns, o[1000:1065].contiguous(), dirs[1000:1065].contiguous(), prim, 100,
                              1e-3, surf_idx=k)
        assert torch.equal(b[k][0].samples_3d, pk.samples_3d) and torch.equal(b[k][1], hk)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 5, 9])
def test_blend_kernel_is_the_reference_expression_bit_for_bit(K):
    """vsa_st_blend against the flip / cumprod / sum expression evaluated by torch on the device."""
    from volsurfs_amd.sphere_trace import blend_surfaces
    for N in (7, 3001):
        rgb, alpha = _blend_inputs(N, K, 10 + K, "cuda")
        assert N < 100 or (bool((alpha == 0).any()) and bool((alpha == 1).any()))
        want = R.blend_restated(rgb, alpha)
        got = blend_surfaces(rgb, alpha)
        for name, a, b in zip(("surfs_transmittance", "surfs_blending_weights", "rgb_fg", "bg_transmittance"), got, want):
            assert a.shape == b.shape, name
            assert torch.equal(a, b), (name, N)


# ---- GPU: the methods

ST_KEYS = {"rgb_fg", "depth_fg", "weights_sum", "bg_transmittance", "normals"}
VOL_KEYS = {"rgb", "rgb_fg", "rgb_bg", "depth_fg", "depth_bg", "depth", "weights_sum", "bg_transmittance", "normals",
            "nr_samples"}
MAX_INCIDENCE_COS = 0.5         # hits steeper than 60 degrees are left out of the depth and normal checks


@pytest.mark.gpu
def test_surf_sphere_traced_render_of_a_sphere_initialised_field(sphere_surf):
    """render_fg_sphere_traced on a 64 x 64 view of the field initialised to a ball of radius 0.3.

    The bounds come from the field's own error, measured here before the render: e = max |sdf(p)| over points of the
    ball's surface, and the largest angle between the stencil gradient and p / |p| there.
      * hit mask: a ray passing the centre at distance rho hits when the field falls below the threshold 1e-3
        somewhere on it, i.e. when rho < 0.3 + 1e-3 -+ e; the mask is compared with `rho < 0.3` outside the band
        |rho - 0.3| <= e + 1e-3 (the threshold belongs to the band: a ray up to 1e-3 outside a perfect ball is a hit);
      * depth: the tracer stops within 1e-3 + e of the sphere along the normal, 1 / cos(incidence) times that along the
        ray; hits steeper than 60 degrees are dropped (25.8 % of the ball's pixels for this camera: the share of the
        silhouette's area outside tan(asin(0.866 * 0.2)) / tan(asin(0.2)) of its radius), so the bound is 2 (1e-3 + e);
      * normals: within twice the measured angle of the analytic normal at the analytic hit point.
    Measured on MI355X: e = 1.17e-3, stencil-gradient angle 0.199 rad; 648 hits against 640 analytic, 16
    pixels in the band, none wrong outside it; 468 kept; depth error 2.05e-3 (bound 4.34e-3), normal error 0.176 rad
    (bound 0.398)."""
    from volsurfs_amd.background import intersect_bounding_primitive
    from volsurfs_amd.surf import get_field_gradients
    m, _ = sphere_surf
    assert m.render_sphere_traced is False and not m.is_training
    sdf = m.models["sdf"]
    g = torch.Generator("cuda").manual_seed(3)
    surf_pts = torch.nn.functional.normalize(torch.randn(20000, 3, device="cuda", generator=g), dim=1) * SPHERE_R
    with torch.no_grad():
        e = float(sdf.main_sdf(surf_pts)[0].abs().max())
        grad = get_field_gradients(sdf.main_sdf, surf_pts)
        cosang = (torch.nn.functional.normalize(grad, dim=1) * surf_pts / SPHERE_R).sum(1).clamp(-1, 1)
        ang = float(torch.acos(cosang).max())
    cam, o, d = _view_rays()
    raycast = intersect_bounding_primitive(m.bounding_primitive, o, d)
    renders, points, grads = m.render_fg_sphere_traced(raycast, 100, 1e-3)
    assert set(renders) == ST_KEYS
    N = o.shape[0]
    for k, c in (("rgb_fg", 3), ("depth_fg", 1), ("weights_sum", 1), ("bg_transmittance", 1), ("normals", 3)):
        assert renders[k].shape == (N, c), k
    hit = renders["weights_sum"][:, 0] > 0
    assert torch.equal(renders["weights_sum"] + renders["bg_transmittance"], torch.ones(N, 1, device="cuda"))
    assert set(renders["weights_sum"].unique().tolist()) == {0.0, 1.0}
    H = int(hit.sum())
    assert points.shape == (H, 3) and grads.shape == (N, 3)
    # analytic ball (float64)
    o64, d64 = o.double(), d.double()
    b = (o64 * d64).sum(1)
    rho = ((o64 * o64).sum(1) - b * b).clamp(min=0).sqrt()
    disc = b * b - ((o64 * o64).sum(1) - SPHERE_R ** 2)
    t0 = -b - disc.clamp(min=0).sqrt()
    p_gt = o64 + t0[:, None] * d64
    n_gt = p_gt / SPHERE_R
    band = (rho - SPHERE_R).abs() <= e + 1e-3
    want = rho < SPHERE_R
    wrong = (hit != want) & ~band
    cos_inc = -(d64 * n_gt).sum(1)
    keep = hit & want & (cos_inc >= MAX_INCIDENCE_COS)
    depth_err = float((renders["depth_fg"][:, 0].double() - t0)[keep].abs().max())
    dots = (renders["normals"].double() * n_gt).sum(1).clamp(-1, 1)
    normal_err = float(torch.acos(dots[keep]).max())
    print(f"surf sphere-traced: field error on the ball e = {e:.3e}, stencil-gradient angle {ang:.3e} rad; {H} hits "
          f"({int(want.sum())} analytic, {int(band.sum())} pixels in the band, {int(wrong.sum())} wrong outside it), "
          f"{int(keep.sum())} kept ({float(keep.sum()) / max(int(want.sum()), 1):.3f}), depth error {depth_err:.3e} "
          f"(bound {(1e-3 + e) / MAX_INCIDENCE_COS:.3e}), normal error {normal_err:.3e} rad (bound {2 * ang:.3e})")
    assert H > 0 and int(wrong.sum()) == 0
    assert int(keep.sum()) >= 0.7 * int(want.sum())
    assert depth_err <= (1e-3 + e) / MAX_INCIDENCE_COS
    assert normal_err <= 2 * ang
    assert bool((renders["rgb_fg"][~hit] == 0).all()) and bool((renders["depth_fg"][~hit] == 0).all())
    assert torch.equal(renders["normals"][hit], torch.nn.functional.normalize(grads[hit], dim=1))
    # render_rays: nothing new without the flag; "volumetric" untouched with it
    plain = m.render_rays(o, d)
    assert set(plain) == {"renders", "samples_3d", "samples_grad"} and set(plain["renders"]) == {"volumetric"}
    assert set(plain["renders"]["volumetric"]) == VOL_KEYS
    m.render_sphere_traced = True
    try:
        both = m.render_rays(o, d)
        m.is_training = True
        assert set(m.render_rays(o[:256].contiguous(), d[:256].contiguous(), iter_nr=400)["renders"]) == {"volumetric"}
    finally:
        m.render_sphere_traced = False
        m.is_training = False
    assert set(both["renders"]) == {"volumetric", "sphere_traced"}
    for k, v in plain["renders"]["volumetric"].items():
        assert torch.equal(v, both["renders"]["volumetric"][k]), k
    st = both["renders"]["sphere_traced"]
    assert set(st) == ST_KEYS | {"rgb", "rgb_bg", "depth_bg", "depth"}
    assert torch.equal(st["rgb_fg"], renders["rgb_fg"]) and torch.equal(st["depth_fg"], renders["depth_fg"])
    assert torch.equal(st["rgb"], st["rgb_fg"] + st["bg_transmittance"] * st["rgb_bg"])


@pytest.fixture(scope="module")
def offsets_method(sphere_surf):
    """OffsetsSurfs with K = 3 (one inner, one outer surface, delta about 0.02) after its offsets init."""
    from test_offsets_surfs_method import _method
    from test_surf_method import _cameras, _gt_images
    from volsurfs_amd.camera import TensorReel
    from volsurfs_amd.surf import get_logistic_beta_from_variance, logistic_distribution_stdev
    from volsurfs_amd.trainer import train
    _, folder = sphere_surf
    torch.manual_seed(1)
    iters = 1000
    mult = 0.02 / logistic_distribution_stdev(get_logistic_beta_from_variance(0.7))
    m = _method(folder, hp={"lr": 1e-3, "nr_inner_surfs": 1, "nr_outer_surfs": 1, "delta_surfs_multiplier": mult,
                            "init_phase_end_iter": iters, "color_init_phase_end_iter": iters + 200,
                            "first_phase_end_iter": iters + 1000})
    cams = _cameras(4)
    train(TensorReel(cams, _gt_images(cams)), m, 0, iters, nr_training_rays=256)
    m.is_training = False
    return m


@pytest.mark.gpu
def test_offsets_surfs_sphere_traced_render(offsets_method):
    from volsurfs_amd.background import intersect_bounding_primitive
    m = offsets_method
    K = m.nr_surfs
    assert K == 3 and m.main_surf_idx == 1 and m.render_sphere_traced is False
    cam, o, d = _view_rays()
    N = o.shape[0]
    raycast = intersect_bounding_primitive(m.bounding_primitive, o, d)
    renders, samples_3d, samples_sdf, samples_grad = m.render_fg_sphere_traced(raycast, 100, 1e-3)
    assert set(renders) == {"surfs_rgb", "surfs_alpha", "surfs_depths", "surfs_normals", "surfs_transmittance",
                            "surfs_blending_weights", "rgb_fg", "bg_transmittance"}
    for k, c in (("surfs_rgb", 3), ("surfs_alpha", 1), ("surfs_depths", 1), ("surfs_normals", 3),
                 ("surfs_transmittance", 1), ("surfs_blending_weights", 1)):
        assert renders[k].shape == (N, K, c), k
    assert renders["rgb_fg"].shape == (N, 3) and renders["bg_transmittance"].shape == (N, 1)
    hit = renders["surfs_depths"][:, :, 0] > 0
    counts = hit.sum(0).tolist()
    print("offsets sphere-traced: hits per surface, inner to outer:", counts)
    assert 0 < counts[0] < counts[1] < counts[2]
    assert samples_3d.shape == (sum(counts), 3) and samples_sdf.shape == (sum(counts), K, 1)
    assert samples_grad.shape == (sum(counts), 3)
    all3 = hit.all(1)
    assert int(all3.sum()) > 100
    dep = renders["surfs_depths"][all3][:, :, 0]
    assert bool((dep[:, 2] < dep[:, 1]).all()) and bool((dep[:, 1] < dep[:, 0]).all())
    # the samples are the hits surface after surface: each lies on its own surface within the threshold
    ends = np.cumsum([0] + counts)
    for k in range(K):
        assert float(samples_sdf[ends[k]:ends[k + 1], k, 0].abs().max()) < 1e-3
    # the blend, recomputed in torch from the returned per-surface tensors
    T, w, fg, bg = R.blend_restated(renders["surfs_rgb"], renders["surfs_alpha"])
    assert torch.equal(renders["surfs_transmittance"], T) and torch.equal(renders["surfs_blending_weights"], w)
    assert torch.equal(renders["rgb_fg"], fg) and torch.equal(renders["bg_transmittance"], bg)
    assert bool((renders["surfs_alpha"][~hit] == 0).all()) and bool((renders["surfs_alpha"][hit] > 0).all())
    # the batched trace gives what per-surface traces give
    from volsurfs_amd.sphere_trace import sphere_trace
    for k in range(K):
        pack, h = sphere_trace(m.models["sdfs"], o, d, m.bounding_primitive, 100, 1e-3, surf_idx=k)
        assert torch.equal(h, hit[:, k])
        assert torch.equal(pack.samples_z[h], renders["surfs_depths"][:, k][h])
    # render_rays
    plain = m.render_rays(o, d)
    assert set(plain["renders"]) == {"volumetric"}
    m.render_sphere_traced = True
    try:
        both = m.render_rays(o, d)
    finally:
        m.render_sphere_traced = False
    assert set(both["renders"]) == {"volumetric", "sphere_traced"}
    for k, v in plain["renders"]["volumetric"].items():
        assert torch.equal(v, both["renders"]["volumetric"][k]), k
    st = both["renders"]["sphere_traced"]
    assert torch.equal(st["rgb_fg"], renders["rgb_fg"])
    assert torch.equal(st["rgb"], st["rgb_fg"] + st["bg_transmittance"] * st["rgb_bg"])


@pytest.mark.gpu
def test_render_camera_sphere_traced_mode_and_render_and_eval(sphere_surf, offsets_method):
    from volsurfs_amd.evaluation import render_and_eval
    cam, _, _ = _view_rays(H=48)
    for m in (sphere_surf[0], offsets_method):
        vol = m.render_camera(cam)
        out = m.render_camera(cam, render_mode="sphere_traced")
        assert m.render_sphere_traced is False
        assert set(out) == set(m.RENDER_KEYS) == set(vol)
        assert out["rgb"].shape == (48, 48, 3) and bool(torch.isfinite(out["rgb"]).all())
        assert torch.equal(m.render_camera(cam)["rgb"], vol["rgb"])
        centre = out["bg_transmittance"][24, 24, 0]
        assert float(centre) < 1.0 and float(out["bg_transmittance"][0, 0, 0]) == 1.0
        with pytest.raises(ValueError):
            m.render_camera(cam, render_mode="nope")
        gt = out["rgb"].clone().unsqueeze(0)
        res = render_and_eval(m, {"test": ([cam], gt)}, save_pngs=False,
                              render_fn=lambda c: m.render_camera(c, render_mode="sphere_traced")["rgb"])
        assert res["test"]["psnr"] > 60.0 or math.isinf(res["test"]["psnr"])
