"""Texture fit (`volsurfs_amd.texture_fit`, csrc/texel_fit.hip): Adam on the 8-bit texel rows of a baked scene
(include/volsurfs_hip.h "Texture fit"), against the numpy restatement tests/texture_fit_restated.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import texture_fit_restated as TF
from texture_scene_cases import RENDER_KEYS, SH_RANGE
from texture_scene_cases import camera as _camera
from texture_scene_cases import random_planes as _random_planes
from texture_scene_cases import scene as _scene
from texture_scene_cases import smooth_planes as _smooth_planes
from texture_scene_cases import stack as _stack

RES = (32, 32, 16)
ALPHA_QUAD = (1, 3, 4, 6)           # VSA_NT_ALPHA_QUAD(d)

# test_recovery: loss_after / loss_before measured on the MI355X and the asserted bound, twice that
RECOVERY_RATIO_MEASURED = 0.137
RECOVERY_RATIO_BOUND = 2 * RECOVERY_RATIO_MEASURED
# test_recovery: at most this share of the student's owned degree-0 texels may go unseen.  Four cameras on a
# tetrahedron's corners leave no point of a sphere more than 70.5 degrees from the nearest view direction; from three
# units away the horizon of the largest shell (radius 0.7) lies at acos(0.7 / 3) = 76.5 degrees, so every point is in
# sight, and at 70.5 degrees a 32^2-atlas texel (side ~0.07 on the inner shell) still spans 0.07 * cos(70.5) * 125 / 3 =
# 1 pixel across and 3 along: the bilinear footprint of the hits (2 x 2 texels) reaches it.  What remains are
# texels owned through `reach` alone, beyond their chart's border on one side: a tenth is generous for those.
UNSEEN_CAP = 0.10


# ---------------------------------------------------------------------------------------------------------------------
# helpers

def _tetra_cameras(distance=3.0, focal=125.0):
    c = distance / 3 ** 0.5
    return [_camera(e, focal=focal) for e in ((c, c, c), (c, -c, -c), (-c, c, -c), (-c, -c, c))]


def _segments(bank):
    p = bank.plan
    return TF.segments(bank.K, bank.D, bank.tex_res, list(p.row_base), list(p.dom_off), bank.seg_start.cpu().numpy(),
                       bank.slot_of.cpu().numpy())


def _apron_is_tied(segs, texels):
    for seg in segs:
        for a in TF.apron_texels(seg.R):
            t = TF.clamp_target(*a, seg.R)
            own = texels[seg.row0 + seg.rows[t] * seg.quads * 4:][:seg.quads * 4]
            if not np.array_equal(texels[seg.row0 + seg.rows[a] * seg.quads * 4:][:seg.quads * 4], own):
                return False
    return True


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def _planes_equal(a, b):
    from volsurfs_amd.texture_export import export_planes
    pa, pb = export_planes(a.baked), export_planes(b.baked)
    return set(pa) == set(pb) and all(torch.equal(pa[k], pb[k]) for k in pa)


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU

def test_fold_sets_partition_the_apron():
    """Every apron texel folds into exactly one interior texel: 8 for the one texel of R = 1, 3 per corner and 1 per
    plain edge texel otherwise, none for the inside; each set in row-major order."""
    for R in (1, 2, 5):
        sets, apron = TF.fold_sets(R), TF.apron_texels(R)
        assert len(apron) == 4 * (R + 2) - 4 and apron == sorted(apron)
        assert sorted(a for v in sets.values() for a in v) == apron
        for (Y, X), v in sets.items():
            assert v == sorted(v) and all(TF.clamp_target(*a, R) == (Y, X) for a in v)
            on_y, on_x = Y in (1, R), X in (1, R)
            want = 8 if R == 1 else 3 if on_y and on_x else 1 if on_y or on_x else 0
            assert len(v) == want, (R, Y, X)
    assert TF.fold_sets(2)[(1, 2)] == [(0, 2), (0, 3), (1, 3)]
    assert TF.fold_sets(1)[(1, 1)] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)]


def test_every_byte_survives_its_master():
    """rintf(255 * (q / 255)) == q in fp32 for all 256 bytes: init followed by a step that does not move p keeps the
    byte."""
    q = np.arange(256, dtype=np.float32)
    p = q / np.float32(255.0)
    assert p.dtype == np.float32 and p[0] == 0 and p[255] == 1
    assert np.array_equal(np.rint(np.float32(255.0) * p), q)


def test_cabi_argument_errors_return_before_any_hip_call():
    """The "device" pointers are addresses of a host buffer nothing reads: every call must return before it touches
    the GPU.  The calls whose arguments are all good name a plan the stage does not support and get as far as that."""
    from volsurfs_amd import _lib
    from volsurfs_amd.neural_textures import Plan
    L = _lib.lib()
    ERR_ARG, ERR_UNSUPPORTED = -1, -2
    buf = (ctypes.c_char * 4096)()
    a16 = (ctypes.addressof(buf) + 15) & ~15
    plan = Plan()
    plan.nr_shells, plan.rgb_degrees, plan.alpha_degrees = 1, 2, 2
    plan.tex_res[0], plan.tex_res[1] = 8, 8
    last = len(plan.row_base) - 1
    ref = ctypes.byref(plan)
    nan, inf = float("nan"), float("inf")

    def init(plan=ref, slot_of=a16, seg=a16, texels=a16, p=a16, m=a16 + 16, v=a16 + 32):
        return L.vsa_texel_fit_init(plan, slot_of, seg, texels, p, m, v, None)

    def step(plan=ref, slot_of=a16, seg=a16, grad=a16, inv=1.0, p=a16, m=a16 + 16, v=a16 + 32, texels=a16, lr=0.01,
             b1=0.9, b2=0.99, eps=1e-15, nr=1, stats=a16):
        return L.vsa_texel_fit_step(plan, slot_of, seg, grad, inv, p, m, v, texels, lr, b1, b2, eps, nr, stats, None)

    assert L.vsa_texel_fit_state_bytes(None) == ERR_ARG
    plan.row_base[last] = 24
    assert L.vsa_texel_fit_state_bytes(ref) == 24 * 4 * 4
    plan.row_format = 1                                    # good arguments, an unsupported plan: past every check
    assert init() == step() == L.vsa_texel_fit_state_bytes(ref) == ERR_UNSUPPORTED
    assert step(lr=0.0, eps=0.0, b1=0.0, b2=0.0, nr=1 << 30) == ERR_UNSUPPORTED
    for kw in ({"plan": None}, {"slot_of": None}, {"seg": None}, {"texels": None}, {"p": None}, {"m": None}, {"v": None},
               {"texels": a16 + 4}, {"p": a16 + 4}, {"m": a16 + 8}, {"v": a16 + 12}):
        assert init(**kw) == ERR_ARG, kw
        assert step(**kw) == ERR_ARG, kw
    for kw in ({"grad": None}, {"stats": None}, {"grad": a16 + 8}, {"stats": a16 + 4}, {"nr": 0}, {"nr": -1},
               {"lr": -1e-3}, {"lr": nan}, {"lr": inf}, {"eps": -1e-15}, {"eps": nan}, {"eps": inf}, {"inv": nan},
               {"inv": inf}, {"inv": -1.0}, {"b1": 1.0}, {"b1": -0.1}, {"b1": nan}, {"b2": 1.0}, {"b2": -0.1},
               {"b2": nan}):
        assert step(**kw) == ERR_ARG, kw
    plan.nr_shells = 0
    assert init() == step() == ERR_ARG
    plan.nr_shells, plan.tex_res[1] = 1, 0
    assert init() == step() == ERR_ARG
    plan.tex_res[1], plan.row_format, plan.alpha_degrees = 8, 0, 1
    assert init() == step() == ERR_UNSUPPORTED
    plan.alpha_degrees, plan.row_base[last] = 2, 1 << 29        # vsa_nt_shade_bwd's 32-bit offsets end here
    assert init() == step() == L.vsa_texel_fit_state_bytes(ref) == ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
# GPU

def _synthetic_gradients(rng, segs, n):
    """f16 gradient rows: 60 % of the quads idle, the rest ~N(0, 40) with a few +-inf and NaN elements; the own quad of
    texel (1, 1) of every segment idle and the same quad of its apron texel (0, 0) live."""
    g = (rng.standard_normal(n) * 40).astype(np.float16).reshape(-1, 4)
    g[rng.random(g.shape[0]) < 0.6] = 0
    g = g.reshape(-1)
    for bad in (np.inf, -np.inf, np.nan):
        g[rng.integers(0, n, 6)] = bad
    via_apron = []
    for seg in segs:
        own = seg.row0 + seg.rows[1, 1] * seg.quads * 4
        apron = seg.row0 + seg.rows[0, 0] * seg.quads * 4
        g[own:own + 4] = 0
        g[apron:apron + 4] = np.float16([3.0, -2.0, 0.0, 1.0])
        via_apron.append(own)
    return g, via_apron


@pytest.mark.gpu
@pytest.mark.parametrize("tex_res", [(5, 2, 1, 1), (8, 4, 4, 2)], ids=lambda r: "x".join(map(str, r)))
def test_init_and_three_steps_equal_the_restatement(tex_res):
    """p, m, v, the bytes, the consumed gradients and the counters, bit for bit: init on random bytes (the apron
    included), then three steps from random state with fresh synthetic gradients each."""
    from volsurfs_amd import _lib
    from volsurfs_amd.texture_export import _empty_baked_bank
    bank = _empty_baked_bank(2, 4, list(tex_res), list(SH_RANGE), False, False, True, True, "cuda")
    segs, ref = _segments(bank), ctypes.byref(bank.plan)
    n = bank.texels.numel()
    assert _lib.workspace_bytes("vsa_texel_fit_state_bytes", ref) == 4 * n
    rng = np.random.default_rng(sum(tex_res))
    texels = rng.integers(0, 256, n).astype(np.uint8)
    junk = rng.random(n).astype(np.float32)                  # init writes interior state only: the rest keeps this
    bank.texels.copy_(torch.from_numpy(texels))
    p, m, v = (torch.from_numpy(junk).cuda() for _ in range(3))
    _lib.call("vsa_texel_fit_init", ref, bank.slot_of, bank.seg_start, bank.texels, p, m, v, _lib.stream_ptr())
    wp, wm, wv, wt = TF.init(segs, texels)
    interior = np.zeros(n, bool)
    for seg in segs:
        for row in seg.rows[1:-1, 1:-1].ravel():
            interior[seg.row0 + row * seg.quads * 4:][:seg.quads * 4] = True
    assert not _apron_is_tied(segs, texels) and _apron_is_tied(segs, wt)
    assert np.array_equal(bank.texels.cpu().numpy(), wt)
    for got, want in ((p, wp), (m, wm), (v, wv)):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(np.where(interior, want, junk)))

    # random state on the interior
    p_h = np.where(interior, rng.random(n), 0).astype(np.float32)
    m_h = np.where(interior, rng.standard_normal(n) * 0.05, 0).astype(np.float32)
    v_h = np.where(interior, rng.random(n) * 0.01, 0).astype(np.float32)
    t_h = wt
    p, m, v = (torch.from_numpy(a).cuda() for a in (p_h, m_h, v_h))
    grad = torch.zeros(n, dtype=torch.float16, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    inv, lr, b1, b2, eps = 1.0 / 64, 0.3, 0.9, 0.99, 1e-15
    seen = np.zeros(4, np.int64)
    for nr in (1, 2, 3):
        g_h, via_apron = _synthetic_gradients(rng, segs, n)
        grad.copy_(torch.from_numpy(g_h))
        _lib.call("vsa_texel_fit_step", ref, bank.slot_of, bank.seg_start, grad, inv, p, m, v, bank.texels, lr, b1, b2,
                  eps, nr, stats, _lib.stream_ptr())
        p_w, m_w, v_w, t_w, g_w, s_w = TF.step(segs, g_h, inv, p_h, m_h, v_h, t_h, lr, b1, b2, eps, nr)
        for own in via_apron:                                # idle on its own row, live through its apron
            assert not np.array_equal(_bits(m_w[own:own + 4]), _bits(m_h[own:own + 4]))
        for name, got, want in (("p", p, p_w), ("m", m, m_w), ("v", v, v_w), ("texels", bank.texels, t_w)):
            diff = int((_bits(got.cpu().numpy()) != _bits(want)).sum())
            assert diff == 0, (nr, name, diff)
        assert np.array_equal(_bits(grad.cpu().numpy()), g_w), nr
        assert stats.cpu().tolist() == s_w, (nr, stats.cpu().tolist(), s_w)
        assert _apron_is_tied(segs, t_w)
        seen += np.asarray(s_w)
        p_h, m_h, v_h, t_h = p_w, m_w, v_w, t_w
    assert (seen > 0).all()                                  # updates, non-finite elements, changed bytes and clamps
    assert (p_h[interior] == 0).any() and (p_h[interior] == 1).any()


@functools.lru_cache(maxsize=None)
def _baked_method():
    from volsurfs_amd.methods import VolSurfs
    method = VolSurfs(list(_stack(1)), max_rays=1024, textures_res=(8, 8, 4, 4))
    with torch.no_grad():            # (tables at their initial 1e-4 give every texel the byte of sigmoid(0))
        method.bank.tables.uniform_(-1.0, 1.0, generator=torch.Generator(device="cuda").manual_seed(3))
    method.bake()
    return method


@pytest.mark.gpu
def test_init_ties_the_apron_of_a_baked_bank_and_steps_keep_it():
    """A bank out of bake() holds the network's values in the apron; after init they equal the clamped interior, after
    every step still.  TextureFit never mutates its source.  lr = 0: no byte changes while m and v do."""
    from volsurfs_amd import _lib
    from volsurfs_amd.texture_fit import TextureFit
    method = _baked_method()
    bank = method.baked
    segs = _segments(bank)
    before = bank.texels.clone()
    assert not _apron_is_tied(segs, before.cpu().numpy())
    rng = np.random.default_rng(5)
    for lr in (0.05, 0.0):
        fit = TextureFit(method, lr=lr)
        assert torch.equal(bank.texels, before) and fit.scene.baked is not bank
        fbank = fit.scene.baked
        fsegs = _segments(fbank)
        t0 = fbank.texels.cpu().numpy()
        assert _apron_is_tied(fsegs, t0)
        for _ in range(3):
            g = (rng.standard_normal(fit.grad_rows.numel()) * 8).astype(np.float16)
            fit.grad_rows.copy_(torch.from_numpy(g))
            fit._scale = 1.0
            stats = fit.step().cpu().tolist()
            assert stats[0] > 0 and not bool(fit.grad_rows.any())
            assert _apron_is_tied(fsegs, fbank.texels.cpu().numpy())
            assert (stats[2] == 0) == (lr == 0.0)
        assert np.array_equal(fbank.texels.cpu().numpy(), t0) == (lr == 0.0)
        assert bool(fit.m.any()) and bool(fit.v.any())
    # init on the baked bank's own rows: the apron of a write_scene -> load_scene round trip
    own = bank.texels.clone()
    p, m, v = (torch.zeros(own.numel(), device="cuda") for _ in range(3))
    _lib.call("vsa_texel_fit_init", ctypes.byref(bank.plan), bank.slot_of, bank.seg_start, own, p, m, v,
              _lib.stream_ptr())
    assert _apron_is_tied(segs, own.cpu().numpy())
    assert np.array_equal(own.cpu().numpy(), TF.init(segs, before.cpu().numpy())[3])


@pytest.mark.gpu
@pytest.mark.parametrize("lr", [1e-3, 3e-2])
def test_fitting_a_scene_to_its_own_render_changes_nothing(lr):
    """The targets are the float "rgb" of the scene's own render_baked_camera: the fused L1's sign(0) is 0 and the
    forward is bit-identical, so no gradient is non-zero, no quad is live, no byte and no state changes."""
    from volsurfs_amd.texture_fit import TextureFit, fit_textures
    scene = _scene(_stack(2), _random_planes(3, RES, 21))
    cams = [_camera((0.3, 0.4, -1.9)), _camera((1.4, -0.9, 0.8))]
    targets = torch.stack([scene.render_baked_camera(c)["rgb"] for c in cams])
    fitted, report = fit_textures(scene, cams, targets=targets, iterations=4, views_per_step=2, lr=lr)
    assert report.loss_before == 0 and report.loss_after == 0 and report.losses == [0.0] * 4 and report.steps == 4
    assert (report.quads_updated, report.bytes_changed, report.nonfinite, report.clamped) == (0, 0, 0, 0)
    assert set(report.texels_touched.values()) == {0}
    assert fitted is not scene and _planes_equal(fitted, scene)
    fit = TextureFit(scene, lr=lr)
    from volsurfs_amd.camera import get_camera_rays
    rays_o, rays_d, _ = get_camera_rays(cams[0])
    fit.accumulate(rays_o, rays_d, targets[0])
    assert float(fit.loss) == 0 and not bool(fit.grad_rows.any())
    fit.step()
    assert not bool(fit.m.any()) and not bool(fit.v.any())


def _element_kinds(bank, segs):
    """bool [elements]: True where an element of an INTERIOR row is padding or belongs to an alpha model the shell
    does not have."""
    frozen = np.zeros(bank.texels.numel(), bool)
    for seg in segs:
        n = 2 * seg.degree + 1
        has_alpha = bank.tex_channels(bank.tex_index(seg.shell, 1, seg.degree)) > 0
        col = np.arange(seg.quads * 4)
        live = col < 3 * n
        if has_alpha:
            live |= (col >= 4 * ALPHA_QUAD[seg.degree]) & (col < 4 * ALPHA_QUAD[seg.degree] + n)
        for row in seg.rows[1:-1, 1:-1].ravel():
            frozen[seg.row0 + row * seg.quads * 4:][:seg.quads * 4] = ~live
    return frozen


@pytest.mark.gpu
@pytest.mark.parametrize("shared_alpha", [False, True], ids=["inner_solid", "inner_solid-shared_alpha"])
def test_elements_without_a_model_and_padding_never_move(shared_alpha):
    """A solid inner shell has no alpha model; with a shared alpha model as well, no shell has one.  Those elements
    and the rows' padding receive no gradient: their bytes, p, m and v stay what init made them."""
    from volsurfs_amd.camera import get_camera_rays
    from volsurfs_amd.texture_fit import TextureFit
    meshes = _stack(1)
    teacher = _scene(meshes, _random_planes(3, RES, 31, solid=True, no_alpha=shared_alpha), solid=True,
                     shared_alpha=shared_alpha)
    student = _scene(meshes, _random_planes(3, RES, 32, solid=True, no_alpha=shared_alpha), solid=True,
                     shared_alpha=shared_alpha)
    fit = TextureFit(student, lr=0.02)
    bank = fit.scene.baked
    frozen = torch.from_numpy(_element_kinds(bank, _segments(bank))).cuda()
    assert bool(frozen.any()) and not bool(frozen.all())
    t0, p0 = bank.texels.clone(), fit.p.clone()
    for cam in _tetra_cameras()[:3]:
        rays_o, rays_d, _ = get_camera_rays(cam)
        fit.accumulate(rays_o, rays_d, teacher.render_baked_camera(cam)["rgb"])
        assert fit.step().cpu().tolist()[0] > 0
    assert not torch.equal(bank.texels, t0)
    assert torch.equal(bank.texels[frozen], t0[frozen]) and torch.equal(fit.p[frozen], p0[frozen])
    assert not bool(fit.m[frozen].any()) and not bool(fit.v[frozen].any())
    assert bool(fit.v[~frozen].any())


@pytest.mark.gpu
def test_a_fitted_scene_survives_write_and_load(tmp_path):
    """What the apron tie is for: write_scene -> load_scene of a fitted scene renders every buffer with the same
    bytes."""
    from volsurfs_amd.texture_export import load_scene, write_scene
    from volsurfs_amd.texture_fit import fit_textures
    meshes = _stack(1)
    teacher = _scene(meshes, _random_planes(3, RES, 41, solid=True), solid=True)
    student = _scene(meshes, _random_planes(3, RES, 42, solid=True), solid=True)
    cams = _tetra_cameras()
    fitted, report = fit_textures(student, cams, teacher=teacher, iterations=6, lr=0.02)
    assert report.bytes_changed > 0 and not _planes_equal(fitted, student)
    write_scene(fitted, str(tmp_path / "fit"))
    back = load_scene(str(tmp_path / "fit"), bvh_builder="device")
    assert _planes_equal(fitted, back)
    assert torch.equal(fitted.baked.texels, back.baked.texels)
    for cam in (_camera((0.3, 0.4, -1.9)), _camera((0.0, 0.0, 0.55)), cams[1]):
        a, b = fitted.render_baked_camera(cam), back.render_baked_camera(cam)
        for k in RENDER_KEYS:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_recovery_of_an_offset_student():
    """The teacher has smooth random planes; the student the same meshes and UVs with every degree-0 colour byte 40
    higher.  40 steps at lr = 1e-2 (a hundredth of the byte range per step: the offset is within reach) over 4
    cameras: the loss over the training views falls below RECOVERY_RATIO_BOUND of what it
    was.  Measured on the MI355X: see RECOVERY_RATIO_MEASURED."""
    from volsurfs_amd.texture_fit import fit_textures
    from volsurfs_amd.texture_transfer import texel_owners
    meshes = _stack(2)
    planes = _smooth_planes(3, RES, 51)
    teacher = _scene(meshes, planes)
    moved = {k: v.clone() for k, v in planes.items()}
    for s in range(3):
        moved[(s, 0)][..., :3] += 40
    student = _scene(meshes, moved)
    fitted, report = fit_textures(student, _tetra_cameras(), teacher=teacher, iterations=40, lr=1e-2, seed=1)
    owned = [int((texel_owners(m, RES[0])[0] >= 0).sum()) for m in meshes]
    unseen = [1 - report.texels_touched[(s, 0)] / owned[s] for s in range(3)]
    ratio = report.loss_after / report.loss_before
    print(f"loss {report.loss_before:.5f} -> {report.loss_after:.5f}, ratio {ratio:.4f} (bound {RECOVERY_RATIO_BOUND}); "
          f"unseen share of owned degree-0 texels per shell {[round(u, 4) for u in unseen]} (cap {UNSEEN_CAP}); "
          f"bytes changed {report.bytes_changed}, clamped {report.clamped}, non-finite {report.nonfinite}")
    assert RECOVERY_RATIO_BOUND < 1
    assert report.nonfinite == 0 and report.steps == 40
    assert max(unseen) < UNSEEN_CAP
    assert report.loss_after < report.loss_before
    assert ratio < RECOVERY_RATIO_BOUND


@pytest.mark.gpu
def test_make_lod_with_refit():
    """make_lod(refit=...) reports "refit" and lowers the training-view loss; refit=None gives the bytes of
    transfer_scene on the same meshes, the path before the argument existed."""
    from volsurfs_amd.texture_fit import FitReport
    from volsurfs_amd.texture_transfer import make_lod, transfer_scene
    src = _scene(_stack(2), _random_planes(3, RES, 13))
    plain, report = make_lod(src, 0.5, padding=2)
    assert "refit" not in report
    assert _planes_equal(plain, transfer_scene(src, plain.tensor_meshes, list(RES)))
    again, report0 = make_lod(src, 0.5, padding=2, refit=None)
    assert "refit" not in report0 and _planes_equal(plain, again)
    fitted, report = make_lod(src, 0.5, padding=2, refit={"nr_cameras": 4, "resolution": (64, 64), "iterations": 12})
    assert set(report) == {"simplify", "atlas", "transfer", "faces", "refit"} and isinstance(report["refit"], FitReport)
    r = report["refit"]
    print(f"make_lod refit: loss {r.loss_before:.5f} -> {r.loss_after:.5f}, bytes changed {r.bytes_changed}")
    assert r.steps == 12 and r.nonfinite == 0 and r.bytes_changed > 0
    assert r.loss_after < r.loss_before
    assert all(torch.equal(a.faces_uvs, b.faces_uvs) for a, b in zip(plain.tensor_meshes, fitted.tensor_meshes))
    assert not _planes_equal(plain, fitted)
    out = fitted.render_baked_camera(_camera((0.2, 0.5, -2.0)))
    assert bool(torch.isfinite(out["rgb"]).all())
