"""Texture transfer (`volsurfs_amd.texture_transfer`, csrc/texture_transfer.hip): baked textures carried from one stack of
shells onto another with other faces and other UVs (include/volsurfs_hip.h "Texture transfer"), against the
numpy restatement tests/texture_transfer_restated.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_distance_restated as MD
import texture_transfer_restated as TT
from texture_scene_cases import RENDER_KEYS, SH_RANGE
from texture_scene_cases import camera as _camera
from texture_scene_cases import constant_byte as _constant_byte
from texture_scene_cases import constant_planes as _constant_planes
from texture_scene_cases import random_planes as _random_planes
from texture_scene_cases import scene as _scene
from texture_scene_cases import stack as _stack

SRC_RES = (32, 32, 16)              # one degree coarser than the others: the per-degree grids differ
DST_RES_UP = (40, 24, 24)           # above / equal-ish / above the source's, not multiples of the 8 x 8 tile
DST_RES_DOWN = (16, 16, 8)


# ---------------------------------------------------------------------------------------------------------------------
# helpers

def _restated(scene, dst_meshes, res, samples, reach, max_distance):
    """The restatement's planes and reports for every (shell, degree) of a transfer."""
    from volsurfs_amd.texture_export import export_planes
    bank, tr = scene.baked, scene.raytracer
    src_planes = export_planes(bank)
    tris = tr.tris.cpu().numpy()
    fuv = scene.face_uvs.cpu().numpy()
    planes, reports = {}, {}
    for s, m in enumerate(dst_meshes):
        off, n = tr.mesh_tri_offset[s], tr.mesh_nr_tris[s]
        has_alpha = not (bool(bank.plan.inner_solid) and s == 0)
        V, F, UV = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.faces_uvs.cpu().numpy()
        for d in range(bank.D):
            planes[(s, d)], reports[(s, d)] = TT.transfer_shell_degree(
                tris[off:off + n], fuv[off:off + n], src_planes[(s, d)].cpu().numpy(), float(bank.plan.sh_lo[d]),
                float(bank.plan.sh_span[d]), bank.anchor, has_alpha, V, F, UV, res[d], samples, reach, max_distance)
    return planes, reports


def _assert_same_render(a, b, keys=RENDER_KEYS):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU

def test_restated_projection_is_the_mesh_distance_chain():
    """`project` writes closest_on_triangle out once more (it needs the region): the same (d2, u, v) as the
    mesh-distance restatement wherever the region is not the interior, and d2 = 0 there."""
    rng = np.random.default_rng(0)
    rec = np.zeros((40, 12), np.float32)
    rec[:, [0, 1, 4, 5, 8, 9]] = rng.uniform(-4, 4, (40, 6)).astype(np.float32)
    rec[0, 4:10] = 0                                   # a point
    rec[1, 8:10] = rec[1, 4:6]                         # a sliver
    q = rng.uniform(-5, 5, (200, 2)).astype(np.float32)
    dd, u, v = TT.project(q[:, 0], q[:, 1], rec)
    p3 = np.concatenate([q, np.zeros((200, 1), np.float32)], 1)
    d0, u0, v0 = MD.closest_on_triangles(p3, rec)
    assert np.array_equal(u, u0) and np.array_equal(v, v0)
    inside = dd != d0
    assert inside.any() and (dd[inside] == 0).all() and (u[inside] > 0).all() and (v[inside] > 0).all()
    assert ((u + v)[inside] < 1.0 + 1e-6).all()


def test_restated_owners_of_one_right_triangle():
    """uv triangle (0, 0), (1, 0), (0, 1) in a 4 x 4 atlas = texel-unit triangle (0, 0), (4, 0), (0, 4): the owners and
    the distances written out by hand."""
    uv = np.array([[[0, 0], [1, 0], [0, 1]]], np.float32)
    own = TT.texel_owners(uv, 4, reach=1.5)
    # centres (c + 0.5, r + 0.5): inside iff c + r + 1 < 4; on the hypotenuse x + y = 4 iff c + r = 3 (an edge region
    # with zero distance); beyond it the distance to the line is (c + r + 1 - 4) / sqrt(2)
    for r in range(4):
        for c in range(4):
            over = c + r + 1 - 4
            want = 0.0 if over <= 0 else over * over / 2.0
            if want <= 1.5 * 1.5:
                assert own["face"][r, c] == 0, (r, c)
                assert abs(float(own["d2"][r, c]) - want) < 1e-6, (r, c, own["d2"][r, c], want)
            else:
                assert own["face"][r, c] == -1 and np.isinf(own["d2"][r, c]), (r, c)
    assert own["d2"][3, 3] == np.inf and own["face"][3, 2] == 0            # 4.5 > 2.25 >= 2.0
    assert np.array_equal(own["d2"] == 0, np.add.outer(np.arange(4), np.arange(4)) <= 3)
    # the rasterizer's rule covers the centres strictly inside: the hypotenuse runs down and to the left (not a top-left
    # edge), so the centres on it are covered by nobody and are owned through the projection alone, at distance 0
    r, c = np.divmod(np.arange(16), 4)
    assert np.array_equal(TT.raster_covers(uv, 4, c, r)[:, 0].reshape(4, 4), np.add.outer(np.arange(4), np.arange(4)) <= 2)
    assert (own["key"][np.add.outer(np.arange(4), np.arange(4)) <= 2] == 0).all()
    assert (own["key"][0, 3], own["key"][3, 0]) == (TT.OUTSIDE, TT.OUTSIDE)
    # a face whose raster covers the texel goes first, whatever its id.  8 x 8 atlas: face 0 is the zero-area segment
    # (3, 0) - (4, 1), which passes through the centre (3.5, 0.5) of texel (0, 3): its projection gives exactly 0 and
    # its raster covers nothing; face 1 is the triangle (0, 0), (5, 0), (0, 5), which covers that texel
    both = np.array([[[0.375, 0], [0.5, 0.125], [0.375, 0]], [[0, 0], [0.625, 0], [0, 0.625]]], np.float32)
    got = TT.texel_owners(both, 8)
    assert got["face"][0, 3] == 1 and got["d2"][0, 3] == 0 and got["key"][0, 3] == 1
    assert TT.texel_owners(both[:1], 8)["key"][0, 3] == TT.OUTSIDE                # alone, the segment owns it at d2 = 0
    # the owned barycentrics of a covered centre reproduce it: (x, y) = 4 (u, v)
    assert np.allclose(own["bary"][1, 0] * 4, (0.5, 1.5), atol=1e-6)
    # reach 0: exactly the covered texels
    own0 = TT.texel_owners(uv, 4, reach=0.0)
    assert np.array_equal(own0["face"] >= 0, own["d2"] == 0)
    # two faces over the same texels: the lower id owns; a NaN uv is a candidate of nothing
    two = np.concatenate([uv, uv, uv], 0)
    two[0, 0, 0] = np.nan
    assert set(np.unique(TT.texel_owners(two, 4)["face"])) == {-1, 1}


def test_restated_nearest_byte_rule():
    for d in range(4):
        lut = TT.expand_lut(-SH_RANGE[d], 2 * SH_RANGE[d])
        assert lut.dtype == np.float32 and (np.diff(lut) >= 0).all()
        got = TT.nearest_byte(lut, lut)
        for q in range(256):
            assert got[q] == np.nonzero(lut == lut[q])[0][0], (d, q)
    # a table with equal entries (fp16 is scale-free: no sh_range makes one): the lowest byte of each run
    flat = np.repeat(TT.expand_lut(-15.0, 30.0)[::2], 2)
    assert flat.shape == (256,) and (np.diff(flat) == 0).sum() == 128
    got = TT.nearest_byte(flat, flat)
    assert all(got[q] == np.nonzero(flat == flat[q])[0][0] for q in range(256))
    # midway between two entries: the lower
    lut = TT.expand_lut(-15.0, 30.0)
    mid = (lut[100] + lut[101]) * np.float32(0.5)
    assert mid - lut[100] == lut[101] - mid and TT.nearest_byte(lut, np.array([mid]))[0] == 100


def test_restated_sums_have_the_rule_shape():
    x = np.arange(64, dtype=np.float64) * 0.1
    assert abs(TT.wave_sum(x) - x.sum()) < 1e-9
    p = np.arange(3000, dtype=np.float64) * 0.3
    assert abs(TT.ordered_sum(p) - p.sum()) < 1e-6


def test_cabi_argument_errors_return_before_any_hip_call():
    from volsurfs_amd import _lib
    from volsurfs_amd.neural_textures import Plan
    L = _lib.lib()
    ERR_ARG, ERR_UNSUPPORTED = -1, -2
    assert L.vsa_textransfer_workspace_bytes(0, 16) == ERR_ARG
    assert L.vsa_textransfer_workspace_bytes(17, 16) == ERR_ARG
    assert L.vsa_textransfer_workspace_bytes(1, 0) == ERR_ARG
    assert L.vsa_textransfer_workspace_bytes(1, 16385) == ERR_ARG
    assert L.vsa_textransfer_workspace_bytes(2, 20) == 2 * 20 * 20 * 8 + 2 * 9 * 8
    buf = (ctypes.c_char * 4096)()
    a16 = (ctypes.addressof(buf) + 15) & ~15                    # a 16-byte aligned host address: never dereferenced
    base1 = (ctypes.c_longlong * 2)(0, 4)
    need = L.vsa_textransfer_workspace_bytes(1, 8)
    own = L.vsa_textransfer_owners
    assert own(None, a16, base1, 1, 8, 1.5, a16, need, None) == ERR_ARG             # NULL
    assert own(a16, None, base1, 1, 8, 1.5, a16, need, None) == ERR_ARG
    assert own(a16, a16, None, 1, 8, 1.5, a16, need, None) == ERR_ARG
    assert own(a16, a16, base1, 1, 8, 1.5, None, need, None) == ERR_ARG
    assert own(a16, a16, base1, 1, 8, 1.5, a16 + 4, need, None) == ERR_ARG          # misaligned workspace
    assert own(a16, a16 + 4, base1, 1, 8, 1.5, a16, need, None) == ERR_ARG          # misaligned records
    assert own(a16, a16, base1, 1, 8, 1.5, a16, need - 1, None) == ERR_ARG          # short workspace
    assert own(a16, a16, base1, 0, 8, 1.5, a16, need, None) == ERR_ARG              # counts out of range
    assert own(a16, a16, base1, 17, 8, 1.5, a16, need, None) == ERR_ARG
    assert own(a16, a16, base1, 1, 0, 1.5, a16, need, None) == ERR_ARG
    assert own(a16, a16, (ctypes.c_longlong * 2)(0, 0), 1, 8, 1.5, a16, need, None) == ERR_ARG      # a shell without faces
    assert own(a16, a16, (ctypes.c_longlong * 2)(0, 1 << 31), 1, 8, 1.5, a16, need, None) == ERR_UNSUPPORTED
    assert own(a16, a16, base1, 1, 8, -0.5, a16, need, None) == ERR_ARG             # reach
    assert own(a16, a16, base1, 1, 8, float("nan"), a16, need, None) == ERR_ARG
    fields = L.vsa_textransfer_owner_fields
    assert fields(None, need, a16, base1, 1, 0, 8, a16, a16, a16, None) == ERR_ARG
    assert fields(a16, need, a16, base1, 1, 1, 8, a16, a16, a16, None) == ERR_ARG   # shell out of range
    assert fields(a16, need - 1, a16, base1, 1, 0, 8, a16, a16, a16, None) == ERR_ARG
    plan = Plan()
    plan.nr_shells, plan.rgb_degrees, plan.alpha_degrees = 1, 2, 2
    plan.tex_res[0], plan.tex_res[1] = 8, 8
    res = (ctypes.c_int32 * 4)(8, 8, 8, 8)
    roots, frames = (ctypes.c_int32 * 1)(0), (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    nbytes = 4 * 8 * 8 * 4

    def planes(plan=ctypes.byref(plan), degree=0, src=a16, src_bytes=nbytes, nr=1, depth=10, samples=1, maxd=1.0,
               ws=a16, ws_bytes=need, dst=a16, dst_bytes=nbytes, stats=a16):
        return L.vsa_textransfer_planes(plan, degree, src, src_bytes, a16, a16, roots, frames, nr, depth, a16, a16, a16,
                                        base1, res, samples, maxd, ws, ws_bytes, dst, dst_bytes, stats, None)
    assert planes(plan=None) == ERR_ARG
    assert planes(src=None) == ERR_ARG and planes(dst=None) == ERR_ARG and planes(stats=None) == ERR_ARG
    assert planes(src=a16 + 4) == ERR_ARG and planes(dst=a16 + 8) == ERR_ARG and planes(ws=a16 + 8) == ERR_ARG
    assert planes(ws_bytes=need - 1) == ERR_ARG
    assert planes(samples=0) == ERR_ARG and planes(samples=5) == ERR_ARG
    assert planes(degree=2) == ERR_ARG and planes(degree=-1) == ERR_ARG
    assert planes(nr=2) == ERR_ARG and planes(depth=48) == ERR_ARG
    assert planes(src_bytes=nbytes - 4) == ERR_ARG and planes(dst_bytes=nbytes + 4) == ERR_ARG
    assert planes(maxd=float("nan")) == ERR_ARG
    plan.alpha_degrees = 1
    assert planes() == ERR_UNSUPPORTED
    plan.alpha_degrees, plan.row_format = 2, 1
    assert planes() == ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
# GPU

@pytest.mark.gpu
def test_texel_centres_read_exactly_that_pixel():
    """1.  A hit whose uv is the stated centre of pixel (r, c) shades with the LUT values of that pixel's bytes."""
    from volsurfs_amd.texture_export import export_planes
    meshes = _stack(2)
    scene = _scene(meshes, _random_planes(3, SRC_RES, 1, solid=True), solid=True)
    bank, tr = scene.baked, scene.raytracer
    planes = export_planes(bank)
    for d, R in enumerate(SRC_RES):
        pix = [(0, 0), (0, R - 1), (R - 1, 0), (R - 1, R - 1), (3, 5), (R // 2, 1), (R - 2, R // 3)]
        uv = torch.tensor([[float(x) for x in TT.texel_centre_uv(r, c, R)] for r, c in pix]).cuda()
        N = len(pix)
        hit_slot = torch.tensor([[tr.mesh_tri_offset[s]] * N for s in range(3)], dtype=torch.int32).cuda()
        tex_uv = uv[None].expand(3, N, 2).contiguous()
        rays_d = torch.tensor([[0.0, 0.0, 1.0]] * N).cuda()
        coeffs = bank.shade(hit_slot, tex_uv, rays_d, tr.tris, want_coeffs=True)[3].cpu().numpy()
        lut = TT.expand_lut(-SH_RANGE[d], 2 * SH_RANGE[d])
        for s in range(3):
            img = planes[(s, d)].cpu().numpy()
            for n, (r, c) in enumerate(pix):
                for i in range(2 * d + 1):
                    for ch in range(4 if s > 0 else 3):             # (shell 0 is solid: no alpha coefficients)
                        assert coeffs[s, n, ch * 16 + d * d + i] == lut[img[i, r, c, ch]], (s, d, r, c, i, ch)


def _hand_mesh():
    """Five faces: a zero-area uv triangle, UVs that leave [0, 1], two overlapping uv triangles, a NaN uv."""
    from volsurfs_amd.mesh import TensorMesh
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1]], np.float32)
    F = np.array([[0, 1, 2], [1, 3, 2], [0, 1, 4], [1, 5, 4], [2, 3, 4]], np.int32)
    nan = float("nan")
    UV = np.array([[[0.2, 0.2], [0.5, 0.5], [0.8, 0.8]],            # zero area
                   [[-0.3, 0.1], [0.4, -0.2], [0.3, 0.45]],         # leaves [0, 1]
                   [[0.5, 0.1], [0.95, 0.1], [0.5, 0.7]],           # overlaps the next
                   [[0.55, 0.15], [1.3, 0.2], [0.6, 0.9]],
                   [[0.1, 0.6], [nan, 0.9], [0.1, 0.9]]], np.float32)
    return TensorMesh(V, F, UV)


def _assert_owners_equal(mesh, R, reach):
    from volsurfs_amd.texture_transfer import texel_owners
    face, bary, d2 = texel_owners(mesh, R, reach)
    recs = TT.face_records(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy())
    want = TT.texel_owners(mesh.faces_uvs.cpu().numpy(), R, reach, recs)
    assert np.array_equal(face.cpu().numpy(), want["face"])
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), want["d2"].view(np.uint32))
    assert np.array_equal(bary.cpu().numpy().view(np.uint32), want["bary"].view(np.uint32))
    return face, d2


@pytest.mark.gpu
def test_owner_is_the_rasterizers_face_where_it_covers():
    """2, the rasterizer clause: where `rasterize_atlas`' face_id >= 0 the owner is that face with d2 = 0.

    "Inside a face" is the rasterizer's own coverage rule (corners snapped to 1/256 texel, top-left edges): the
    projection onto the exact triangle alone disagreed with it on 3 of 613 texels at R = 40, each with the
    rasterizer's face less than 1.1e-3 texels from the centre.  The restated coverage rule is checked
    against `rasterize_atlas` on the way.  Each figure is printed before the assertion."""
    from volsurfs_amd.atlas import rasterize_atlas
    from volsurfs_amd.texture_transfer import texel_owners
    mesh = _stack(2)[1]
    uv = mesh.faces_uvs.cpu().numpy()
    total = 0
    for R in (24, 40):
        face, _, d2 = texel_owners(mesh, R, 1.5)
        fid, _ = rasterize_atlas(mesh, R)
        r, c = np.divmod(np.arange(R * R), R)
        covers = TT.raster_covers(uv, R, c, r)
        lowest = np.where(covers.any(1), covers.argmax(1), -1).reshape(R, R)
        assert np.array_equal(lowest, fid.cpu().numpy())
        cov = fid >= 0
        wrong = int((face[cov] != fid[cov]).sum()), int((d2[cov] != 0).sum())
        print(f"R = {R}: {int(cov.sum())} rasterized texels, owner differs on {wrong[0]}, d2 != 0 on {wrong[1]}")
        for r, c in torch.nonzero(cov & (face != fid)).cpu().tolist():
            theirs = TT.project(np.float32([c + 0.5]), np.float32([r + 0.5]), TT.uv_records(uv[int(fid[r, c])][None], R))
            print(f"  texel ({r}, {c}): owner {int(face[r, c])}, rasterizer {int(fid[r, c])} at d2 = {theirs[0][0, 0]:.3e}"
                  f" (its snapping step squared: {(1 / 256) ** 2:.3e})")
        total += sum(wrong)
    assert total == 0


@pytest.mark.gpu
def test_owners_equal_the_restatement():
    """2."""
    from volsurfs_amd.texture_transfer import texel_owners
    mesh = _stack(2)[1]
    for R in (24, 40):
        face, d2 = _assert_owners_equal(mesh, R, 1.5)
        face0, _, _ = texel_owners(mesh, R, 0.0)
        assert torch.equal(face0 >= 0, d2 == 0)
        assert torch.equal(face0[face0 >= 0], face[face0 >= 0])
    hand = _hand_mesh()
    face, d2 = _assert_owners_equal(hand, 16, 1.5)
    _assert_owners_equal(hand, 16, 0.0)
    assert 4 not in set(face.cpu().numpy().ravel().tolist())                 # the NaN face owns nothing
    assert {0, 1, 2, 3} <= set(face.cpu().numpy().ravel().tolist())


@pytest.mark.gpu
def test_every_texel_a_lookup_can_read_is_owned():
    """3.  4 096 surface samples at every degree's resolution: every interior texel of the lerp footprint is owned at
    reach 1.5.  A condition, not a measurement."""
    from volsurfs_amd.mesh_distance import sample_surface
    from volsurfs_amd.texture_transfer import texel_owners
    for mesh in (_stack(1)[0], _stack(2)[2]):
        _, fc, bary = sample_surface(mesh, 4096, seed=3)
        fuv = mesh.faces_uvs.reshape(-1, 6)[fc].cpu().numpy()
        b = bary.cpu().numpy()
        u, v = TT.interp_uv(fuv, b[:, 0], b[:, 1])
        for R in sorted(set(SRC_RES + DST_RES_UP + DST_RES_DOWN)):
            face = texel_owners(mesh, R, 1.5)[0].cpu().numpy()
            i0, j0, _, _ = TT.footprint(u, v, R, False)
            for ky in (0, 1):
                for kx in (0, 1):
                    ix, iy = i0 + kx, j0 + ky
                    ok = (ix >= 0) & (ix < R) & (iy >= 0) & (iy < R)
                    assert ok.sum() > 3000
                    assert (face[R - 1 - ix[ok], iy[ok]] >= 0).all(), (R, kx, ky)


CASES = [  # source subdiv, destination subdiv, samples, lerp, solid inner shell, destination resolutions, builder
    (2, 1, 1, True, False, DST_RES_UP, "host"),
    (1, 2, 2, True, True, DST_RES_DOWN, "device"),
    (2, 1, 2, False, True, DST_RES_DOWN, "ploc"),
    (1, 2, 1, False, False, DST_RES_UP, "device"),
    (2, 1, 1, True, True, DST_RES_DOWN, "ploc"),
    (1, 2, 2, True, False, DST_RES_UP, "host"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:5]) + f"-{c[5][0]}-{c[6]}")
def test_transfer_equals_the_restatement(case):
    """4.  Every byte and every report field, the fp64 sum included."""
    from volsurfs_amd.texture_transfer import transfer_planes
    src_div, dst_div, samples, lerp, solid, res, builder = case
    scene = _scene(_stack(src_div), _random_planes(3, SRC_RES, 7 + src_div, solid), lerp, solid, builder)
    dst = _stack(dst_div)
    max_distance = 0.01                 # (between the 80-face and the 320-face sphere's sagitta: some samples are far)
    planes, reports = transfer_planes(scene, dst, res, samples=samples, max_distance=max_distance)
    want_planes, want_reports = _restated(scene, dst, res, samples, 1.5, max_distance)
    assert set(planes) == set(want_planes)
    for key in sorted(planes):
        got = planes[key].cpu().numpy()
        assert got.shape == want_planes[key].shape
        diff = int((got != want_planes[key]).sum())
        assert diff == 0, (key, diff, got.size)
        r, w = reports[key], want_reports[key]
        for f in ("texels", "owned", "covered", "samples", "far", "max_distance", "sum_d2"):
            assert r[f] == w[f], (key, f, r[f], w[f])
        assert 0 < r["covered"] <= r["owned"] < r["texels"] and r["samples"] == r["owned"] * samples * samples
        assert r["rms_distance"] == (r["sum_d2"] / r["samples"]) ** 0.5


@pytest.mark.gpu
def test_degree_zero_stack_equals_the_restatement():
    """4, SH degree 0: one degree, one coefficient."""
    from volsurfs_amd.texture_transfer import transfer_planes
    scene = _scene(_stack(2), _random_planes(3, (32,), 5, False))
    dst = _stack(1)
    planes, reports = transfer_planes(scene, dst, (24,), samples=2)
    want_planes, want_reports = _restated(scene, dst, (24,), 2, 1.5, np.inf)
    assert set(planes) == {(s, 0) for s in range(3)}
    for key in planes:
        assert np.array_equal(planes[key].cpu().numpy(), want_planes[key]), key
        assert reports[key]["sum_d2"] == want_reports[key]["sum_d2"] and reports[key]["far"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [1, 3])
def test_constant_planes_stay_constant(samples):
    """5."""
    from volsurfs_amd.texture_transfer import texel_owners, transfer_planes
    scene = _scene(_stack(2), _constant_planes(3, SRC_RES, True), solid=True)
    dst = _stack(1)
    planes, _ = transfer_planes(scene, dst, DST_RES_UP, samples=samples)
    for (s, d), p in planes.items():
        owned = (texel_owners(dst[s], DST_RES_UP[d])[0] >= 0).cpu().numpy()
        lut = TT.expand_lut(-SH_RANGE[d], 2 * SH_RANGE[d])
        got = p.cpu().numpy()
        for i in range(2 * d + 1):
            b = int(TT.nearest_byte(lut, lut[_constant_byte(s, d, i)]))
            assert b == _constant_byte(s, d, i)
            a = 255 if s == 0 else b
            assert (got[i][owned] == np.array([b, b, b, a], np.uint8)).all(), (s, d, i)
            assert (got[i][~owned] == np.array([0, 0, 0, 255 if s == 0 else 0], np.uint8)).all(), (s, d, i)


@pytest.mark.gpu
def test_same_geometry_other_atlas_renders_the_same_bytes():
    """6."""
    from volsurfs_amd.texture_transfer import transfer_scene
    scene = _scene(_stack(2), _constant_planes(3, SRC_RES, True), solid=True)
    other = _stack(2, 96, 3)
    assert not torch.equal(other[0].faces_uvs, _stack(2)[0].faces_uvs)
    moved = transfer_scene(scene, other, (48, 24, 24))
    assert torch.equal(moved.bg_color, scene.bg_color) and moved.baked.anchor == scene.baked.anchor
    for eye in ((0.0, 0.3, -2.0), (1.4, -0.9, 0.8), (0.05, 0.1, 0.0), (0.0, 0.0, 0.55)):
        cam = _camera(eye)
        _assert_same_render(scene.render_baked_camera(cam), moved.render_baked_camera(cam))
    for eye in ((0.0, 0.3, -2.0), (1.4, -0.9, 0.8)):
        cam = _camera(eye)
        a, b = scene.render_baked_camera(cam, hits="raster"), moved.render_baked_camera(cam, hits="raster")
        _assert_same_render(a, b)
        assert float(a["rgb"].std()) > 0


@pytest.mark.gpu
def test_write_scene_round_trip(tmp_path):
    """7."""
    from volsurfs_amd.renderers import VolsurfsRenderer
    from volsurfs_amd.texture_export import export_planes, load_scene, write_scene
    from volsurfs_amd.texture_transfer import transfer_scene
    src = _scene(_stack(2), _random_planes(3, SRC_RES, 11, True), solid=True)
    scene = transfer_scene(src, _stack(1), DST_RES_UP)
    meta = write_scene(scene, str(tmp_path / "lod"))
    assert meta["bg_color"] == [0.25, 0.5, 1.0] and len(meta["meshes"]) == 3
    assert [m["ignore_alpha"] for m in meta["meshes"]] == [True, False, False]
    assert os.path.exists(tmp_path / "lod" / "textures" / "mesh_2_texture_2_feature_4.png")
    back = load_scene(str(tmp_path / "lod"), bvh_builder="device")
    a, b = export_planes(scene.baked), export_planes(back.baked)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    cam = _camera((0.3, 0.4, -1.9))
    _assert_same_render(scene.render_baked_camera(cam), back.render_baked_camera(cam))
    r = VolsurfsRenderer.from_scene(str(tmp_path / "lod"), bvh_builder="device")
    _assert_same_render(scene.render_baked_camera(cam), r.render_baked_camera(cam))


@pytest.mark.gpu
def test_make_lod_and_lod_chain(tmp_path):
    """8."""
    from volsurfs_amd.mesh_intersect import shells_nested
    from volsurfs_amd.texture_export import export_planes, load_scene
    from volsurfs_amd.texture_transfer import lod_chain, make_lod
    src = _scene(_stack(2), _random_planes(3, SRC_RES, 13, False))
    assert all(shells_nested(list(_stack(2))))
    scene, report = make_lod(src, 0.5, padding=2)
    assert set(report) == {"simplify", "atlas", "transfer", "faces"}
    assert report["faces"] == [r.faces_out for r in report["simplify"]] == [int(m.faces.shape[0]) for m in scene.tensor_meshes]
    assert all(f < 320 for f in report["faces"])
    assert all(shells_nested(scene.tensor_meshes)) and all(report["simplify"].nested)
    assert len(report["atlas"]) == 3 and set(report["transfer"]) == {(s, d) for s in range(3) for d in range(3)}
    assert all(r["owned"] > 0 for r in report["transfer"].values())
    cam = _camera((0.2, 0.5, -2.0))
    out = scene.render_baked_camera(cam)
    assert out["rgb"].shape == (64 * 64, 3) and bool(torch.isfinite(out["rgb"]).all()) and float(out["rgb"].std()) > 0
    again, _ = make_lod(src, 0.5, padding=2)
    a, b = export_planes(scene.baked), export_planes(again.baked)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(m.faces_uvs, n.faces_uvs) for m, n in zip(scene.tensor_meshes, again.tensor_meshes))
    reports = lod_chain(src, [0.5], str(tmp_path), padding=2)
    assert reports[0] is None and reports[1]["faces"] == report["faces"]
    assert sorted(os.listdir(tmp_path)) == ["lod_0", "lod_1"]
    lod0 = load_scene(str(tmp_path / "lod_0"), bvh_builder="device")
    _assert_same_render(src.render_baked_camera(cam), lod0.render_baked_camera(cam))
    lod1 = load_scene(str(tmp_path / "lod_1"), bvh_builder="device")
    _assert_same_render(scene.render_baked_camera(cam), lod1.render_baked_camera(cam))


@pytest.mark.gpu
def test_argument_errors_raise_before_any_launch():
    """9."""
    from volsurfs_amd._lib import VolsurfsHipError
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.texture_transfer import texel_owners, transfer_planes, transfer_scene
    scene = _scene(_stack(1), _random_planes(3, SRC_RES, 2, False))
    dst = list(_stack(2))
    with pytest.raises(VolsurfsHipError, match="3 shells"):
        transfer_planes(scene, dst[:2])
    bare = TensorMesh(dst[1].vertices, dst[1].faces, None)
    with pytest.raises(VolsurfsHipError, match="UVs"):
        transfer_planes(scene, [dst[0], bare, dst[2]])
    for samples in (0, 5, 1.5):
        with pytest.raises(VolsurfsHipError, match="samples"):
            transfer_planes(scene, dst, samples=samples)
    for reach in (-1.0, float("nan")):
        with pytest.raises(VolsurfsHipError, match="reach"):
            transfer_planes(scene, dst, reach=reach)
        with pytest.raises(VolsurfsHipError, match="reach"):
            texel_owners(dst[0], 16, reach)
    with pytest.raises(VolsurfsHipError, match="resolution"):
        transfer_planes(scene, dst, textures_res=(16, 0, 16))
    method = VolSurfs(list(_stack(1)), max_rays=1024, textures_res=(32, 32, 16, 16))
    with pytest.raises(VolsurfsHipError, match="baked"):
        transfer_scene(method, dst)
    with pytest.raises(VolsurfsHipError, match="baked"):
        method.transfer_to(dst)
