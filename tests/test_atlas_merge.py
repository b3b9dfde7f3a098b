"""Merged charts (compute_atlas(charts="merged"), vsa_atlas_merged).

`atlas_merge_restated.restate_merged` is the numpy restatement of the rules in include/volsurfs_hip.h; the kernels are
held to it bit for bit, and it is itself held to atlas validity (test_atlas._check_atlas's rules with the area test
generalised: a face of a merged group keeps at least min_cos of its area along its group's D, a face of an unmerged
group at least half along its label) and, where nothing merges, to test_atlas.restate byte for byte.

Measured with the restatement (R = 512, p = 4; box charts -> groups, merge rounds run, charts after splits, utilization):
A: box 39 charts 0.389; 0.5: 39 -> 32, 4 rounds, 32, 0.391; 0.3: 39 -> 9, 9 rounds, 9, 0.453.
B: box 309 -> 374 charts 0.269; 0.5: 309 -> 209, 8 rounds, 279, 0.305; 0.3: 309 -> 70, 51 rounds, 151, 0.335."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from volsurfs_amd import atlas
from volsurfs_amd.mesh import icosphere

from tests.atlas_merge_restated import face_normals, restate_merged
from tests.test_atlas import GPU_MESHES, MESHES, restate
from uv_raster_restated import raster

R0, P0 = 512, 4


@functools.lru_cache(None)
def _noisy_ico():
    P, F = icosphere(4, 0.5)
    P = np.asarray(P, np.float64)
    d = P / np.linalg.norm(P, axis=1, keepdims=True)
    lobes = 1 + 0.15 * np.sin(5 * d[:, 0]) * np.sin(4 * d[:, 1]) * np.cos(3 * d[:, 2])
    rng = np.random.default_rng(0)
    A = (P * lobes[:, None] + rng.normal(0, 0.004, P.shape)).astype(np.float32)
    B = (P * lobes[:, None] + rng.normal(0, 0.008, P.shape)).astype(np.float32)
    return (A, np.asarray(F)), (B, np.asarray(F))


CPU_MESHES = dict(MESHES, A=lambda: _noisy_ico()[0], B=lambda: _noisy_ico()[1])
ALL_MESHES = dict(GPU_MESHES, A=CPU_MESHES["A"], B=CPU_MESHES["B"])


@functools.lru_cache(None)
def _mesh(name):
    return ALL_MESHES[name]()


@functools.lru_cache(None)
def _restated(name, R, p, min_cos, rounds=64):
    """One restatement per case, shared by the tests that need it and left unchanged."""
    P, F = _mesh(name)
    return restate_merged(P, F, R, p, min_cos, rounds, return_groups=True)


@functools.lru_cache(None)
def _box_restated(name, R, p):
    P, F = _mesh(name)
    return restate(P, F, R, p)


def _check_merged_atlas(P, F, uv, chart, groups, st, R, p, min_cos):
    """test_atlas._check_atlas's rules, the area test generalised to merged groups."""
    lab, grp, merged, A = groups
    P64 = np.asarray(P, np.float64)
    F = np.asarray(F, np.int64)
    assert uv.shape == (len(F), 3, 2) and (uv >= 0).all() and (uv <= 1).all()
    u = uv.astype(np.float64)
    area_uv = 0.5 * ((u[:, 1, 0] - u[:, 0, 0]) * (u[:, 2, 1] - u[:, 0, 1])
                     - (u[:, 1, 1] - u[:, 0, 1]) * (u[:, 2, 0] - u[:, 0, 0]))
    perim = np.linalg.norm(u[:, 1] - u[:, 0], axis=1) + np.linalg.norm(u[:, 2] - u[:, 1], axis=1) + \
        np.linalg.norm(u[:, 0] - u[:, 2], axis=1)
    assert (area_uv >= -4.0 * 2.0 ** -24 * perim).all(), "a face flips in UV"
    n = np.cross(P64[F[:, 1]] - P64[F[:, 0]], P64[F[:, 2]] - P64[F[:, 0]])
    nl = np.linalg.norm(n, axis=1)
    in_m = merged[grp]
    # unmerged groups: the old half-area test against the label
    d = np.where(lab & 1, -1.0, 1.0) * n[np.arange(len(F)), lab >> 1]
    k = (nl > 0) & ~in_m
    assert (d[k] >= (0.5 - 1e-6) * nl[k]).all(), "a face of an unmerged group keeps less than half its area"
    # merged groups: rule 3 against the group's D, on the label stage's fp32 normals in fp64, as the rule states it
    n32 = face_normals(np.asarray(P, np.float32), F).astype(np.float64)
    D = A[grp]
    c = (n32[:, 0] * D[:, 0] + n32[:, 1] * D[:, 1]) + n32[:, 2] * D[:, 2]
    nn = (n32[:, 0] * n32[:, 0] + n32[:, 1] * n32[:, 1]) + n32[:, 2] * n32[:, 2]
    DD = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
    k = in_m & (nn > 0)
    assert ((c[k] > 0) & (c[k] * c[k] >= ((min_cos * min_cos) * nn[k]) * DD[k])).all(), "rule 3 fails in a merged group"
    # the projected area along the direction each face is projected along, against the UV area at the returned scale
    proj = np.where(in_m, (n * D).sum(1) / np.sqrt(np.maximum(DD, 1e-300)), d)
    k = nl > 1e-3 * nl.max()
    ratio = area_uv[k] / (0.5 * proj[k] * (st["scale"] / R) ** 2)
    assert np.allclose(ratio, 1.0, atol=1e-2), (ratio.min(), ratio.max())
    fid, count, _, _ = raster(uv, R)
    assert count.max() <= 1, "a texel is covered twice"
    assert int((count > 0).sum()) == st["covered"]
    cm = np.where(fid >= 0, np.asarray(chart)[np.maximum(fid, 0)], -1)
    g = 2 * p
    pad = np.full((R + 2 * g, R + 2 * g), -1, np.int64)
    pad[g:g + R, g:g + R] = cm
    for di in range(-g, g + 1):
        for dj in range(-g, g + 1):
            sh = pad[g + dj:g + dj + R, g + di:g + di + R]
            assert not ((cm >= 0) & (sh >= 0) & (sh != cm)).any(), "two charts closer than 2p texels"
    assert st["charts"] == int(np.asarray(chart).max()) + 1
    assert st["groups"] == len(np.unique(grp)) and st["groups"] <= st["box_charts"]


# ------------------------------------------------------------------------------------------------ no GPU needed

@pytest.mark.parametrize("min_cos", [0.5, 0.3])
@pytest.mark.parametrize("name", list(CPU_MESHES))
def test_restatement_is_a_valid_atlas(name, min_cos):
    P, F = _mesh(name)
    uv, chart, st, groups = _restated(name, R0, P0, min_cos)
    _check_merged_atlas(P, F, uv, chart, groups, st, R0, P0, min_cos)
    print(f"{name} @{min_cos}: box charts {st['box_charts']} -> groups {st['groups']} in {st['merge_rounds']} rounds, "
          f"charts {st['charts']}, split rounds {st['split_rounds']}, utilization {st['covered'] / R0 ** 2:.3f}")


@pytest.mark.parametrize("name", ["ico3", "torus", "helix"])
def test_no_merges_is_the_box_atlas(name):
    uv, chart, st, _ = _restated(name, R0, P0, 0.5)
    buv, bchart, bst = _box_restated(name, R0, P0)
    assert st["groups"] == st["box_charts"] and st["valid_pairs_left"] == 0
    assert uv.tobytes() == buv.tobytes() and chart.tobytes() == bchart.tobytes()
    assert {k: st[k] for k in bst} == bst


def test_groups_on_the_noisy_ico():
    for name in ("A", "B"):
        half, third = _restated(name, R0, P0, 0.5)[2], _restated(name, R0, P0, 0.3)[2]
        print(name, half, third)
        assert half["groups"] < half["box_charts"]
        assert third["groups"] <= third["box_charts"] // 2
    assert _restated("A", R0, P0, 0.5)[2]["valid_pairs_left"] == 0
    assert _restated("A", R0, P0, 0.3)[2]["valid_pairs_left"] == 0
    assert _restated("B", R0, P0, 0.3)[2]["merge_rounds"] <= 64
    assert _restated("B", R0, P0, 0.3)[2]["valid_pairs_left"] == 0


def test_two_rounds_stop_early_on_a_valid_atlas():
    P, F = _mesh("B")
    uv, chart, st, groups = _restated("B", R0, P0, 0.3, 2)
    assert st["merge_rounds"] == 2 and st["valid_pairs_left"] > 0
    assert st["groups"] < st["box_charts"]
    _check_merged_atlas(P, F, uv, chart, groups, st, R0, P0, 0.3)


def test_zero_rounds_is_the_box_atlas():
    uv, chart, st, _ = _restated("B", R0, P0, 0.3, 0)
    buv, bchart, bst = _box_restated("B", R0, P0)
    assert uv.tobytes() == buv.tobytes() and chart.tobytes() == bchart.tobytes()
    assert {k: st[k] for k in bst} == bst and st["merge_rounds"] == 0 and st["groups"] == st["box_charts"]


def test_zero_area_faces_never_make_a_zero_direction():
    """Faces with n_f = 0 pass rule 3 against any D, but they all carry label 0, so adjacent ones are one box chart and
    no pair of groups consists of them alone: every merged group has D != 0 and a finite frame."""
    P, F = _mesh("B")
    P = P.copy()
    for f in (10, 700, 2500, 4000):                    # collapse an edge: the two faces at it get zero area
        P[F[f, 1]] = P[F[f, 0]]
    uv, chart, st, (lab, grp, merged, A) = restate_merged(P, F, R0, P0, 0.3, 64, return_groups=True)
    assert ((face_normals(P, F) == 0).all(1)).sum() >= 8 and st["groups"] < st["box_charts"]
    assert ((A[merged] * A[merged]).sum(1) > 0).all() and np.isfinite(uv).all()
    _check_merged_atlas(P, F, uv, chart, (lab, grp, merged, A), st, R0, P0, 0.3)


def test_arguments_are_refused_before_any_device_call():
    from volsurfs_amd.mesh import TensorMesh
    V, F = icosphere(1, 0.5)
    m = TensorMesh(V, F, None, device="cpu")        # a cpu mesh: reaching the mesh check would raise for that instead
    with pytest.raises(ValueError, match="charts must be one of"):
        atlas.compute_atlas(m, charts="nonsense")
    for bad in (0, 1.5, float("nan"), -0.2):
        with pytest.raises(ValueError, match="min_cos"):
            atlas.compute_atlas(m, charts="merged", min_cos=bad)
    with pytest.raises(ValueError, match="merge_rounds"):
        atlas.compute_atlas(m, charts="merged", merge_rounds=-1)
    with pytest.raises(ValueError, match="charts must be one of"):
        atlas.compute_meshes_atlas("nowhere", "nowhere", charts="nonsense")


# ------------------------------------------------------------------------------------------------------- GPU

def _gpu(P, F, R, p, **kw):
    from volsurfs_amd.mesh import TensorMesh
    m = TensorMesh(torch.from_numpy(np.asarray(P, np.float32)), torch.from_numpy(np.asarray(F, np.int32)), None,
                   device="cuda")
    return atlas.compute_atlas(m, R, p, return_stats=True, return_charts=True, **kw)


def _assert_equals_restatement(got, want):
    m, gst, gchart = got
    uv, chart, st = want[:3]
    assert torch.equal(m.faces_uvs.cpu().view(torch.int32), torch.from_numpy(uv).view(torch.int32))
    assert torch.equal(gchart.cpu(), torch.from_numpy(chart))
    assert {k: gst[k] for k in st} == st


@pytest.mark.gpu
@pytest.mark.parametrize("min_cos", [0.5, 0.3])
@pytest.mark.parametrize("R,p", [(256, 2), (1024, 4)])
@pytest.mark.parametrize("name", ["ico3", "torus", "helix", "A", "B", "sphere_simplified", "lobed_simplified"])
def test_exact_vs_restatement(name, R, p, min_cos):
    P, F = _mesh(name)
    want = _restated(name, R, p, min_cos)
    got = _gpu(P, F, R, p, charts="merged", min_cos=min_cos)
    again = _gpu(P, F, R, p, charts="merged", min_cos=min_cos)
    _assert_equals_restatement(got, want)
    assert torch.equal(got[0].faces_uvs.view(torch.int32), again[0].faces_uvs.view(torch.int32))
    assert torch.equal(got[2], again[2]) and got[1] == again[1]
    st = got[1]
    print(f"{name} R={R} p={p} @{min_cos}: F {len(F)}, box charts {st['box_charts']} -> groups {st['groups']} in "
          f"{st['merge_rounds']} rounds, charts {st['charts']}, split rounds {st['split_rounds']}, "
          f"utilization {st['utilization']:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ico3", "torus"])
def test_no_merges_is_the_box_atlas_on_the_device(name):
    P, F = _mesh(name)
    m, st, chart = _gpu(P, F, R0, P0, charts="merged")
    b, bst, bchart = _gpu(P, F, R0, P0, charts="box")
    assert torch.equal(m.faces_uvs.view(torch.int32), b.faces_uvs.view(torch.int32)) and torch.equal(chart, bchart)
    assert {k: st[k] for k in bst} == bst and st["groups"] == st["box_charts"] == bst["charts"]
    assert set(st) - set(bst) == {"box_charts", "groups", "merge_rounds", "valid_pairs_left"}


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", [0, 1, 2, 64])
def test_round_loop_and_early_stop(rounds):
    P, F = _mesh("B")
    got = _gpu(P, F, R0, P0, charts="merged", min_cos=0.3, merge_rounds=rounds)
    _assert_equals_restatement(got, _restated("B", R0, P0, 0.3, rounds))
    assert got[1]["merge_rounds"] == (rounds if rounds < 64 else _restated("B", R0, P0, 0.3)[2]["merge_rounds"])
    if rounds == 0:
        b, bst, bchart = _gpu(P, F, R0, P0, charts="box")
        assert torch.equal(got[0].faces_uvs.view(torch.int32), b.faces_uvs.view(torch.int32))
        assert torch.equal(got[2], bchart) and {k: got[1][k] for k in bst} == bst


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_raster_of_the_merged_atlas(name):
    P, F = _mesh(name)
    stage_ms = {}
    m, st, _ = _gpu(P, F, R0, P0, charts="merged", min_cos=0.3, stage_ms=stage_ms)
    _, count = atlas.rasterize_atlas(m, R0)
    assert int(count.max()) <= 1 and int((count > 0).sum()) == st["covered"]
    assert tuple(stage_ms) == atlas.MERGED_STAGES and stage_ms["merge"] > 0


@pytest.mark.gpu
def test_workspace_is_linear_and_bad_arguments_are_err_arg():
    from volsurfs_amd import _lib
    a, b = atlas.merged_workspace_bytes(1000, 2000, 256), atlas.merged_workspace_bytes(100000, 200000, 256)
    r = 4 * 256 * 256
    assert a > r and b > r
    assert (b - r) < 101 * (a - r)
    assert atlas.merged_workspace_bytes(1000, 2000, 1024) - a == 4 * (1024 ** 2 - 256 ** 2)
    assert a > atlas.workspace_bytes(1000, 2000, 256)
    V, F = icosphere(2, 0.5)
    P = torch.from_numpy(np.asarray(V, np.float32)).cuda()
    Fd = torch.from_numpy(np.asarray(F, np.int32)).cuda()
    nv, nf = int(P.shape[0]), int(Fd.shape[0])
    need = atlas.merged_workspace_bytes(nv, nf, 256)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    uv = torch.empty(nf, 3, 2, device="cuda")
    chart = torch.empty(nf, dtype=torch.int32, device="cuda")
    stats = (ctypes.c_longlong * 8)()
    scale = ctypes.c_float(0.0)

    def call(min_cos, rounds, nbytes):
        return _lib.lib().vsa_atlas_merged(P.data_ptr(), nv, Fd.data_ptr(), nf, 256, 2, min_cos, rounds, ws.data_ptr(),
                                           nbytes, uv.data_ptr(), chart.data_ptr(), ctypes.addressof(stats),
                                           ctypes.addressof(scale), None, _lib.stream_ptr().value)

    ERR_ARG = -1
    assert call(0.5, 64, need - 1) == ERR_ARG          # a short workspace
    assert call(0.0, 64, need) == ERR_ARG
    assert call(1.5, 64, need) == ERR_ARG
    assert call(float("nan"), 64, need) == ERR_ARG
    assert call(0.5, -1, need) == ERR_ARG
    assert call(0.5, 64, need) == 0 and stats[0] == 6 and stats[4] == 6 and stats[5] == 6


@pytest.mark.gpu
def test_end_to_end_files_training_and_lod(tmp_path):
    from tests.test_isosurface import _lobed_fn as lobed
    from tests.test_texture_transfer import SRC_RES, _random_planes, _scene, _stack
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.camera import pinhole_rays
    from volsurfs_amd.mesh import load_obj, load_ply
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.simplify import simplify_meshes
    from volsurfs_amd.texture_transfer import make_lod
    meshes, levels = iso.extract_level_sets(lobed, 64, 2, delta_surfs=0.01)
    raw, simp, uvd = (str(tmp_path / d) for d in ("meshes", "meshes_simplified", "meshes_simplified_uvs"))
    iso.save_level_sets(meshes, levels, raw)
    simplify_meshes(raw, simp, 0.1)
    paths = atlas.compute_meshes_atlas(simp, uvd, 1024, 4, charts="merged", min_cos=0.3)
    stems = [f"{round(lv, 4)}" for lv in levels]
    assert [os.path.basename(x) for x in paths] == [s + ".obj" for s in stems]
    for s, path in zip(stems, paths):
        assert os.path.getsize(os.path.join(uvd, "atlas", s + ".png")) > 0
        want, st = atlas.compute_atlas(load_ply(os.path.join(simp, s + ".ply")), 1024, 4, return_stats=True,
                                       charts="merged", min_cos=0.3)
        got = load_obj(path)
        assert got.has_uvs and torch.equal(got.faces_uvs, want.faces_uvs) and torch.equal(got.faces, want.faces)
        assert 1 <= st["groups"] <= st["box_charts"]
    m = VolSurfs.from_meshes_path(uvd, str(tmp_path / "ckpt"), using_neural_textures=True, max_rays=4096,
                                  textures_res=(256, 128, 64, 32), nr_warmup_iters=2, lr=2e-3)
    o, d = pinhole_rays(48, 48, focal=60.0, cam_pos=(0.0, 0.0, -1.6))
    gt = torch.rand(48 * 48, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) * 0.2 + 0.4
    loss = m(o, d, gt, iter_nr=0, is_first_iter=True)[0]["loss"]
    loss.backward()
    assert torch.isfinite(loss)
    grads = [q.grad for q in m.parameters() if q.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    src = _scene(_stack(2), _random_planes(3, SRC_RES, 13, False))
    scene, report = make_lod(src, 0.5, padding=2, charts="merged", min_cos=0.3)
    assert len(report["atlas"]) == 3 and all("groups" in st for st in report["atlas"])


@pytest.mark.gpu
def test_large_shell_is_deterministic_and_exact():
    """The lobed n = 512 shell simplified to 0.1 of test_atlas (about 60k faces: deep union-find trees, a split round)
    at min_cos = 0.4: the same bits on three calls, and the restatement's."""
    from tests.test_isosurface import _h, _lobed_fn
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.simplify import simplify_mesh
    n = 512
    mc = iso.marching_cubes(iso.sample_grid(_lobed_fn, n), [0.0], [-1.0] * 3, [_h(n)] * 3)[0]
    m = simplify_mesh(mc, 0.1)
    del mc
    runs = [atlas.compute_atlas(m, 1024, 4, return_stats=True, return_charts=True, charts="merged", min_cos=0.4)
            for _ in range(3)]
    for a, st, ch in runs[1:]:
        assert torch.equal(a.faces_uvs.view(torch.int32), runs[0][0].faces_uvs.view(torch.int32))
        assert torch.equal(ch, runs[0][2]) and st == runs[0][1]
    P, F = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
    want = restate_merged(P, F, 1024, 4, 0.4, 64)
    st = runs[0][1]
    print(f"lobed n=512 @0.1, min_cos 0.4: F {len(F)}, box charts {st['box_charts']} -> groups {st['groups']} in "
          f"{st['merge_rounds']} rounds, charts {st['charts']}, split rounds {st['split_rounds']}, "
          f"utilization {st['utilization']:.3f}")
    assert len(F) > 50000 and st["groups"] < st["box_charts"]
    _assert_equals_restatement(runs[0], want)
