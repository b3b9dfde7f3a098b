"""Mesh repair on the device (volsurfs_amd/mesh_repair.py, csrc/mesh_repair.hip, the `repair=` of volsurfs_amd/mesh_sdf.py;
DESIGN §32) against the rules restated in tests/mesh_repair_restated.py, on the meshes of tests/mesh_winding_restated.py
un-welded into shuffled soups with 40 % of their faces flipped.  The reference has no such stage.  Every discrete result
(maps, flips, components, counts) is compared for equality; nothing here has a tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mesh_repair_restated as R
import mesh_sdf_restated as S
import mesh_winding_restated as W
from volsurfs_amd import _lib

ERR_ARG = -1
gpu = pytest.mark.gpu
# the margin of tests/test_mesh_winding.py for the far field at beta = 2 (twice the largest error measured there)
APPROX_BOUND_2 = 0.0620
WELDED_VERTICES = {"closed": 642, "capped": 593, "lobed": 2562}
UNDECIDED_FACES = {"closed": 0, "capped": 0, "holes": 10, "cube_open": 0, "two_spheres": 0, "lobed": 0}


# ---------------------------------------------------------------------------------------------------------- CPU

def test_entry_points_declared_built_and_prototyped():
    names, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    P, I, LL, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    expected = {
        "vsa_mesh_weld_workspace_bytes": (LL, [LL, LL]),
        "vsa_mesh_weld": (I, [P, LL, P, LL, D, I, I, P, LL, P, P, P, P, P, P, P]),
        "vsa_mesh_orient_workspace_bytes": (LL, [LL, LL]),
        "vsa_mesh_orient": (I, [P, LL, P, LL, I, P, P, LL, P, P, P, P, P, P, P]),
    }
    for n, proto in expected.items():
        assert n in names, f"{n} is not declared in include/volsurfs_hip.h"
        assert hasattr(cdll, n), f"{n} is not in the built library"
        assert protos.get(n) == proto, n


def test_argument_errors_before_any_hip_call():
    """Every VSA_ERR_ARG case of the entry points.  The "device" pointers are null or the address of a host buffer
    nothing reads: each call must return before it touches the GPU (this test runs without one)."""
    L = _lib.lib()
    buf = (ctypes.c_longlong * 16)()
    p = ctypes.addressof(buf)

    for name in ("vsa_mesh_weld_workspace_bytes", "vsa_mesh_orient_workspace_bytes"):
        for v, f in ((0, 4), (-1, 4), (4, 0), (4, -2)):
            assert getattr(L, name)(v, f) == ERR_ARG, (name, v, f)
    assert L.vsa_mesh_weld_workspace_bytes(1 << 31, 4) == -2                      # (VSA_ERR_UNSUPPORTED)
    assert L.vsa_mesh_orient_workspace_bytes(4, (0x7FFFFFFF // 3 - 1) // 2 + 1) == -2    # 2 F has to fit

    def weld(verts=p, V=4, faces=p, F=4, tol=0.0, ws=p, ws_bytes=1 << 30, out_v=p, out_f=p, vmap=p, fmap=p, stats=p):
        return L.vsa_mesh_weld(verts, V, faces, F, tol, 1, 1, ws, ws_bytes, out_v, out_f, vmap, fmap, stats, None, None)

    pointers = ("verts", "faces", "ws", "out_v", "out_f", "vmap", "fmap", "stats")
    null = {k: None for k in pointers}
    for name in pointers:
        assert weld(**{name: None}) == ERR_ARG, name
    for kw in ({"V": 0}, {"V": -3}, {"F": 0}, {"F": -1}, {"tol": -1e-9}, {"tol": -1.0}, {"tol": float("nan")},
               {"tol": float("inf")}, {"ws_bytes": 16}, {"ws_bytes": 0}):
        assert weld(**kw) == ERR_ARG, kw
        assert weld(**dict(null, **kw)) == ERR_ARG, kw

    def orient(verts=p, V=4, faces=p, F=4, uvs=None, ws=p, ws_bytes=1 << 30, out_f=p, out_uvs=None, flipped=p,
               component=p, stats=p):
        return L.vsa_mesh_orient(verts, V, faces, F, 1, uvs, ws, ws_bytes, out_f, out_uvs, flipped, component, stats,
                                 None, None)

    pointers = ("verts", "faces", "ws", "out_f", "flipped", "component", "stats")
    null = {k: None for k in pointers}
    for name in pointers:
        assert orient(**{name: None}) == ERR_ARG, name
    assert orient(uvs=p, out_uvs=None) == ERR_ARG                                  # UVs in, nowhere to write them
    for kw in ({"V": 0}, {"V": -3}, {"F": 0}, {"F": -1}, {"ws_bytes": 16}, {"ws_bytes": 0}):
        assert orient(**kw) == ERR_ARG, kw
        assert orient(**dict(null, **kw)) == ERR_ARG, kw


def test_restatement_against_ground_truth():
    """The rules themselves, in numpy: welding a scrambled soup finds the distinct positions, orienting it gives every
    face of a decided component its original normal, the Moebius strip is one component that cannot be oriented, and
    no component's |S| / U is anywhere near the threshold of 2^-20."""
    for name in R.NAMES:
        v, f = W.mesh(name)
        sv, sf, _ = R.soup(name)
        assert sv.shape == (3 * f.shape[0], 3) and sv.dtype == np.float32 and sf.dtype == np.int32
        assert R.census(sv, sf) == {"boundary": 3 * f.shape[0], "non_manifold": 0, "inconsistent": 0}
        w = R.welded(name)
        distinct = np.unique(v[np.unique(f)], axis=0).shape[0]
        assert w["report"]["vertices_out"] == w["vertices"].shape[0] == distinct, name
        if name in WELDED_VERTICES:
            assert distinct == WELDED_VERTICES[name], name
        assert np.array_equal(w["face_map"], np.arange(f.shape[0])) and w["faces"].shape == f.shape
        assert np.array_equal(w["vertices"][w["faces"]], sv[sf])                    # no corner moved
        o = R.oriented(name)
        agree = (R.normals(v, f) * R.normals(w["vertices"], o["faces"])).sum(1) > 0
        decided = o["decided_face"]
        assert agree[decided].all(), name
        assert o["report"]["undecided_faces"] == int((~decided).sum()) == UNDECIDED_FACES[name], name
        assert o["report"]["undecided_components"] == UNDECIDED_FACES[name]        # (single faces)
        assert o["report"]["unorientable_components"] == 0
        ratios = np.asarray(list(o["ratio"].values()))
        print(name, o["report"], "|S| / U:", np.sort(ratios)[[0, -1]])
        assert ((ratios > 0.05) | (ratios < 2.0 ** -40)).all(), name
        if name in ("closed", "two_spheres", "lobed"):
            assert R.census(w["vertices"], o["faces"]) == {"boundary": 0, "non_manifold": 0, "inconsistent": 0}
            for m in np.unique(o["component"]):              # |S| = 3 x the volume (S: before the component's flip)
                sel = o["component"] == m
                vol = S.signed_volume(w["vertices"], o["faces"][sel])
                assert abs(abs(o["S"][m]) - 3.0 * vol) <= 1e-12 and vol > 0, (name, m)
    mv, mf = R.mobius()
    assert mf.shape == (48, 3) and R.census(mv, mf) == {"boundary": 48, "non_manifold": 0, "inconsistent": 1}
    o = R.oriented("mobius")
    assert o["report"] == {"components": 1, "flipped": 0, "unorientable_components": 1, "undecided_components": 0,
                           "undecided_faces": 0}
    assert not o["flipped"].any() and not o["component"].any()
    # the grouping and the tolerance rule on a few points by hand
    assert R.group_rows(np.array([[3, 1, 2], [0, 0, 0], [3, 1, 2], [0, 0, 1], [0, 0, 0]])).tolist() == [0, 1, 0, 3, 1]
    line = np.array([[0, 0, 0], [0.2, 0, 0], [0.4, 0, 0], [1, 0, 0], [np.nan, 0, 0], [np.nan, 0, 0]], np.float32)
    assert R.weld_rep(line, 0.25).tolist() == [0, 0, 0, 3, 4, 5]
    assert R.weld_rep(line, 0.0).tolist() == [0, 1, 2, 3, 4, 5]
    with pytest.raises(ValueError):
        R.weld_rep(line, 1e-7)


# ---------------------------------------------------------------------------------------------------------- GPU

def _mesh(v, f, uvs=None):
    from volsurfs_amd.mesh import TensorMesh
    m = TensorMesh(np.asarray(v, np.float32), np.asarray(f, np.int32), uvs, device="cuda")
    if uvs is not None:
        m.has_uvs = True
    return m


def _np(t):
    return t.cpu().numpy()


def _same_weld(got, ref, what):
    mesh, vmap, fmap, report = got
    assert np.array_equal(_np(mesh.vertices).view(np.uint32), ref["vertices"].view(np.uint32)), what
    assert mesh.faces.dtype == torch.int32 and np.array_equal(_np(mesh.faces), ref["faces"]), what
    assert vmap.dtype == torch.int32 and np.array_equal(_np(vmap), ref["vertex_map"]), what
    assert fmap.dtype == torch.int32 and np.array_equal(_np(fmap), ref["face_map"]), what
    assert report == ref["report"], what


@gpu
@pytest.mark.parametrize("name", R.NAMES)
def test_weld_exact(name):
    from volsurfs_amd import mesh_repair as MR
    sv, sf, _ = R.soup(name)
    got = MR.weld_vertices(_mesh(sv, sf))
    _same_weld(got, R.welded(name), name)
    if name in WELDED_VERTICES:
        assert got[3]["vertices_out"] == WELDED_VERTICES[name]
    again = MR.weld_vertices(_mesh(sv, sf), stage_ms=(ms := {}))
    assert torch.equal(again[0].faces, got[0].faces) and torch.equal(again[1], got[1]) and set(ms) == set(MR.WELD_STAGES)


def _by_hand():
    """The points that exercise the cells at tol = 0.25, and faces over consecutive triples of them."""
    up = float(np.nextafter(np.float32(0.25), np.float32(1.0)))
    nan = float("nan")
    pts = [[0.1875, 5, 5], [0.3125, 5, 5],                     # 0.5 tol apart across the border between cells 0 and 1
           [10, 0, 0], [10.2, 0, 0], [10.4, 0, 0],             # a chain: |ab|, |bc| <= tol < |ac|
           [20, 0, 0], [20.25, 0, 0],                          # exactly tol apart: one
           [0, 40, 0], [up, 40, 0],                            # the next float32 after tol apart: two
           [-0.05, -7, -7], [0.05, -7, -7],                    # across the border between cells -1 and 0
           [-3.1, -3.1, -3.1], [-3.3, -3.1, -3.1], [-3.1, -3.4, -3.1],
           [0.0, 60, 0], [-0.0, 60, 0],                        # one point at any tol
           [nan, 0, 0], [nan, 0, 0], [1, nan, 1]]              # alone, every one
    pts += [[50, 50, 50]] * 8
    v = np.asarray(pts, np.float32)
    n = v.shape[0]
    f = np.stack([np.arange(n), (np.arange(n) + 1) % n, (np.arange(n) + 2) % n], 1).astype(np.int32)
    return v, f


@gpu
def test_weld_within_a_tolerance():
    from volsurfs_amd import mesh_repair as MR
    sv, sf, _ = R.soup("closed")
    jitter = np.random.default_rng(12).uniform(-1e-6, 1e-6, sv.shape)
    jv = (sv.astype(np.float64) + jitter).astype(np.float32)
    ref = R.weld(jv, sf, 1e-5)
    exact = R.welded("closed")
    assert np.array_equal(ref["vertex_map"], exact["vertex_map"]) and ref["report"]["vertices_out"] == 642
    got = MR.weld_vertices(_mesh(jv, sf), tol=1e-5)
    _same_weld(got, ref, "jittered")
    assert got[3]["vertices_out"] == 642 and np.array_equal(_np(got[1]), exact["vertex_map"])
    v, f = _by_hand()
    rep = R.weld_rep(v, 0.25)
    assert rep[:16].tolist() == [0, 0, 2, 2, 2, 5, 5, 7, 8, 9, 9, 11, 11, 13, 14, 14]
    assert rep[16:19].tolist() == [16, 17, 18] and (rep[19:] == 19).all()
    for tol in (0.25, 0.0, 1e-3):
        for flags in ((True, True), (False, False)):
            _same_weld(MR.weld_vertices(_mesh(v, f), tol, *flags), R.weld(v, f, tol, *flags), (tol, flags))
    with pytest.raises(ValueError, match="tol"):
        MR.weld_vertices(_mesh(sv, sf), tol=1e-7)                 # 0.34 / 1e-7 is beyond 2^20 cells
    for tol in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            MR.weld_vertices(_mesh(sv, sf), tol=tol)


@functools.lru_cache(maxsize=None)
def _welded_input(name):
    if name == "mobius":
        return R.mobius()
    w = R.welded(name)
    return w["vertices"], w["faces"]


@gpu
@pytest.mark.parametrize("name", R.NAMES + ("mobius",))
def test_orient(name):
    from volsurfs_amd import mesh_repair as MR
    v, f = _welded_input(name)
    ref = R.oriented(name)
    mesh, flipped, component, report = MR.orient_faces(_mesh(v, f), stage_ms=(ms := {}))
    assert flipped.dtype == torch.bool and component.dtype == torch.int32 and set(ms) == set(MR.ORIENT_STAGES)
    assert np.array_equal(_np(flipped), ref["flipped"]), name
    assert np.array_equal(_np(component), ref["component"]), name
    assert np.array_equal(_np(mesh.faces), ref["faces"]) and report == ref["report"], name
    assert np.array_equal(_np(mesh.vertices).view(np.uint32), v.view(np.uint32))
    again = MR.orient_faces(_mesh(v, f))
    assert torch.equal(again[0].faces, mesh.faces) and torch.equal(again[1], flipped) and again[3] == report
    assert torch.equal(again[2], component)
    if name == "mobius":
        assert report["unorientable_components"] == 1 and report["flipped"] == 0
        return
    # ground truth: face f of the soup is face f of the mesh it was made from
    ov, of = W.mesh(name)
    agree = (R.normals(ov, of) * R.normals(v, _np(mesh.faces))).sum(1) > 0
    decided = ref["decided_face"]
    assert agree[decided].all(), name
    assert report["undecided_faces"] == int((~decided).sum()) == UNDECIDED_FACES[name]
    assert report["undecided_faces"] <= 0.01 * of.shape[0]
    # an oriented mesh is left alone, and outward=False mirrors every decided component
    second = MR.orient_faces(mesh)
    assert not second[1].any() and torch.equal(second[0].faces, mesh.faces) and second[3]["flipped"] == 0
    inward = MR.orient_faces(mesh, outward=False)
    assert np.array_equal(_np(inward[1]), decided)
    back = MR.orient_faces(inward[0])
    assert torch.equal(back[0].faces, mesh.faces)                                  # flipping twice restores the bits


@gpu
def test_outward_meshes_are_left_alone():
    from volsurfs_amd import mesh_repair as MR
    for name in ("closed", "capped", "cube_open", "two_spheres", "lobed"):
        v, f = W.mesh(name)
        mesh, flipped, _, report = MR.orient_faces(_mesh(v, f))
        assert not flipped.any() and report["flipped"] == 0 and np.array_equal(_np(mesh.faces), f), name


@gpu
def test_duplicates_degenerates_and_attributes():
    from volsurfs_amd import mesh_repair as MR
    from volsurfs_amd.mesh import icosphere
    v, f = icosphere(1, 0.3)
    nv, nf = v.shape[0], f.shape[0]
    junk = np.array([[5, 5, 9], [3, 3, 3], [1, 2, 1]], np.int32)
    # every face twice, the second copy reversed and over a second copy of the vertices; then the junk
    faces = np.concatenate([f, f[:, ::-1] + nv, junk]).astype(np.int32)
    verts = np.concatenate([v, v])
    rng = np.random.default_rng(13)
    uvs = rng.random((faces.shape[0], 3, 2)).astype(np.float32)
    colors = rng.random((2 * nv, 3)).astype(np.float32)
    mesh = _mesh(verts, faces, torch.from_numpy(uvs))
    out, col, vmap, fmap, report = MR.weld_vertices(mesh, vertex_colors=torch.from_numpy(colors).cuda())
    assert report == {"vertices_in": 2 * nv, "vertices_out": nv, "degenerate_dropped": 3, "duplicates_dropped": nf}
    assert np.array_equal(_np(out.vertices), v) and np.array_equal(_np(out.faces), f)      # exactly the first copies
    assert np.array_equal(_np(vmap), np.concatenate([np.arange(nv), np.arange(nv)]))
    assert np.array_equal(_np(fmap), np.concatenate([np.arange(nf), np.full(nf + 3, -1)]))
    assert out.has_uvs and np.array_equal(_np(out.get_faces_uvs()).reshape(-1, 3, 2), uvs[:nf])
    assert np.array_equal(_np(col), colors[:nv])
    ref = R.weld(verts, faces)
    _same_weld((out, vmap, fmap, report), ref, "doubled")
    # kept when not asked to drop
    kept = MR.weld_vertices(mesh, drop_degenerate=False, drop_duplicates=False)
    _same_weld(kept, R.weld(verts, faces, 0.0, False, False), "kept")
    assert kept[0].faces.shape[0] == 2 * nf + 3
    # the UVs follow the flips
    flip = rng.random(nf) < 0.5
    scrambled = f.copy()
    scrambled[flip] = scrambled[flip][:, [0, 2, 1]]
    src = _mesh(v, scrambled, torch.from_numpy(uvs[:nf]))
    fixed, flipped, _, rep = MR.orient_faces(src)
    assert np.array_equal(_np(fixed.faces), f) and np.array_equal(_np(flipped), flip) and rep["flipped"] == int(flip.sum())
    want = uvs[:nf].copy()
    want[flip] = want[flip][:, [0, 2, 1]]
    assert fixed.has_uvs and np.array_equal(_np(fixed.get_faces_uvs()).reshape(-1, 3, 2), want)


@gpu
def test_repaired_meshes_take_their_sign():
    from volsurfs_amd import mesh_repair as MR
    from volsurfs_amd import mesh_sdf as MS
    zero = {"boundary": 0, "non_manifold": 0, "inconsistent": 0}
    for name in ("closed", "lobed"):
        v, f = W.mesh(name)
        sv, sf, _ = R.soup(name)
        repaired, report = MR.repair_mesh(_mesh(sv, sf))
        assert report["census_before"] == dict(zero, boundary=3 * f.shape[0]) and report["census_after"] == zero, name
        assert report["vertices_out"] == WELDED_VERTICES[name] and report["components"] == 1
        q = torch.from_numpy(W.queries(name)).cuda()
        inside = MS.contains(q, _mesh(v, f))
        assert torch.equal(MS.contains(q, repaired), inside) and 0 < int(inside.sum()) < q.shape[0], name
        assert not torch.equal(MS.contains(q, _mesh(sv, sf)), inside), name        # the soup itself has no such sign
    v, f = W.mesh("capped")
    sv, sf, _ = R.soup("capped")
    repaired, report = MR.repair_mesh(_mesh(sv, sf))
    assert report["census_after"] == dict(zero, boundary=W.boundary_edges(f))
    q = torch.from_numpy(W.queries("capped")).cuda()
    w64 = W.oracle("capped")
    sure = np.abs(w64 - 0.5) > APPROX_BOUND_2
    negative = _np(torch.signbit(MS.signed_distance(q, repaired, sign="winding")["dist"]))
    original = _np(torch.signbit(MS.signed_distance(q, _mesh(v, f), sign="winding")["dist"]))
    assert np.array_equal(negative[sure], (w64 > 0.5)[sure]) and np.array_equal(negative[sure], original[sure])
    # weld or orient alone
    only, r = MR.repair_mesh(_mesh(sv, sf), orient=False)
    assert "components" not in r and r["census_after"]["inconsistent"] > 0 and r["vertices_out"] == 593
    only, r = MR.repair_mesh(_mesh(sv, sf), weld=False)
    assert "vertices_out" not in r and r["components"] == f.shape[0] and r["undecided_faces"] == f.shape[0]


@gpu
def test_shells_from_a_soup():
    from volsurfs_amd import mesh_sdf as MS
    from volsurfs_amd import mesh_winding as MW
    sv, sf, _ = R.soup("closed")
    meshes, levels, report = MS.offset_shells(_mesh(sv, sf), 3, nr_points_per_dim=48, repair=True, return_report=True)
    assert len(meshes) == 3 and len(levels) == 3 and report["vertices_out"] == 642
    assert report["census_after"] == {"boundary": 0, "non_manifold": 0, "inconsistent": 0}
    for m in meshes:
        assert m.faces.shape[0] > 0 and MW.is_closed(m)
    nesting = MS.shell_nesting(meshes, n=5037, seed=0)
    print(nesting)
    assert [c["pair"] for c in nesting] == [(0, 1), (1, 2)] and all(c["outside"] == 0 for c in nesting)
    two = MS.offset_shells(_mesh(sv, sf), 3, nr_points_per_dim=48, repair=True)
    assert len(two) == 2 and all(torch.equal(a.faces, b.faces) and torch.equal(a.vertices, b.vertices)
                                 for a, b in zip(two[0], meshes))
    # repair=False is the call without the argument, byte for byte
    v, f = W.mesh("closed")
    plain = MS.offset_shells(_mesh(v, f), 3, nr_points_per_dim=48)
    off = MS.offset_shells(_mesh(v, f), 3, nr_points_per_dim=48, repair=False)
    assert len(off) == 2 and off[1] == plain[1]
    for a, b in zip(off[0], plain[0]):
        assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)
    assert MS.offset_shells(_mesh(v, f), 3, nr_points_per_dim=48, return_report=True)[2] is None


@gpu
def test_repair_meshes_round_trip(tmp_path):
    from volsurfs_amd import mesh_repair as MR
    from volsurfs_amd.mesh import load_ply, save_ply
    src = tmp_path / "meshes"
    src.mkdir()
    names = {"-0.01.ply": "cube_open", "0.01.ply": "two_spheres"}
    for file, name in names.items():
        sv, sf, _ = R.soup(name)
        save_ply(str(src / file), _mesh(sv, sf))
    paths, reports = MR.repair_meshes(str(src), str(tmp_path / "meshes_repaired"))
    assert [p.split("/")[-1] for p in paths] == list(names) and len(reports) == 2
    for path, name in zip(paths, names.values()):
        ref = R.oriented(name)
        m = load_ply(path)
        assert np.array_equal(_np(m.vertices), R.welded(name)["vertices"]) and np.array_equal(_np(m.faces), ref["faces"])
    assert reports[1]["census_after"] == {"boundary": 0, "non_manifold": 0, "inconsistent": 0}
    assert reports[0]["vertices_out"] == 8 and reports[1]["components"] == 2
