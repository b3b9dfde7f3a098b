"""Guarded simplification and the shell stack (csrc/simplify.hip: smp_guard, vsa_simplify_guarded;
volsurfs_amd/simplify.py: simplify_mesh(guards=), simplify_shells, simplify_meshes_nested).

tests/simplify_guarded_restated.py restates the rule (include/volsurfs_hip.h "Mesh simplification": `guard`; DESIGN
§36) in numpy; the kernels are held to it bit for bit on two small lobed stacks (G1, G2) and on an open mesh.  What the
rule promises -- no consecutive pair of outputs has more crossing pairs than its inputs, none for a stack that had none
-- is checked on marching-cubes shells (C, D), where simplifying every shell on its own makes them cross."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import mesh_intersect_restated as mir
from tests import simplify_guarded_restated as sgr
from tests.test_isosurface import _h, _lobed, _topology
from tests.test_simplify import MESHES, _boundary_loops, _check_valid, restate as plain_restate
from volsurfs_amd import _lib
from volsurfs_amd import simplify as smp
from volsurfs_amd.mesh import icosphere

gpu = pytest.mark.gpu

# The figures of the rule's first numpy prototype for G1 / G2 at ratio 0.25 (per shell, inner to outer).
G1_ROUNDS, G1_FACES = [21, 22, 21], [80, 80, 80]
G2_FACES = [82, 124, 94]


@functools.lru_cache(maxsize=None)
def _stack(name):
    return sgr.lobed_stack(**{"G1": sgr.G1, "G2": sgr.G2}[name])


@functools.lru_cache(maxsize=None)
def _restated_stack(name, anchor):
    return sgr.restate_shells(_stack(name), sgr.G_RATIO, anchor)


@functools.lru_cache(maxsize=None)
def _plain(name, ratio):
    return plain_restate(*MESHES[name](), ratio)


def _far():
    v, f = icosphere(0)
    return (v * np.float32(10.0)).astype(np.float32), f


def _winding(point, V, F):
    """The winding number of the closed mesh (V, F) about `point` (Van Oosterom-Strackee solid angles, float64)."""
    T = np.asarray(V, np.float64)[np.asarray(F, np.int64)] - np.asarray(point, np.float64)
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    la, lb, lc = (np.linalg.norm(x, axis=1) for x in (a, b, c))
    num = np.einsum("ij,ij->i", a, np.cross(b, c))
    den = la * lb * lc + (a * b).sum(1) * lc + (b * c).sum(1) * la + (c * a).sum(1) * lb
    return 2.0 * np.arctan2(num, den).sum() / (4.0 * np.pi)


# ------------------------------------------------------------------------------------------------ no GPU needed

@pytest.mark.parametrize("name", ["G1", "G2"])
def test_restated_stack_stays_nested(name):
    meshes = _stack(name)
    out, reports, cin, cout = _restated_stack(name, None)
    assert cin == [0, 0] and cout == [0, 0]
    plain = [plain_restate(v, f, sgr.G_RATIO)[:2] for v, f in meshes]
    assert sum(sgr.crossing_pairs(plain[k], plain[k + 1]) for k in range(2)) > 0, "the plain path must cross here"
    for k in range(2):                                      # no crossing + one vertex inside = shell k inside k + 1
        assert len(mir.mesh_crossings(*out[k], *out[k + 1])["pairs"]) == 0
        assert round(_winding(out[k][0][0], *out[k + 1])) == 1
        assert round(_winding(out[k + 1][0][0], *out[k])) == 0
    for k, (r, (v, f)) in enumerate(zip(reports, out)):
        assert r["shell"] == k and r["faces_in"] == 320 and r["target"] == 80 and r["faces_out"] == len(f)
        assert r["self_crossings"] == 0 and r["guard_rejected"] > 0
        _check_valid(v, f, 2)
    assert [r["guards"] for r in reports] == [(("out", 1),), (("in", 0), ("in", 2)), (("out", 1),)]
    if name == "G1":
        assert not any(r["stalled"] for r in reports)
        assert [r["faces_out"] for r in reports] == G1_FACES and [r["rounds"] for r in reports] == G1_ROUNDS
    else:
        assert all(r["stalled"] for r in reports) and [r["faces_out"] for r in reports] == G2_FACES


def test_stack_order():
    assert sgr.stack_order(5) == [(2, [("in", 1), ("in", 3)]), (3, [("out", 2), ("in", 4)]), (4, [("out", 3)]),
                                  (1, [("in", 0), ("out", 2)]), (0, [("out", 1)])]
    assert sgr.stack_order(3, 0) == [(0, [("in", 1)]), (1, [("out", 0), ("in", 2)]), (2, [("out", 1)])]
    assert sgr.stack_order(2) == [(1, [("in", 0)]), (0, [("out", 1)])]


@pytest.mark.parametrize("name", ["ico3", "torus"])
def test_far_guard_leaves_the_restated_bytes(name):
    V, F, st = _plain(name, 0.1)
    v, f, gst = sgr.restate(*MESHES[name](), 0.1, [_far()])
    assert np.array_equal(v.view(np.int32), V.view(np.int32)) and np.array_equal(f, F)
    assert gst["guard_rejected"] == 0 and {k: gst[k] for k in st} == st


def test_guard_faces_out_of_range_are_no_faces():
    v, f = _far()
    bad = np.concatenate([f, [[0, 1, len(v)], [-1, 0, 1]]]).astype(np.int32)
    assert np.array_equal(sgr.guard_triangles(v, bad), sgr.guard_triangles(v, f))


def test_entry_points_declared_built_and_prototyped():
    names, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    expected = {
        "vsa_simplify_guarded_workspace_bytes": (LL, [LL, LL]),
        "vsa_simplify_guarded": (I, [P, LL, P, LL, LL, I, P, P, P, P, P, P, P, P, P, P, LL, P, P, P, P, P]),
    }
    for n, proto in expected.items():
        assert n in names, f"{n} is not declared in include/volsurfs_hip.h"
        assert hasattr(cdll, n), f"{n} is not in the built library"
        assert protos.get(n) == proto, n
    for n in ("simplify_shells", "simplify_meshes_nested", "ShellSimplifyReport"):
        assert n in smp.__all__ and hasattr(smp, n)
    assert smp.ShellSimplifyReport._fields == sgr.REPORT_FIELDS
    assert smp.GUARDED_STAGES == ("init", "edges", "cost", "guard", "select", "collapse", "compact")


def test_entry_point_argument_errors_before_any_hip_call():
    """Every VSA_ERR_ARG case of the guard arguments.  The "device" pointers are null or the address of a host buffer
    nothing reads: each call must return before it touches the GPU (this test runs without one)."""
    L = _lib.lib()
    buf = (ctypes.c_longlong * 16)()
    p = ctypes.addressof(buf)
    ERR_ARG, ERR_UNSUPPORTED = -1, -2

    def call(nr=2, qnodes=(p, p), tris=(p, p), roots=(0, 0), frames=True, depths=(10, 10), verts=(p, p), nv=(5, 5),
             faces=(p, p), nf=(5, 5), drop=None):
        ptrs = lambda xs: (ctypes.c_void_p * 4)(*xs)
        args = {"qnodes": ptrs(qnodes), "tris": ptrs(tris), "roots": (ctypes.c_int32 * 4)(*roots),
                "frames": (ctypes.c_float * 24)(*([0, 0, 0, 1, 1, 1] * 4)) if frames else None,
                "depths": (ctypes.c_int32 * 4)(*depths), "verts": ptrs(verts), "nv": (ctypes.c_longlong * 4)(*nv),
                "faces": ptrs(faces), "nf": (ctypes.c_longlong * 4)(*nf)}
        if drop:
            args[drop] = None
        return L.vsa_simplify_guarded(p, 1 << 32, p, 100, 10, nr, args["qnodes"], args["tris"], args["roots"],
                                      args["frames"], args["depths"], args["verts"], args["nv"], args["faces"],
                                      args["nf"], p, 1 << 30, p, p, p, None, None)

    # (the mesh has 2^32 vertices: with good guards the call gets as far as vsa_simplify's own size check and returns
    # VSA_ERR_UNSUPPORTED, still before any HIP call; a bad guard argument is found first)
    assert call() == ERR_UNSUPPORTED
    assert call(nr=1) == call(nr=4, qnodes=(p,) * 4, tris=(p,) * 4, roots=(0,) * 4, depths=(47,) * 4, verts=(p,) * 4,
                              nv=(1,) * 4, faces=(p,) * 4, nf=(1,) * 4) == ERR_UNSUPPORTED
    for nr in (0, -1, 5):
        assert call(nr=nr) == ERR_ARG
    for name in ("qnodes", "tris", "roots", "frames", "depths", "verts", "nv", "faces", "nf"):
        assert call(drop=name) == ERR_ARG, name
    assert call(qnodes=(p, None)) == ERR_ARG and call(tris=(None, p)) == ERR_ARG
    assert call(verts=(p, None)) == ERR_ARG and call(faces=(None, p)) == ERR_ARG
    assert call(nv=(5, 0)) == ERR_ARG and call(nf=(0, 5)) == ERR_ARG
    assert call(roots=(0, -1)) == ERR_ARG and call(depths=(10, 48)) == ERR_ARG
    assert L.vsa_simplify_guarded_workspace_bytes(0, 10) == ERR_ARG
    assert L.vsa_simplify_guarded_workspace_bytes(10, 0) == ERR_ARG


# ------------------------------------------------------------------------------------------------------- GPU

def _mesh(v, f, device="cuda"):
    from volsurfs_amd.mesh import TensorMesh
    return TensorMesh(np.asarray(v, np.float32), np.asarray(f, np.int32), None, device=device)


def _assert_bits(mesh, V, F, what=""):
    assert torch.equal(mesh.faces.cpu(), torch.from_numpy(np.asarray(F, np.int32))), what
    assert torch.equal(mesh.vertices.cpu().view(torch.int32), torch.from_numpy(np.asarray(V, np.float32)).view(torch.int32)), what


def _same(a, b):
    return torch.equal(a.faces, b.faces) and torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))


@gpu
def test_python_argument_errors_before_any_hip_call():
    good = [_mesh(*m) for m in _stack("G1")]
    from volsurfs_amd.mesh import TensorMesh
    empty = TensorMesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None, device="cuda")
    with pytest.raises(ValueError):
        smp.simplify_shells(good[:1])
    with pytest.raises(ValueError):
        smp.simplify_shells([])
    with pytest.raises(ValueError):
        smp.simplify_shells([good[0], empty, good[2]])
    with pytest.raises(ValueError):
        smp.simplify_shells([good[0], _mesh(*_stack("G1")[1], device="cpu")])
    for kw in (dict(anchor=3), dict(anchor=-1), dict(builder="none"), dict(sign="none"),
               dict(target_nr_faces_ratio=0.0), dict(target_nr_faces_ratio=1.5)):
        with pytest.raises(ValueError):
            smp.simplify_shells(good, **kw)
    with pytest.raises(ValueError):
        smp.simplify_mesh(good[0], 0.5, guards=[good[1]] * 5)
    with pytest.raises(ValueError):
        smp.simplify_mesh(good[0], 0.5, guards=[empty])
    with pytest.raises(ValueError):
        smp.simplify_mesh(good[0], 0.5, guards=[_mesh(*_stack("G1")[1], device="cpu")])
    with pytest.raises(TypeError):
        smp.simplify_mesh(good[0], 0.5, guards=[(1, 2)])
    with pytest.raises(ValueError):
        smp.simplify_mesh(good[0], 0.0, guards=[good[1]])


@gpu
@pytest.mark.parametrize("anchor", [None, 0])
@pytest.mark.parametrize("builder", ["host", "device", "ploc"])
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_stack_equals_restatement(name, builder, anchor):
    ref_out, ref_reports, cin, cout = _restated_stack(name, anchor)
    meshes = [_mesh(*m) for m in _stack(name)]
    out, reports = smp.simplify_shells(meshes, sgr.G_RATIO, anchor=anchor, builder=builder)
    again, reports2 = smp.simplify_shells(meshes, sgr.G_RATIO, anchor=anchor, builder=builder)
    assert len(out) == len(reports) == 3
    for k in range(3):
        _assert_bits(out[k], *ref_out[k], (name, builder, anchor, k))
        assert _same(out[k], again[k])
        assert not out[k].has_uvs
        assert isinstance(reports[k], smp.ShellSimplifyReport)
        for field in sgr.REPORT_FIELDS:
            assert getattr(reports[k], field) == ref_reports[k][field], (k, field)
    assert list(reports) == list(reports2)
    assert reports.crossings_in == cin == [0, 0] and reports.crossings_out == cout == [0, 0]
    assert reports.nested == [True, True]


@functools.lru_cache(maxsize=None)
def _open_case():
    """test_simplify's open mesh (a marching-cubes sphere of radius 0.5 cut at |x| <= 0.3) inside the G1 outer shell
    scaled to enclose it, restated at ratio 0.1."""
    V, F = MESHES["open_mc"]()
    gv, gf = _stack("G1")[2]
    guard = ((gv * np.float32(OPEN_GUARD_SCALE)).astype(np.float32), gf)
    return (V, F), guard, sgr.restate(V, F, 0.1, [guard])


OPEN_GUARD_SCALE = 1.25


@gpu
def test_open_mesh_equals_restatement():
    from volsurfs_amd.raytrace import RayTracer
    (V, F), guard, (rv, rf, rst) = _open_case()
    assert sgr.crossing_pairs((V, F), guard) == 0 and rst["guard_rejected"] > 0, "the guard must bite and not cross"
    for g in (_mesh(*guard), (RayTracer([_mesh(*guard)], builder="ploc"), 0)):
        got, st = smp.simplify_mesh(_mesh(V, F), 0.1, return_stats=True, guards=[g])
        _assert_bits(got, rv, rf)
        assert {k: st[k] for k in rst} == rst and st["faces_in"] == len(F)
    _check_valid(rv, rf, None, _boundary_loops(F))
    assert sgr.crossing_pairs((rv, rf), guard) == 0


@gpu
@pytest.mark.parametrize("name", ["ico3", "torus", "open_mc"])
def test_far_guard_equals_plain(name):
    V, F = MESHES[name]()
    far = _mesh(*_far())
    for ratio in (0.5, 0.1, 0.025):
        plain, pst = smp.simplify_mesh(_mesh(V, F), ratio, return_stats=True)
        got, st = smp.simplify_mesh(_mesh(V, F), ratio, return_stats=True, guards=[far, far])
        assert _same(got, plain), (name, ratio)
        assert st.pop("guard_rejected") == 0 and st == pst


@gpu
def test_no_guards_is_the_old_entry_point():
    V, F, st = _plain("ico3", 0.1)
    for guards in (None, []):
        _lib.kernel_events = {}
        try:
            got, gst = smp.simplify_mesh(_mesh(*MESHES["ico3"]()), 0.1, return_stats=True, guards=guards)
            called = set(_lib.kernel_events)
        finally:
            _lib.kernel_events = None
        assert called == {"vsa_simplify"}
        _assert_bits(got, V, F)
        assert "guard_rejected" not in gst and {k: gst[k] for k in st} == st


@gpu
def test_degenerate_guard_faces_change_nothing():
    """A guard with a NaN vertex, faces with an index out of range and a zero-area face gives what the same guard
    without those faces gives.  The tree handed to the entry point is built over a finite, in-range stand-in of the same
    face count (what a tree builder makes of a NaN or of an index out of range is specified nowhere, and the faces in
    question cross nothing wherever their boxes lie); the guard's vertex and face arrays are the degenerate ones."""
    from volsurfs_amd.raytrace import RayTracer
    (V, F), (gv, gf), _ = _open_case()
    nan_vertex = 7
    at_nan = (gf == nan_vertex).any(1)
    extra = np.array([[len(gv), 0, 1], [2, -1, 3], [5, 5, 5]], np.int32)
    clean = (gv, gf[~at_nan])
    bad_v = gv.copy()
    bad_v[nan_vertex, 2] = np.nan
    bad_f = np.concatenate([gf[:100], extra, gf[100:]]).astype(np.int32)
    stand_in = np.concatenate([gf[:100], [[0, 0, 0]] * 3, gf[100:]]).astype(np.int32)
    want, wst = smp.simplify_mesh(_mesh(V, F), 0.1, return_stats=True, guards=[_mesh(*clean)])
    assert wst["guard_rejected"] > 0
    ref = sgr.restate(V, F, 0.1, [(bad_v, bad_f)])
    tracer = RayTracer([_mesh(gv, stand_in)], builder="device")
    tracer._meshes[0] = _mesh(bad_v, bad_f)
    got, st = smp.simplify_mesh(_mesh(V, F), 0.1, return_stats=True, guards=[(tracer, 0)])
    torch.cuda.synchronize()
    assert _same(got, want) and st == wst
    _assert_bits(got, ref[0], ref[1])
    assert st["guard_rejected"] == ref[2]["guard_rejected"]


def _mc_shells(levels):
    from volsurfs_amd import isosurface as iso
    n = 48
    grid = torch.from_numpy(_lobed((n, n, n))).cuda()
    return iso.marching_cubes(grid, list(levels), [-1.0] * 3, [_h(n)] * 3)


C_LEVELS, C_RATIO = (-0.04, 0.0, 0.04), 0.02
D_LEVELS, D_RATIO = (-0.01, 0.0, 0.01), 0.1


@functools.lru_cache(maxsize=None)
def _case_c():
    meshes = _mc_shells(C_LEVELS)
    return meshes, smp.simplify_shells(meshes, C_RATIO)


@gpu
def test_property_c_nested_where_the_plain_path_crosses():
    from volsurfs_amd.mesh_intersect import shell_crossings, shells_nested
    meshes, (out, reports) = _case_c()
    assert reports.crossings_in == [0, 0]
    print("C:", [tuple(r) for r in reports], reports.crossings_out, reports.nested)
    assert reports.crossings_out == [0, 0]
    assert shells_nested(out) == [True, True] and reports.nested == [True, True]
    for m, o, r in zip(meshes, out, reports):
        euler = _topology(m.vertices.cpu().numpy(), m.faces.cpu().numpy())
        _check_valid(o.vertices.cpu().numpy(), o.faces.cpu().numpy(), euler)
        assert r.faces_out == o.faces.shape[0] <= r.faces_in == m.faces.shape[0]
        assert r.target == smp.target_faces(r.faces_in, C_RATIO) and (r.stalled or r.faces_out <= r.target)
    plain = [smp.simplify_mesh(m, C_RATIO) for m in meshes]
    crossed = [c["pairs"] for c in shell_crossings(plain)]
    print("C plain:", crossed)
    assert sum(crossed) > 0, "simplifying each shell on its own must make these shells cross"


@gpu
def test_property_d_crossings_do_not_grow():
    meshes = _mc_shells(D_LEVELS)
    out, reports = smp.simplify_shells(meshes, D_RATIO)
    print("D:", [tuple(r) for r in reports], reports.crossings_in, reports.crossings_out)
    assert reports.crossings_in == [0, 16]
    assert all(o <= i for o, i in zip(reports.crossings_out, reports.crossings_in))
    assert all(r.faces_out <= r.faces_in for r in reports)


@gpu
def test_stage_on_a_directory(tmp_path):
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.mesh import load_meshes_indexed_from_path
    meshes, (want, want_reports) = _case_c()
    raw, out = str(tmp_path / "meshes"), str(tmp_path / "meshes_simplified")
    iso.save_level_sets(meshes, list(C_LEVELS), raw)
    paths, reports, check = smp.simplify_meshes_nested(raw, out, C_RATIO)
    assert sorted(os.listdir(out)) == sorted(os.listdir(raw)) and len(paths) == 3
    assert [os.path.basename(p) for p in paths] == [f"{round(lv, 4)}.ply" for lv in C_LEVELS]
    loaded = load_meshes_indexed_from_path(None, out)
    for w, l in zip(want, loaded):
        assert not l.has_uvs and _same(w, l)
    assert list(reports) == list(want_reports)
    assert [c["pairs"] for c in check["crossings"]] == reports.crossings_out == want_reports.crossings_out
    assert check["self_crossings"] == [r.self_crossings for r in reports]
    assert check["nested"] == reports.nested
