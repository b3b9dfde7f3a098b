"""Mesh smoothing on the device (volsurfs_amd/mesh_smooth.py, csrc/mesh_smooth.hip) against the restated rule
(tests/mesh_smooth_restated.py: numpy, in the device's operation order).  The reference has no such stage.  Every
comparison with the restatement is exact equality: the vertices' bits and every report field."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import mesh_intersect_restated as X
import mesh_smooth_restated as M
import shell_untangle_restated as R
from volsurfs_amd import _lib

ERR_ARG, ERR_UNSUPPORTED = -1, -2
gpu = pytest.mark.gpu
BUILDERS = ["host", "device", "ploc"]
STACK_S = dict(subdiv=2, K=3, amp=0.06, gap=0.045)


@functools.lru_cache(maxsize=None)
def _stack(name):
    stack = R.lobed_stack(**{"S": STACK_S, "A": R.STACK_A, "B": R.STACK_B}[name])
    for v, f in stack:
        v.setflags(write=False)
        f.setflags(write=False)
    return stack


@functools.lru_cache(maxsize=None)
def _mesh_of(name):
    v, f = {"sphere": M.noisy_sphere, "open": M.open_mesh, "fan": M.fan, "triangle": _triangle, "loose": _loose,
            "nan": _nan}[name]()
    v.setflags(write=False)
    return v, f


def _triangle():
    return np.array([[0, 0, 0], [1, 0, 0], [0.2, 0.9, 0.3]], np.float32), np.array([[0, 1, 2]], np.int32)


def _loose():
    """The noisy sphere with a vertex no face names."""
    v, f = M.noisy_sphere()
    return np.concatenate([v, [[0.1, 0.2, 0.3]]]).astype(np.float32), f


NAN_VERTEX = 17


def _nan():
    v, f = M.noisy_sphere()
    v = v.copy()
    v[NAN_VERTEX, 1] = np.nan
    return v, f


@functools.lru_cache(maxsize=None)
def _ref(name, **kw):
    """The restated answer for one mesh: (vertices, report, log).  Computed once, shared, never written to."""
    v, rep, log = M.restate(*_mesh_of(name), **kw)
    v.setflags(write=False)
    return v, rep, log


@functools.lru_cache(maxsize=None)
def _ref_middle(name, guarded):
    stack = _stack(name)
    v, rep, log = M.restate(*stack[1], guards=(stack[0], stack[2]) if guarded else ())
    v.setflags(write=False)
    return v, rep, log


@functools.lru_cache(maxsize=None)
def _ref_shells(name, anchor=None):
    out, reports, stack = M.restate_shells(_stack(name), anchor=anchor)
    for v in out:
        v.setflags(write=False)
    return out, reports, stack


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _pairs_with_neighbours(v, name):
    stack = _stack(name)
    return [M.crossing_pairs(*stack[0], v, stack[1][1]), M.crossing_pairs(v, stack[1][1], *stack[2])]


# ---------------------------------------------------------------------------------------------------------- CPU

def test_entry_points_declared_built_and_prototyped():
    import volsurfs_amd
    from volsurfs_amd import mesh_smooth
    names, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    P, I, LL, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    expected = {
        "vsa_mesh_smooth_workspace_bytes": (LL, [LL, LL]),
        "vsa_mesh_smooth_prepare": (I, [P, LL, LL, P, LL, P]),
        "vsa_mesh_smooth_step": (I, [P, P, P, LL, LL, I, F, I, P, LL, P, P]),
        "vsa_mesh_smooth_guard": (I, [P, P, P, LL, LL, I, P, P, P, P, P, P, P, P, P, I, I, P, LL, P]),
        "vsa_mesh_smooth_revert": (I, [P, P, LL, LL, I, P, LL, P, P]),
    }
    for n, proto in expected.items():
        assert n in names, f"{n} is not declared in include/volsurfs_hip.h"
        assert hasattr(cdll, n), f"{n} is not in the built library"
        assert protos.get(n) == proto, n
    for n in ("smooth_mesh", "smooth_shells", "smooth_meshes", "SmoothReport"):
        assert n in mesh_smooth.__all__ and n in volsurfs_amd.__all__
        assert getattr(volsurfs_amd, n) is getattr(mesh_smooth, n)
    assert mesh_smooth.SmoothReport._fields == M.FIELDS


def test_entry_point_argument_errors_before_any_hip_call():
    """Every VSA_ERR_ARG case of the entry points.  The "device" pointers are null or the address of a host buffer
    nothing reads: each call must return before it touches the GPU (this test runs without one).  The calls whose
    arguments are all good name a mesh of 2^32 vertices: they get as far as the size check and return
    VSA_ERR_UNSUPPORTED, still before any HIP call."""
    L = _lib.lib()
    buf = (ctypes.c_longlong * 16)()
    p, q = ctypes.addressof(buf), ctypes.addressof(buf) + 64
    HUGE = 1 << 32

    def prepare(faces=p, nv=100, nf=10, ws=p, ws_bytes=8):
        return L.vsa_mesh_smooth_prepare(faces, nv, nf, ws, ws_bytes, None)

    def step(src=p, dst=q, faces=p, nv=100, nf=10, half=0, w=0.5, fixed=1, ws=p, ws_bytes=8, state=p):
        return L.vsa_mesh_smooth_step(src, dst, faces, nv, nf, half, w, fixed, ws, ws_bytes, state, None)

    def revert(before=p, after=q, nv=100, nf=10, rnd=0, ws=p, ws_bytes=8, state=p):
        return L.vsa_mesh_smooth_revert(before, after, nv, nf, rnd, ws, ws_bytes, state, None)

    def guard(before=p, after=q, mfaces=p, mv=100, mf=10, nr=2, qnodes=(p, p), tris=(p, p), roots=(0, 0), depths=(10, 10),
              verts=(p, p), nv=(5, 5), faces=(p, p), nf=(5, 5), first=0, rnd=0, ws=p, ws_bytes=8, drop=None):
        ptrs = lambda xs: (ctypes.c_void_p * 4)(*xs)
        args = {"qnodes": ptrs(qnodes), "tris": ptrs(tris), "roots": (ctypes.c_int32 * 4)(*roots),
                "frames": (ctypes.c_float * 24)(*([0, 0, 0, 1, 1, 1] * 4)), "depths": (ctypes.c_int32 * 4)(*depths),
                "verts": ptrs(verts), "nv": (ctypes.c_longlong * 4)(*nv), "faces": ptrs(faces),
                "nf": (ctypes.c_longlong * 4)(*nf)}
        if drop:
            args[drop] = None
        return L.vsa_mesh_smooth_guard(before, after, mfaces, mv, mf, nr, args["qnodes"], args["tris"], args["roots"],
                                       args["frames"], args["depths"], args["verts"], args["nv"], args["faces"],
                                       args["nf"], first, rnd, ws, ws_bytes, None)

    # good arguments, a mesh too large: past every argument check
    assert prepare(nv=HUGE) == step(nv=HUGE) == revert(nv=HUGE) == guard(mv=HUGE) == ERR_UNSUPPORTED
    assert step(nv=HUGE, half=1, w=-0.53) == step(nv=HUGE, half=1, w=0.0) == step(nv=HUGE, w=1.0) == ERR_UNSUPPORTED
    assert guard(mv=HUGE, first=4, rnd=6) == ERR_UNSUPPORTED
    assert guard(mv=HUGE, nr=1) == guard(mv=HUGE, nr=4, qnodes=(p,) * 4, tris=(p,) * 4, roots=(0,) * 4,
                                         depths=(47,) * 4, verts=(p,) * 4, nv=(1,) * 4, faces=(p,) * 4,
                                         nf=(1,) * 4) == ERR_UNSUPPORTED
    # a workspace that is too small (8 bytes), with everything else good
    assert prepare() == step() == revert() == guard() == ERR_ARG
    for kw in ({"faces": None}, {"ws": None}, {"nv": 0}, {"nv": -3}, {"nf": 0}, {"nf": -1}):
        assert prepare(**dict(kw, ws_bytes=1 << 40)) == ERR_ARG, kw
    nan, inf = float("nan"), float("inf")
    for kw in ({"src": None}, {"dst": None}, {"dst": p}, {"faces": None}, {"ws": None}, {"state": None}, {"nv": 0},
               {"nf": 0}, {"w": 0.0}, {"w": -0.5}, {"w": 1.5}, {"w": nan}, {"w": inf}, {"half": 1, "w": 0.1},
               {"half": 1, "w": nan}, {"half": 1, "w": -inf}, {"half": 2, "w": 0.5}, {"half": -1, "w": 0.5}):
        assert step(**dict({"nv": HUGE}, **kw)) == ERR_ARG, kw
    for kw in ({"before": None}, {"after": None}, {"ws": None}, {"state": None}, {"nv": 0}, {"nf": 0}, {"rnd": -1}):
        assert revert(**dict({"nv": HUGE}, **kw)) == ERR_ARG, kw
    for kw in ({"before": None}, {"after": None}, {"mfaces": None}, {"ws": None}, {"mv": 0}, {"mf": 0}, {"rnd": -1},
               {"first": -1}, {"first": 3, "rnd": 2},
               {"nr": 0}, {"nr": -1}, {"nr": 5}, {"roots": (0, -1)}, {"depths": (10, 48)}, {"depths": (99, 10)},
               {"qnodes": (p, None)}, {"tris": (None, p)}, {"verts": (p, None)}, {"faces": (None, p)}, {"nv": (5, 0)},
               {"nf": (0, 5)}):
        assert guard(**dict({"mv": HUGE}, **kw)) == ERR_ARG, kw
    for name in ("qnodes", "tris", "roots", "frames", "depths", "verts", "nv", "faces", "nf"):
        assert guard(mv=HUGE, drop=name) == ERR_ARG, name
    for v, f in ((0, 5), (5, 0), (-1, 5)):
        assert L.vsa_mesh_smooth_workspace_bytes(v, f) == ERR_ARG
    assert L.vsa_mesh_smooth_workspace_bytes(HUGE, 5) == ERR_UNSUPPORTED


def test_python_argument_errors_before_any_hip_call():
    from volsurfs_amd.mesh import TensorMesh, icosphere
    from volsurfs_amd.mesh_smooth import smooth_mesh, smooth_shells
    shells = [TensorMesh(*icosphere(1, r), device="cpu") for r in (0.5, 0.6, 0.7)]
    rule = [dict(iterations=-1), dict(iterations=2.0), dict(iterations="3"), dict(iterations=True), dict(lam=0.0),
            dict(lam=-0.5), dict(lam=1.5), dict(lam=float("nan")), dict(mu=0.1), dict(mu=float("nan")),
            dict(mu=float("-inf")), dict()]                      # (the last: every argument fine, the meshes on the CPU)
    for kw in rule + [dict(meshes=shells[:1]), dict(meshes=[]), dict(anchor=3), dict(anchor=-1), dict(builder="sah")]:
        kw = dict(kw)
        meshes = kw.pop("meshes", shells)
        with pytest.raises(ValueError):
            smooth_shells(meshes, **kw)
    for kw in rule + [dict(guards=shells[:1]), dict(guards=[shells[1]] * 5)]:
        with pytest.raises(ValueError):
            smooth_mesh(shells[0], **kw)


def test_restatement_noisy_sphere():
    v, f = _mesh_of("sphere")
    assert v.shape == (642, 3) and f.shape == (1280, 3) and v.dtype == np.float32
    mean0, std0 = M.radius_stats(v)
    out, rep, _ = _ref("sphere")
    mean1, std1 = M.radius_stats(out)
    print("radius mean, std:", (mean0, std0), "->", (mean1, std1))
    assert std1 < 0.5 * std0 and abs(mean1 - mean0) < 0.01 * mean0
    assert (round(std0, 6), round(std1, 6), round(mean0, 6), round(mean1, 6)) == (0.011434, 0.003984, 0.500807, 0.502310)
    assert rep["moved_vertices"] == 642 and rep["boundary_vertices"] == rep["stuck"] == rep["self_crossings_after"] == 0
    laplace, _, _ = _ref("sphere", mu=0.0)                         # what mu is for: without it the sphere shrinks
    mean2, _ = M.radius_stats(laplace)
    print("mu = 0:", mean2)
    assert mean2 < 0.96 * mean0 and round(mean2, 6) == 0.473192
    same, rep0, _ = _ref("sphere", iterations=0)
    assert np.array_equal(_bits(same), _bits(v)) and rep0["moved_vertices"] == 0 and rep0["max_displacement"] == 0.0


def test_restatement_ring_order_is_the_corner_slots():
    """The ring of `topology` against the rule's words, slot by slot, on a mesh with a face that names a vertex twice."""
    f = np.array([[0, 1, 2], [2, 1, 3], [3, 3, 0], [1, 0, 3]], np.int32)
    topo = M.topology(f, 5)
    for v in range(5):
        slots = [(i, c) for i in range(len(f)) for c in range(3) if f[i, c] == v]
        sel = topo["v"] == v
        assert topo["slots"][v] == len(slots) and topo["rank"][sel].tolist() == list(range(len(slots)))
        assert topo["a"][sel].tolist() == [f[i, (c + 1) % 3] for i, c in slots]
        assert topo["b"][sel].tolist() == [f[i, (c + 2) % 3] for i, c in slots]
    # the keys: 01 x 2, 12 x 2, 13 x 2, 03 x 3; once each: 02, 23 and the edge 33 of the face that names 3 twice
    assert topo["slots"][4] == 0 and topo["boundary"].tolist() == [True, False, True, True, False]


def test_restatement_open_mesh_boundary():
    v, f = _mesh_of("open")
    assert 0 < len(f) < 1280
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    uniq, count = np.unique(edges, axis=0, return_counts=True)
    boundary = np.zeros(len(v), bool)
    boundary[uniq[count == 1].reshape(-1)] = True
    assert boundary.sum() > 10
    fixed, rep, _ = _ref("open")
    assert rep["boundary_vertices"] == int(boundary.sum())
    assert np.array_equal(_bits(fixed)[boundary], _bits(v)[boundary])
    used = np.zeros(len(v), bool)
    used[f.reshape(-1)] = True
    assert (_bits(fixed) != _bits(v)).any(1)[used & ~boundary].all() and rep["moved_vertices"] == (used & ~boundary).sum()
    free, rep, _ = _ref("open", fix_boundary=False)
    assert rep["boundary_vertices"] == int(boundary.sum()) and (_bits(free) != _bits(v)).any(1)[boundary].all()


def test_restatement_stack_s():
    stack = _stack("S")
    assert stack[1][0].shape == (162, 3) and stack[1][1].shape == (320, 3)
    assert [len(M.crossing_pairs(*stack[k], *stack[k + 1])) for k in range(2)] == [0, 0]
    plain, _, _ = _ref_middle("S", False)
    assert [len(p) for p in _pairs_with_neighbours(plain, "S")] == [48, 0]
    guarded, rep, log = _ref_middle("S", True)
    assert [len(p) for p in _pairs_with_neighbours(guarded, "S")] == [0, 0]
    assert [r for r, _ in log] == [6, 6, 6, 8, 18, 18, 18, 12, 12, 6] and [n for _, n in log] == [2] * 10
    assert rep["moved_vertices"] == 162 and rep["self_crossings_after"] == 0
    assert rep["reverted"] == 110 and rep["guard_rounds"] == 20


def test_restatement_box_filter_equals_brute_force():
    """The filtered pair sets and counts of the restatement against `mesh_intersect_restated`'s brute force."""
    stack = _stack("A")
    for k in range(2):
        brute = X.mesh_crossings(*stack[k], *stack[k + 1])["pairs"]
        assert M.crossing_pairs(*stack[k], *stack[k + 1]) == {tuple(p) for p in brute.tolist()}
    plain, _, _ = _ref_middle("S", False)
    f = _stack("S")[1][1]
    assert len(X.mesh_crossings(*_stack("S")[0], plain, f)["pairs"]) == 48
    pinched = plain.copy()
    pinched[5] = pinched[5] * np.float32(-1.5)                     # a vertex pulled out through the far side
    assert M.self_crossing_count(pinched, f) == len(X.self_crossings(pinched, f)["pairs"]) > 0


def test_restatement_stack_a_keeps_its_crossings():
    stack = _stack("A")
    before = [M.crossing_pairs(*stack[k], *stack[k + 1]) for k in range(2)]
    assert [len(p) for p in before] == [48, 44]
    out, rep, _ = _ref_middle("A", True)
    after = _pairs_with_neighbours(out, "A")
    assert [len(p) for p in after] == [48, 44] and after[0] <= before[0] and after[1] <= before[1]
    assert rep["moved_vertices"] > 0 and rep["reverted"] > 0


def test_restatement_shells_s():
    out, reports, stack = _ref_shells("S")
    assert stack == {"crossings_in": [0, 0], "crossings_out": [0, 0], "nested": [True, True]}
    assert [r["guards"] for r in reports] == [(("out", 1),), (("in", 0), ("in", 2)), (("out", 1),)]
    assert all(set(r) == set(M.FIELDS) for r in reports) and np.array_equal(_bits(out[1]), _bits(_ref_middle("S", True)[0]))


def test_restatement_loose_and_nan_vertices():
    v, f = _mesh_of("loose")
    out, rep, _ = _ref("loose", iterations=2)
    assert np.array_equal(_bits(out[-1]), _bits(v[-1])) and rep["moved_vertices"] == 642
    assert np.array_equal(_bits(out[:-1]), _bits(M.restate(*_mesh_of("sphere"), iterations=2)[0]))
    v, f = _mesh_of("nan")
    ring = np.unique(f[(f == NAN_VERTEX).any(1)])
    around = ring[ring != NAN_VERTEX]
    assert len(around) in (5, 6)
    out, rep, _ = _ref("nan", iterations=2)
    assert np.array_equal(_bits(out[ring]), _bits(v[ring]))        # the NaN does not spread: its ring stays, it stays
    assert rep["stuck"] == 4 * len(ring) and rep["self_crossings_after"] is None
    assert rep["moved_vertices"] == 642 - len(ring) and np.isfinite(np.delete(out, NAN_VERTEX, 0)).all()


# ---------------------------------------------------------------------------------------------------------- GPU

def _mesh(v, f):
    from volsurfs_amd.mesh import TensorMesh
    return TensorMesh(np.array(v, np.float32), np.array(f, np.int32), device="cuda")


def _assert_report(rep, ref, shell=0, guards=(), what=""):
    ref = dict({"shell": shell, "guards": tuple(guards)}, **ref)
    for field in M.FIELDS:
        assert getattr(rep, field) == ref[field], (what, field, getattr(rep, field), ref[field])


def _assert_mesh_equal(name, **kw):
    return _assert_arrays_equal(*_mesh_of(name), _ref(name, **kw), name, **kw)


def _assert_arrays_equal(v, f, ref, name, **kw):
    from volsurfs_amd.mesh_smooth import smooth_mesh
    ref_v, ref, ref_log = ref
    log = []
    out, rep = smooth_mesh(_mesh(v, f), log=log, **kw)
    assert np.array_equal(_bits(out.vertices.cpu().numpy()), _bits(ref_v)), (name, kw)
    _assert_report(rep, ref, what=(name, kw))
    assert log == ref_log and np.array_equal(out.faces.cpu().numpy(), f)
    return out, rep


@gpu
@pytest.mark.parametrize("iterations", [0, 1, 10])
def test_noisy_sphere_equals_the_restatement(iterations):
    out, rep = _assert_mesh_equal("sphere", iterations=iterations)
    if iterations == 0:
        assert np.array_equal(_bits(out.vertices.cpu().numpy()), _bits(_mesh_of("sphere")[0])) and rep.moved_vertices == 0


@gpu
@pytest.mark.parametrize("fix_boundary", [True, False])
def test_open_mesh_equals_the_restatement(fix_boundary):
    _, rep = _assert_mesh_equal("open", fix_boundary=fix_boundary)
    assert rep.boundary_vertices > 10


@gpu
@pytest.mark.parametrize("name,kw", [("fan", dict(fix_boundary=False)), ("fan", dict()), ("triangle", dict()),
                                     ("triangle", dict(fix_boundary=False, iterations=3)),
                                     ("loose", dict(iterations=2)), ("nan", dict(iterations=2)),
                                     ("sphere", dict(mu=0.0)), ("sphere", dict(lam=1.0, mu=-1.0, iterations=3))])
def test_small_and_degenerate_meshes_equal_the_restatement(name, kw):
    out, rep = _assert_mesh_equal(name, **kw)
    if name == "fan" and not kw.get("fix_boundary", True):
        assert rep.moved_vertices == 201                            # the apex' ring of 200 slots: longer than a wave
    if name == "nan":
        assert rep.stuck > 0 and rep.self_crossings_after is None


@gpu
def test_guards_as_meshes_and_as_tracer_pairs_for_every_builder():
    from volsurfs_amd.mesh_smooth import smooth_mesh
    from volsurfs_amd.raytrace import RayTracer
    stack = _stack("S")
    ref_v, ref, ref_log = _ref_middle("S", True)
    runs = [("meshes", [_mesh(*stack[0]), _mesh(*stack[2])])]
    for builder in BUILDERS:
        tracer = RayTracer([_mesh(*m) for m in stack], builder=builder)
        runs.append((builder, [(tracer, 0), (tracer, 2)]))
    for what, guards in runs:
        log = []
        out, rep = smooth_mesh(_mesh(*stack[1]), guards=guards, log=log)
        assert np.array_equal(_bits(out.vertices.cpu().numpy()), _bits(ref_v)), what
        _assert_report(rep, ref, guards=(("guard", 0), ("guard", 1)), what=what)
        assert log == ref_log, what
    plain_v, plain, _ = _ref_middle("S", False)
    for guards in (None, []):
        out, rep = smooth_mesh(_mesh(*stack[1]), guards=guards)
        assert np.array_equal(_bits(out.vertices.cpu().numpy()), _bits(plain_v))
        _assert_report(rep, plain, what=guards)


@gpu
def test_one_guard_and_a_crossing_input():
    """Stack A crosses already: the guarded middle shell keeps exactly the crossings it had.  One guard alone, too."""
    from volsurfs_amd.mesh_smooth import smooth_mesh
    stack = _stack("A")
    ref_v, ref, ref_log = _ref_middle("A", True)
    log = []
    out, rep = smooth_mesh(_mesh(*stack[1]), guards=[_mesh(*stack[0]), _mesh(*stack[2])], log=log)
    assert np.array_equal(_bits(out.vertices.cpu().numpy()), _bits(ref_v)) and log == ref_log
    _assert_report(rep, ref, guards=(("guard", 0), ("guard", 1)))
    stack = _stack("S")
    one_v, one, one_log = M.restate(*stack[1], iterations=4, guards=(stack[0],))
    log = []
    out, rep = smooth_mesh(_mesh(*stack[1]), iterations=4, guards=[_mesh(*stack[0])], log=log)
    assert np.array_equal(_bits(out.vertices.cpu().numpy()), _bits(one_v)) and log == one_log
    _assert_report(rep, one, guards=(("guard", 0),))


@gpu
@pytest.mark.parametrize("name,anchor,builder", [("S", None, "device"), ("S", 0, "host"), ("B", None, "device"),
                                                 ("B", 4, "ploc")])
def test_stacks_equal_the_restatement(name, anchor, builder):
    from volsurfs_amd.mesh_smooth import smooth_shells
    stack = _stack(name)
    ref_v, ref_reports, ref_stack = _ref_shells(name, anchor)
    out, reports = smooth_shells([_mesh(*m) for m in stack], anchor=anchor, builder=builder)
    for k, (m, rep) in enumerate(zip(out, reports)):
        assert np.array_equal(_bits(m.vertices.cpu().numpy()), _bits(ref_v[k])), (name, anchor, k)
        _assert_report(rep, ref_reports[k], k, ref_reports[k]["guards"], (name, anchor, k))
        assert m.faces.dtype == torch.int32 and np.array_equal(m.faces.cpu().numpy(), stack[k][1])
    assert reports.crossings_in == ref_stack["crossings_in"] and reports.crossings_out == ref_stack["crossings_out"]
    assert reports.nested == ref_stack["nested"]
    assert all(o <= i for o, i in zip(reports.crossings_out, reports.crossings_in))


@gpu
def test_determinism_and_what_is_carried_over():
    from volsurfs_amd.mesh_smooth import smooth_mesh
    stack = _stack("S")
    rng = np.random.default_rng(3)
    mesh = _mesh(*stack[1])
    mesh.faces_uvs = torch.from_numpy(rng.random((320, 3, 2), dtype=np.float32)).cuda()
    mesh.has_uvs = True
    mesh.vertex_colors = torch.from_numpy(rng.random((162, 3), dtype=np.float32)).cuda()
    kept = [t.clone() for t in (mesh.vertices, mesh.faces, mesh.faces_uvs, mesh.vertex_colors)]
    guards = [_mesh(*stack[0]), _mesh(*stack[2])]
    runs = [smooth_mesh(mesh, guards=guards) for _ in range(2)]
    assert runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][0].vertices.view(torch.int32), runs[1][0].vertices.view(torch.int32))
    for t, k in zip((mesh.vertices, mesh.faces, mesh.faces_uvs, mesh.vertex_colors), kept):
        assert torch.equal(t, k)                                  # the input is not written
    out = runs[0][0]
    assert out.vertices.data_ptr() != mesh.vertices.data_ptr() and out.has_uvs is True
    assert torch.equal(out.faces, mesh.faces) and torch.equal(out.faces_uvs, mesh.faces_uvs)
    assert torch.equal(out.vertex_colors, mesh.vertex_colors)
    same, _ = smooth_mesh(mesh, iterations=0)
    assert torch.equal(same.vertices.view(torch.int32), mesh.vertices.view(torch.int32))
    assert same.vertices.data_ptr() != mesh.vertices.data_ptr()


@gpu
def test_stage(tmp_path):
    """`smooth_meshes` on stack S written as an OBJ with per-corner UVs, a binary PLY with colours and an ascii PLY:
    names and formats kept, UVs, colours and faces byte-equal, the vertices `smooth_shells`' (the restatement's), and
    the second return value `check_shells(out_dir)`."""
    from volsurfs_amd.mesh import load_obj, load_ply, save_obj, save_ply
    from volsurfs_amd.mesh_intersect import check_shells
    from volsurfs_amd.mesh_smooth import smooth_meshes
    stack = _stack("S")
    names = ["-0.01.obj", "0.0.ply", "0.01.ply"]
    rng = np.random.default_rng(5)
    src, dst = tmp_path / "meshes", tmp_path / "meshes_smooth"
    src.mkdir()
    for name, (v, f) in zip(names, stack):
        m = _mesh(v, f)
        m.faces_uvs = torch.from_numpy(rng.random((len(f), 3, 2), dtype=np.float32)).cuda()
        if name.endswith(".obj"):
            save_obj(str(src / name), m)
        else:
            colors = rng.integers(0, 256, (len(v), 3)).astype(np.float32) / 255.0 if name == "0.0.ply" else None
            save_ply(str(src / name), m, binary=name == "0.0.ply", vertex_colors=colors)
    reports, check = smooth_meshes(str(src), str(dst))
    assert sorted(os.listdir(dst)) == sorted(os.listdir(src)) == sorted(names)
    assert check == check_shells(str(dst))
    assert [os.path.basename(p) for p in check["files"]] == names
    assert check["nested"] == [True, True] == reports.nested and check["self_crossings"] == [0] * 3
    assert [e["pairs"] for e in check["crossings"]] == [0, 0] == reports.crossings_out
    ref_v, ref_reports, _ = _ref_shells("S")
    for k, name in enumerate(names):
        _assert_report(reports[k], ref_reports[k], k, ref_reports[k]["guards"], name)
        a, b = str(src / name), str(dst / name)
        if name.endswith(".obj"):
            before, after = load_obj(a), load_obj(b)
        else:
            (before, c0), (after, c1) = load_ply(a, return_colors=True), load_ply(b, return_colors=True)
            assert (c0 is None) == (c1 is None) == (name != "0.0.ply") and (c0 is None or torch.equal(c0, c1))
            with open(a, "rb") as fa, open(b, "rb") as fb:
                assert fa.read(40).split(b"\n")[1] == fb.read(40).split(b"\n")[1]           # ascii stays ascii
        assert torch.equal(before.faces, after.faces) and after.has_uvs
        assert torch.equal(before.faces_uvs.view(torch.int32), after.faces_uvs.view(torch.int32))
        assert np.array_equal(_bits(after.vertices.cpu().numpy()), _bits(ref_v[k])), name


def _mc_field():
    """A 32^3 lobed field with additive noise, negative inside: its zero set is a bumpy closed surface inside the grid."""
    n = 32
    x = (np.arange(n, dtype=np.float64) + 0.5) / n - 0.5
    X3, Y3, Z3 = np.meshgrid(x, x, x, indexing="ij")
    r = np.sqrt(X3 * X3 + Y3 * Y3 + Z3 * Z3)
    lobes = 0.05 * np.sin(3.0 * np.arctan2(Y3, X3)) * np.sin(3.0 * np.arccos(np.clip(Z3 / np.maximum(r, 1e-9), -1, 1)))
    noise = np.random.default_rng(7).uniform(-0.012, 0.012, (n, n, n))
    return (r - 0.3 - lobes + noise).astype(np.float32), float(x[0]), 1.0 / n


@gpu
def test_marching_cubes_mesh_equals_the_restatement():
    """Irregular valence, V not a multiple of the block: the extraction's own output, 5 iterations."""
    from volsurfs_amd.isosurface import marching_cubes
    grid, origin, spacing = _mc_field()
    mesh = marching_cubes(torch.from_numpy(grid).cuda(), 0.0, (origin,) * 3, (spacing,) * 3)[0]
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    valence = np.bincount(f.reshape(-1), minlength=len(v))
    print("marching cubes:", v.shape, f.shape, "valence", valence.min(), valence.max())
    assert len(v) > 1000 and len(v) % 256 != 0 and len(v) % 64 != 0 and valence.max() > valence.min() >= 3
    out, rep = _assert_arrays_equal(v, f, M.restate(v, f, iterations=5), "marching cubes", iterations=5)
    assert rep.moved_vertices == len(v) and rep.boundary_vertices == 0
