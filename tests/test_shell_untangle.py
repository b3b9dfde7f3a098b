"""Shell untangling on the device (volsurfs_amd/shell_untangle.py, RayTracer.untangle, csrc/shell_untangle.hip; DESIGN
§34) against the restated rule (tests/shell_untangle_restated.py: numpy, in the device's operation order).  The reference
has no such stage.  Every comparison with the restatement is exact equality: the vertices' bits and every report field."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import mesh_intersect_restated as X
import mesh_sdf_restated as S
import shell_untangle_restated as R
from volsurfs_amd import _lib
from volsurfs_amd.mesh import icosphere

ERR_ARG = -1
gpu = pytest.mark.gpu
BUILDERS = ["host", "device", "ploc"]


@functools.lru_cache(maxsize=None)
def _stack(name):
    return R.lobed_stack(**{"A": R.STACK_A, "B": R.STACK_B, "A1": dict(R.STACK_A, subdiv=1)}[name])


def _margin(name):
    return R.MARGIN_B if name == "B" else R.MARGIN_A


@functools.lru_cache(maxsize=None)
def _ref(name, anchor=None):
    """The restated answer for a stack: (vertices, reports).  Computed once, shared, never written to."""
    out, reports = R.untangle_shells(_stack(name), anchor=anchor, margin=_margin(name))
    for v in out:
        v.setflags(write=False)
    return out, reports


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------- CPU

def test_entry_points_declared_built_and_prototyped():
    names, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    P, I, LL, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    expected = {
        "vsa_shell_untangle_workspace_bytes": (LL, [LL]),
        "vsa_shell_untangle_project": (I, [P, P, I, P, I, P, LL, P, LL, F, P, LL, I, F, I, I, P, LL, P, P]),
        "vsa_shell_untangle_escalate": (I, [P, P, LL, LL, I, P, LL, P]),
    }
    for n, proto in expected.items():
        assert n in names, f"{n} is not declared in include/volsurfs_hip.h"
        assert hasattr(cdll, n), f"{n} is not in the built library"
        assert protos.get(n) == proto, n


def test_entry_point_argument_errors_before_any_hip_call():
    """Every VSA_ERR_ARG case of the entry points.  The "device" pointers are null or the address of a host buffer
    nothing reads: each call must return before it touches the GPU (this test runs without one)."""
    L = _lib.lib()
    buf = (ctypes.c_longlong * 16)()
    p = ctypes.addressof(buf)
    frame = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)

    def project(qnodes=p, tris=p, root=0, frame=frame, depth=10, table=p, base=0, moments=None, mroot=0, beta=2.0,
                verts=p, nv=100, side=1, margin=1e-3, max_level=6, rnd=0, ws=p, ws_bytes=1 << 20, state=p):
        return L.vsa_shell_untangle_project(qnodes, tris, root, frame, depth, table, base, moments, mroot, beta, verts,
                                            nv, side, margin, max_level, rnd, ws, ws_bytes, state, None)

    def escalate(count=p, faces=p, nf=10, nv=100, rnd=0, ws=p, ws_bytes=1 << 20):
        return L.vsa_shell_untangle_escalate(count, faces, nf, nv, rnd, ws, ws_bytes, None)

    cases = [{n: None} for n in ("qnodes", "tris", "frame", "table", "verts", "ws", "state")]
    cases += [{"root": -1}, {"depth": 48}, {"depth": 99}, {"base": -1}, {"nv": 0}, {"nv": -5}, {"side": 0}, {"side": 2},
              {"side": -2}, {"margin": 0.0}, {"margin": -1e-3}, {"margin": float("inf")}, {"margin": float("nan")},
              {"max_level": -1}, {"max_level": 31}, {"rnd": -1}, {"ws_bytes": 8},
              {"moments": p, "mroot": -1}, {"moments": p, "beta": 1.0}, {"moments": p, "beta": float("nan")}]
    for kw in cases:
        assert project(**kw) == ERR_ARG, kw
    for kw in ({"count": None}, {"faces": None}, {"ws": None}, {"nf": 0}, {"nf": -1}, {"nv": 0}, {"rnd": -1},
               {"ws_bytes": 8}):
        assert escalate(**kw) == ERR_ARG, kw
    for n in (0, -1):
        assert L.vsa_shell_untangle_workspace_bytes(n) == ERR_ARG
    assert L.vsa_shell_untangle_workspace_bytes(100) >= 800


def test_python_argument_errors_before_any_hip_call():
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.shell_untangle import untangle_shells
    shells = [TensorMesh(*icosphere(1, r), device="cpu") for r in (0.5, 0.6, 0.7)]
    bad = [dict(meshes=shells[:1]), dict(meshes=[]), dict(anchor=3), dict(anchor=-1), dict(margin=0.0),
           dict(margin=-1.0), dict(margin=float("nan")), dict(margin=float("inf")), dict(max_rounds=0),
           dict(max_level=-1), dict(max_level=31), dict(sign="parity"), dict(beta=1.0),
           dict()]                                               # (the last: every argument fine, the meshes on the CPU)
    for kw in bad:
        kw = dict(kw)
        meshes = kw.pop("meshes", shells)
        with pytest.raises(ValueError):
            untangle_shells(meshes, **kw)


def _assert_guarantees(stack, out, reports, margin, anchor):
    K = len(stack)
    assert np.array_equal(_bits(out[anchor]), _bits(stack[anchor][0]))
    assert reports[anchor]["side"] == 0 and reports[anchor]["against"] is None
    for k in range(K):
        if k == anchor:
            continue
        rep = reports[k]
        side, against = (1, k - 1) if k > anchor else (-1, k + 1)
        assert (rep["shell"], rep["side"], rep["against"]) == (k, side, against)
        assert rep["converged"] and rep["stuck"] == 0 and rep["crossings_after"] == 0
        q = S.signed_distance(out[k], out[against], stack[against][1])
        assert (np.float32(side) * q["dist"] >= np.float32(margin)).all(), k
        assert len(X.mesh_crossings(out[k], stack[k][1], out[against], stack[against][1])["pairs"]) == 0
        moved = (_bits(out[k]) != _bits(stack[k][0])).any(1)
        assert rep["moved_vertices"] == int(moved.sum()) > 0
        d = out[k].astype(np.float64) - stack[k][0].astype(np.float64)
        assert rep["max_displacement"] == np.sqrt((d * d).sum(1)).max()


def test_restatement_stack_a():
    stack = _stack("A")
    before = [len(X.mesh_crossings(*stack[k], *stack[k + 1])["pairs"]) for k in range(2)]
    assert before == [48, 44]
    out, reports = _ref("A")
    _assert_guarantees(stack, out, reports, R.MARGIN_A, 1)
    assert [r["crossings_before"] for r in reports] == [48, 0, 44]
    assert [r["rounds"] for r in reports] == [2, 0, 4]
    assert [r["max_level"] for r in reports] == [0, 0, 2]
    assert [r["self_crossings_after"] for r in reports] == [0, 0, 0]


def test_restatement_stack_b():
    stack = _stack("B")
    before = [len(X.mesh_crossings(*stack[k], *stack[k + 1])["pairs"]) for k in range(4)]
    assert before == [90, 138, 142, 96]
    out, reports = _ref("B")
    _assert_guarantees(stack, out, reports, R.MARGIN_B, 2)
    assert max(r["rounds"] for r in reports) <= 7 and max(r["max_level"] for r in reports) == 4
    assert [r["self_crossings_after"] for r in reports] == [0] * 5
    # the pairs next to the anchor start from the input's crossings; the others from what their neighbour became
    assert reports[1]["crossings_before"] == 138 and reports[3]["crossings_before"] == 142


def test_restatement_a_vertex_that_needs_nothing_keeps_its_bits():
    stack = _stack("A")
    v, f = stack[0]
    xv, xf = stack[1]
    table = S.pseudonormal_table(xv, xf)
    new, moved, stuck, _ = R.project(v, np.zeros(len(v), np.int64), xv, xf, table, -1, R.MARGIN_A, 6)
    clear = -S.signed_distance(v, xv, xf, table)["dist"] >= np.float32(R.MARGIN_A)
    assert clear.any() and (~clear).any() and not stuck.any()
    assert np.array_equal(moved, ~clear) and np.array_equal(_bits(new)[clear], _bits(v)[clear])
    q = S.signed_distance(new[moved], xv, xf, table)              # one step: the overshoot clears the margin
    assert (-q["dist"] >= np.float32(R.MARGIN_A)).all()


# ---------------------------------------------------------------------------------------------------------- GPU

def _mesh(v, f):
    from volsurfs_amd.mesh import TensorMesh
    return TensorMesh(np.asarray(v, np.float32), np.asarray(f, np.int32), device="cuda")


def _assert_report(rep, ref, what=""):
    for field in R.FIELDS:
        assert getattr(rep, field) == ref[field], (what, field, getattr(rep, field), ref[field])


def _assert_stack_equal(out, reports, ref, what=""):
    ref_v, ref_reports = ref
    for k, (m, rep) in enumerate(zip(out, reports)):
        assert np.array_equal(_bits(m.vertices.cpu().numpy()), _bits(ref_v[k])), (what, k)
        _assert_report(rep, ref_reports[k], (what, k))


@gpu
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name,anchor", [("A", None), ("B", None), ("B", 0), ("B", 4)])
def test_stacks_equal_the_restatement(name, anchor, builder):
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.shell_untangle import untangle_shells
    stack = _stack(name)
    tracer = RayTracer([_mesh(*m) for m in stack], builder=builder)
    out, reports = untangle_shells(tracer, anchor=anchor, margin=_margin(name))
    _assert_stack_equal(out, reports, _ref(name, anchor), (name, anchor, builder))
    for m, (_, f) in zip(out, stack):
        assert m.faces.dtype == torch.int32 and np.array_equal(m.faces.cpu().numpy(), f)
    if builder == "device":                                       # a list of meshes: the tracer is built inside
        out2, reports2 = untangle_shells([_mesh(*m) for m in stack], anchor=anchor, margin=_margin(name))
        assert reports2 == reports and all(torch.equal(a.vertices, b.vertices) for a, b in zip(out, out2))


def _pair_on_device(mv, mf, xv, xf, side, builder="device", **kw):
    """(vertices, report, log) of M = (mv, mf) against X = (xv, xf) through RayTracer.untangle."""
    from volsurfs_amd.raytrace import RayTracer
    tracer = RayTracer([_mesh(xv, xf), _mesh(mv, mf)], builder=builder)
    log = []
    rep = tracer.untangle(1, 0, side, log=log, **kw)
    return tracer._meshes[1].vertices.cpu().numpy(), rep, log


def _assert_pair_equal(mv, mf, xv, xf, side, what="", builders=("device",), **kw):
    ref_v, ref, ref_log = R.untangle_pair(mv, mf, xv, xf, side, **kw)
    ref = dict(ref, shell=1, against=0)
    for builder in builders:
        v, rep, log = _pair_on_device(mv, mf, xv, xf, side, builder, **kw)
        assert np.array_equal(_bits(v), _bits(ref_v)), (what, builder)
        _assert_report(rep, ref, (what, builder))
        assert [(a, b, np.float32(c), d) for a, b, c, d in log] == \
               [(a, b, np.float32(c), d) for a, b, c, d in ref_log], (what, builder)
    return ref_v, ref


@gpu
def test_hand_cube_with_a_corner_pulled_through():
    """A cube inside a cube, one corner of the inner one pulled through the outer one's +x face.  Inward, the inner cube
    against the outer: the corner is the one violated vertex.  Outward, the outer cube against the inner: none of its
    vertices is violated at first; its faces cross, and escalation pulls them off."""
    inner, f = S.cube(0.25)
    outer, _ = S.cube(0.30)
    inner = inner.copy()
    inner[7] = (0.40, 0.20, 0.15)
    assert len(X.mesh_crossings(inner, f, outer, f)["pairs"]) > 0
    _, ref = _assert_pair_equal(inner, f, outer, f, -1, "inward", BUILDERS, margin=0.01)
    assert ref["converged"] and ref["moved_vertices"] == 1 and ref["crossings_after"] == 0
    q = S.signed_distance(outer, inner, f)
    assert (q["dist"] >= np.float32(0.01)).all()                  # clear vertices, crossing faces
    _, ref = _assert_pair_equal(outer, f, inner, f, 1, "outward", BUILDERS, margin=0.01)
    assert ref["max_level"] >= 1 and ref["crossings_before"] > 0


@gpu
def test_hand_closest_features():
    """One triangle against a cube: a vertex exactly on a face (dist = +0: it moves along the pseudonormal), one
    whose closest feature is an edge, one whose closest feature is a corner."""
    xv, xf = S.cube(0.25)
    mv = np.array([[0.25, 0.05, 0.10], [0.30, 0.30, 0.05], [0.30, 0.30, 0.30]], np.float32)
    mf = np.array([[0, 1, 2]], np.int32)
    q = S.signed_distance(mv, xv, xf)
    assert q["dist"][0] == 0 and not np.signbit(q["dist"][0]) and q["region"][0] == S.IN
    assert q["region"][1] in (S.AB, S.AC, S.BC) and q["region"][2] in (S.A, S.B, S.C)
    assert (q["dist"] < np.float32(0.1)).all()
    ref_v, ref = _assert_pair_equal(mv, mf, xv, xf, 1, "features", BUILDERS, margin=0.1)
    assert ref["moved_vertices"] == 3 and ref["converged"]
    assert np.array_equal(ref_v[0], np.array([0.25 + np.float32(0.125), 0.05, 0.10], np.float32))
    # inward from the same places: the vertex on the face goes the other way
    _assert_pair_equal(mv, mf, xv, xf, -1, "features inward", margin=0.01, max_rounds=4)


def _padded(name, total):
    """The stack's outer pair with the moving shell padded by unreferenced vertices to `total`: copies of the fixed
    shell's vertices scaled to lie below its surface, inside the margin and far outside it, in turn."""
    (xv, xf), (mv, mf) = _stack(name)[1], _stack(name)[2]
    n = total - len(mv)
    assert n > 0
    scale = np.array([0.97, 1.004, 1.05, 1.3], np.float32)[np.arange(n) % 4]
    pads = xv[(7 * np.arange(n)) % len(xv)] * scale[:, None]
    return np.concatenate([mv, pads]).astype(np.float32), mf, xv, xf


@gpu
@pytest.mark.parametrize("name,total", [("A1", n) for n in (63, 64, 65, 127, 128, 129)] +
                         [("A", n) for n in (191, 192, 193, 255, 256, 257)])
def test_wave_edges(name, total):
    """Vertex counts around the multiples of a wave.  Stack A's shells have 162 vertices: they are padded to the edges
    of the third and fourth wave, and its 42-vertex sister (subdiv 1) to those of the first and second."""
    mv, mf, xv, xf = _padded(name, total)
    ref_v, ref = _assert_pair_equal(mv, mf, xv, xf, 1, (name, total), margin=R.MARGIN_A)
    n = len(_stack(name)[2][0])
    assert (_bits(ref_v[n:]) != _bits(mv[n:])).any() and (_bits(ref_v[n:]) == _bits(mv[n:])).all(1).any()


@gpu
@pytest.mark.parametrize("max_rounds", [1, 3])
def test_exhaustion(max_rounds):
    (xv, xf), (mv, mf) = _stack("A")[1], _stack("A")[2]
    _, ref = _assert_pair_equal(mv, mf, xv, xf, 1, max_rounds, BUILDERS, margin=R.MARGIN_A, max_rounds=max_rounds)
    assert not ref["converged"] and ref["rounds"] == max_rounds


@gpu
def test_nothing_to_do():
    from volsurfs_amd.shell_untangle import untangle_shells
    shells = [icosphere(2, r) for r in (0.5, 1.0, 1.5)]
    out, reports = untangle_shells([_mesh(*m) for m in shells])
    for k, (m, rep) in enumerate(zip(out, reports)):
        assert np.array_equal(_bits(m.vertices.cpu().numpy()), _bits(shells[k][0]))
        assert rep.moved_vertices == 0 and rep.max_displacement == 0.0 and rep.converged and rep.stuck == 0
        assert rep.rounds == (0 if k == 1 else 1) and rep.crossings_before == rep.crossings_after == 0
        assert rep.self_crossings_after == 0 and rep.max_level == 0


@gpu
def test_degenerate_input():
    """Zero-area faces in the fixed shell, a duplicate of a crossing face in the moving shell, and a NaN vertex in the
    moving shell: it is left alone, counted neither as moved nor as stuck, and the others move as if it were absent.
    (The NaN vertex is one no face names: what a tree builder makes of a face with a NaN corner is not specified
    anywhere, and the moving shell's tree is built too.)"""
    (xv, xf), (mv, mf) = _stack("A")[1], _stack("A")[2]
    busy = int(np.flatnonzero(X.mesh_crossings(mv, mf, xv, xf)["count_a"])[0])
    xf2 = np.concatenate([xf[:40], [[5, 5, 5], [9, 31, 9]], xf[40:]]).astype(np.int32)
    mf2 = np.concatenate([mf, mf[busy:busy + 1]]).astype(np.int32)
    mv2 = np.concatenate([mv, [[np.nan, 0.1, 0.2]], [[0.0, 0.0, np.nan]]]).astype(np.float32)
    ref_v, ref = _assert_pair_equal(mv2, mf2, xv, xf2, 1, "degenerate", BUILDERS, margin=R.MARGIN_A)
    plain_v, plain, _ = R.untangle_pair(mv, mf, xv, xf, 1, margin=R.MARGIN_A)
    assert np.array_equal(_bits(ref_v[len(mv):]), _bits(mv2[len(mv):])) and ref["stuck"] == 0
    assert np.array_equal(_bits(ref_v[:len(mv)]), _bits(plain_v)) and ref["moved_vertices"] == plain["moved_vertices"]
    # inward too: there a query without a closest record must not count as violated (its distance is +inf)
    (xv, xf), (mv, mf) = _stack("A")[1], _stack("A")[0]
    mv2 = np.concatenate([mv, [[np.nan, 0.1, 0.2]]]).astype(np.float32)
    ref_v, ref = _assert_pair_equal(mv2, mf, xv, xf, -1, "degenerate inward", margin=R.MARGIN_A)
    assert np.array_equal(_bits(ref_v[-1:]), _bits(mv2[-1:])) and ref["stuck"] == 0 and ref["converged"]
    torch.cuda.synchronize()


@gpu
def test_determinism():
    from volsurfs_amd.shell_untangle import untangle_shells
    stack = _stack("B")
    runs = [untangle_shells([_mesh(*m) for m in stack], margin=R.MARGIN_B) for _ in range(2)]
    assert runs[0][1] == runs[1][1]
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))


@gpu
def test_stage(tmp_path):
    """`untangle_meshes` on stack B written as OBJ with per-corner UVs and as PLY with colours: names and formats kept,
    UVs, colours and faces byte-equal, the vertices the restatement's, `check_shells` clean, and the method loads it."""
    from volsurfs_amd.mesh import load_obj, load_ply, save_obj, save_ply
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.shell_untangle import untangle_meshes
    stack = _stack("B")
    names = ["-0.04", "-0.02", "0.0", "0.02", "0.04"]
    rng = np.random.default_rng(5)
    for ext in ("obj", "ply"):
        src, dst = tmp_path / f"meshes_{ext}", tmp_path / f"untangled_{ext}"
        src.mkdir()
        for name, (v, f) in zip(names, stack):
            m = _mesh(v, f)
            m.faces_uvs = torch.from_numpy(rng.random((len(f), 3, 2), dtype=np.float32)).cuda()
            if ext == "obj":
                save_obj(str(src / f"{name}.obj"), m)
            else:
                save_ply(str(src / f"{name}.ply"), m, binary=name != "0.02",
                         vertex_colors=rng.integers(0, 256, (len(v), 3)).astype(np.float32) / 255.0)
        report, check = untangle_meshes(str(src), str(dst), margin=R.MARGIN_B)
        assert sorted(os.listdir(dst)) == sorted(os.listdir(src)) == sorted(f"{n}.{ext}" for n in names)
        assert [os.path.basename(p) for p in check["files"]] == [f"{n}.{ext}" for n in names]
        assert check["nested"] == [True] * 4 and check["self_crossings"] == [0] * 5
        assert [e["pairs"] for e in check["crossings"]] == [0] * 4
        ref_v, ref_reports = _ref("B")
        for k, name in enumerate(names):
            _assert_report(report[k], ref_reports[k], (ext, k))
            a, b = str(src / f"{name}.{ext}"), str(dst / f"{name}.{ext}")
            if ext == "obj":
                before, after = load_obj(a), load_obj(b)
            else:
                (before, c0), (after, c1) = load_ply(a, return_colors=True), load_ply(b, return_colors=True)
                assert c0 is not None and torch.equal(c0, c1)
                with open(a, "rb") as fa, open(b, "rb") as fb:
                    assert fa.read(40).split(b"\n")[1] == fb.read(40).split(b"\n")[1]       # ascii stays ascii
            assert torch.equal(before.faces, after.faces) and after.has_uvs
            assert torch.equal(before.faces_uvs.view(torch.int32), after.faces_uvs.view(torch.int32))
            assert np.array_equal(_bits(after.vertices.cpu().numpy()), _bits(ref_v[k])), (ext, k)
        if ext == "obj":
            m = VolSurfs.from_meshes_path(str(dst), str(tmp_path / "ckpt"), max_rays=4096, textures_res=(64, 32, 16, 8))
            assert m.nr_meshes == 5


def _holed_stack():
    """Stack A with the six faces around vertex HOLE_VERTEX of the fixed (middle) shell removed."""
    stack = [(v, f) for v, f in _stack("A")]
    xv, xf = stack[1]
    ring = (xf == HOLE_VERTEX).any(1)
    assert ring.sum() == 6
    stack[1] = (xv, xf[~ring])
    return stack


HOLE_VERTEX = 100


def test_restatement_winding_converges_on_the_holed_stack():
    """With the exact float64 winding number as the sign: the input of the device's property test converges."""
    stack = _holed_stack()
    out, reports = R.untangle_shells(stack, margin=R.MARGIN_A, sign="winding")
    for k in (0, 2):
        assert reports[k]["converged"] and reports[k]["crossings_after"] == 0 and reports[k]["moved_vertices"] > 0


@gpu
def test_winding_sign_on_an_open_fixed_shell():
    """A property test: the device sums the winding number in fp32 with a far field, the restatement exactly."""
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.shell_untangle import untangle_shells
    stack = _holed_stack()
    tracer = RayTracer([_mesh(*m) for m in stack], builder="device")
    assert tracer.edge_census(1)["boundary"] == 6
    out, reports = untangle_shells(tracer, margin=R.MARGIN_A, sign="winding")
    for k, side in ((0, -1), (2, 1)):
        rep = reports[k]
        assert rep.converged and rep.crossings_after == 0 and rep.stuck == 0 and rep.moved_vertices > 0
        v = out[k].vertices
        moved = (v.view(torch.int32) != torch.from_numpy(_bits(stack[k][0])).cuda()).any(1)
        assert int(moved.sum()) == rep.moved_vertices
        d = tracer.signed_distance(v[moved].contiguous(), 1, sign="winding")["dist"]
        assert bool((side * d >= np.float32(R.MARGIN_A)).all())
        assert len(X.mesh_crossings(v.cpu().numpy(), stack[k][1], *stack[1])["pairs"]) == 0
