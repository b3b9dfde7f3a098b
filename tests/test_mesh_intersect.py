"""Exact mesh crossings on the device (volsurfs_amd/mesh_intersect.py, RayTracer.crossings, csrc/mesh_cross.hip,
csrc/cross_walk.h) against the restated rule (tests/mesh_intersect_restated.py: brute force over all pairs in
numpy float64, in the device's operation order).  The reference has no such stage.  Every comparison is exact equality:
pairs, counts and segment end points."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import mesh_intersect_restated as R
from volsurfs_amd import _lib
from volsurfs_amd.mesh import icosphere

ERR_ARG = -1
gpu = pytest.mark.gpu

# A = (0,0,0), (4,0,0), (0,4,0) against each B: does it cross?
HAND_A = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
HAND = [
    ([(1, 1, -1), (1, 1, 1), (3, 3, 1)], True),       # pierces the interior
    ([(1, 1, 1), (1, 1, 2), (3, 3, 1)], False),       # above
    ([(1, 1, 0), (1, 1, 2), (3, 3, 1)], False),       # a vertex touches the plane
    ([(1, 1, 0), (3, 1, 0), (1, 3, 0)], False),       # coplanar overlap
    ([(0, 0, 0), (2, 1, -1), (2, 1, 1)], True),       # shares a vertex, the opposite edge pierces
    ([(0, 0, 0), (4, 0, 0), (0, 1, 3)], False),       # shares an edge
    ([(2, 0, -1), (2, 0, 1), (2, -3, 0)], True),      # through an edge of A
    ([(4, 0, -1), (4, 0, 1), (7, 0, 0)], True),       # through a vertex of A
    ([(5, 5, -1), (5, 5, 1), (6, 6, 0)], False),      # beside
]
SHIFT = np.array([0.5, 0.1, 0.05], np.float32)


# ---------------------------------------------------------------------------------------------------------- CPU

def test_entry_points_declared_built_and_prototyped():
    names, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    mesh_args = [P, P, I, P, I, P, LL, P, LL, P, LL, P, LL, P, I]
    expected = {
        "vsa_mesh_cross_workspace_bytes": (LL, [LL, LL, I]),
        "vsa_mesh_cross_count": (I, mesh_args + [P, P, P, P, P, LL, P]),
        "vsa_mesh_cross_emit": (I, mesh_args + [P, LL, P, P, P, LL, P]),
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
    frame = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)

    def mesh_args(qnodes=p, tris=p, root=0, frame=frame, depth=10, tv=p, ntv=4, tf=p, ntf=5, qv=p, nqv=4, qf=p,
                  nqf=5, order=None, self_mode=0):
        return (qnodes, tris, root, frame, depth, tv, ntv, tf, ntf, qv, nqv, qf, nqf, order, self_mode)

    def count(count_q=p, count_t=p, offsets=p, total=p, ws=p, ws_bytes=1 << 20, **kw):
        return L.vsa_mesh_cross_count(*mesh_args(**kw), count_q, count_t, offsets, total, ws, ws_bytes, None)

    def emit(offsets=p, nr_pairs=3, pairs=p, segs=p, ws=p, ws_bytes=1 << 20, **kw):
        return L.vsa_mesh_cross_emit(*mesh_args(**kw), offsets, nr_pairs, pairs, segs, ws, ws_bytes, None)

    shared = [{n: None} for n in ("qnodes", "tris", "frame", "tv", "tf", "qv", "qf")]
    shared += [{"root": -1}, {"depth": 48}, {"depth": 99}, {"ntv": 0}, {"ntf": 0}, {"ntf": -2}, {"nqv": 0}, {"nqf": 0},
               {"nqf": -1}, {"self_mode": 2}, {"self_mode": -1}, {"self_mode": 1, "nqf": 6}, {"self_mode": 1, "nqv": 3}]
    null = dict(qnodes=None, tris=None, tv=None, tf=None, qv=None, qf=None)
    for kw in shared:
        assert count(**kw) == ERR_ARG, kw
        assert emit(**kw) == ERR_ARG, kw
        assert count(**dict(kw, **null)) == ERR_ARG, kw
        assert emit(**dict(kw, **null), offsets=None, pairs=None, ws=None) == ERR_ARG, kw
    for kw in ({"count_q": None}, {"count_t": None}, {"offsets": None}, {"total": None}, {"ws": None},
               {"count_q": None, "self_mode": 1}, {"offsets": None, "count_t": None, "self_mode": 1}):
        assert count(**kw) == ERR_ARG, kw
    for kw in ({"offsets": None}, {"pairs": None}, {"ws": None}, {"nr_pairs": 0}, {"nr_pairs": -3}):
        assert emit(**kw) == ERR_ARG, kw
    for args in ((0, 0, 0), (-1, 0, 0), (5, -1, 0), (0, 3, 1)):
        assert L.vsa_mesh_cross_workspace_bytes(*args) == ERR_ARG, args


def _tri(points):
    return np.array(points, np.float64)


def test_restatement_hand_cases_in_both_orders():
    A = _tri(HAND_A)
    for points, expected in HAND:
        B = _tri(points)
        assert bool(R.crosses(A, B)) == expected, points
        assert bool(R.crosses(B, A)) == expected, points
    # orient on a unit corner: the volume form, and its sign under a swap
    o, x, y, z = _tri([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)])
    assert R.orient(x, y, z, o) == 1.0 and R.orient(y, x, z, o) == -1.0


def test_restatement_segment_of_the_first_case():
    """The piercing triangle's edges 0 and 2 go through A's plane at (1, 1, 0) and (2, 2, 0).  With the piercing
    triangle as the first argument those are the first and the last piercing edge.  The second point lies on A's
    border, where A's own edge 1 passes through the border of the other triangle: three edges pierce, and with A as the
    first argument the first and the last of them give the same point (include/volsurfs_hip.h "segment")."""
    A, B = _tri(HAND_A), _tri(HAND[0][0])
    assert np.array_equal(R.segment(B, A), [[1.0, 1.0, 0.0], [2.0, 2.0, 0.0]])
    assert R.pierces(A, B)[0].tolist() == [False, True, False, True, False, True]
    assert np.array_equal(R.segment(A, B), [[2.0, 2.0, 0.0], [2.0, 2.0, 0.0]])
    assert np.isnan(R.segment(A, _tri(HAND[1][0]))).all()


def test_restatement_icospheres():
    v, f = icosphere(2)
    assert len(R.self_crossings(v, f)["pairs"]) == 0
    assert len(R.mesh_crossings(v, f, v * np.float32(0.99), f)["pairs"]) == 0
    res = R.mesh_crossings(v, f, v + SHIFT, f)
    assert len(res["pairs"]) > 0
    assert res["count_a"].sum() == res["count_b"].sum() == len(res["pairs"])
    assert np.isfinite(res["segments"]).all()
    # a NaN vertex: its faces cross nothing, not even by the edge between their two other vertices
    bad = v.copy()
    bad[f[res["pairs"][0, 0], 0], 0] = np.nan
    touched = np.flatnonzero((f == f[res["pairs"][0, 0], 0]).any(1))
    assert R.mesh_crossings(bad, f, v + SHIFT, f)["count_a"][touched].sum() == 0
    assert R.mesh_crossings(v + SHIFT, f, bad, f)["count_b"][touched].sum() == 0


# ---------------------------------------------------------------------------------------------------------- GPU

def _mesh(v, f):
    from volsurfs_amd.mesh import TensorMesh
    return TensorMesh(np.asarray(v, np.float32), np.asarray(f, np.int32), device="cuda")


def _assert_equal(res, ref, what=""):
    pairs = res.pairs.cpu().numpy()
    assert pairs.dtype == np.int64 and np.array_equal(pairs, ref["pairs"]), what
    assert res.count_a.dtype == torch.int32 and np.array_equal(res.count_a.cpu().numpy(), ref["count_a"]), what
    assert np.array_equal(res.count_b.cpu().numpy(), ref["count_b"]), what
    if res.segments is not None:
        seg = res.segments.cpu().numpy()
        assert seg.dtype == np.float64 and seg.shape == ref["segments"].shape, what
        assert np.array_equal(seg, ref["segments"]), what


def _assert_sorted(pairs):
    key = pairs[:, 0] * (1 << 32) + pairs[:, 1]
    assert bool((key[1:] > key[:-1]).all())


@functools.lru_cache(maxsize=None)
def _two_spheres():
    """icosphere(2) (320 faces) and icosphere(3) (1 280 faces) moved by SHIFT, with the restated answer both ways."""
    va, fa = icosphere(2)
    vb, fb = icosphere(3)
    vb = vb + SHIFT
    ab = R.mesh_crossings(va, fa, vb, fb)
    ba = R.mesh_crossings(vb, fb, va, fa)
    assert len(ab["pairs"]) > 100 and len(ba["pairs"]) > 100
    return (va, fa), (vb, fb), ab, ba


@gpu
def test_hand_cases_on_the_device():
    """The nine hand cases as one-face meshes, in both orders, with segments."""
    from volsurfs_amd.mesh_intersect import mesh_crossings
    one = [[0, 1, 2]]
    for points, expected in HAND:
        for a, b in ((HAND_A, points), (points, HAND_A)):
            res = mesh_crossings(_mesh(a, one), _mesh(b, one), segments=True)
            _assert_equal(res, R.mesh_crossings(a, one, b, one), (a, b))
            assert res.pairs.shape[0] == int(expected), (a, b)
    res = mesh_crossings(_mesh(HAND[0][0], one), _mesh(HAND_A, one), segments=True)
    assert res.segments.cpu().tolist() == [[[1.0, 1.0, 0.0], [2.0, 2.0, 0.0]]]
    assert res.length() == 2.0 ** 0.5


@gpu
@pytest.mark.parametrize("direction", ["ab", "ba"])
@pytest.mark.parametrize("builder", ["host", "device", "ploc"])
def test_two_meshes_equal_brute_force(builder, direction):
    from volsurfs_amd.mesh_intersect import mesh_crossings
    from volsurfs_amd.raytrace import RayTracer
    a, b, ab, ba = _two_spheres()
    (q, t, ref) = (a, b, ab) if direction == "ab" else (b, a, ba)
    tracer = RayTracer([_mesh(*t)], builder=builder)
    res = mesh_crossings(_mesh(*q), (tracer, 0), segments=True)
    _assert_equal(res, ref, (builder, direction))
    _assert_sorted(res.pairs)
    assert int(res.count_a.sum()) == int(res.count_b.sum()) == res.pairs.shape[0]
    again = tracer.crossings(_mesh(*q), 0, segments=True)
    for x, y in zip(res, again):
        assert torch.equal(x, y)
    # the query in a tracer of its own: taken in leaf order, the same bytes
    other = mesh_crossings((RayTracer([_mesh(*q)], builder=builder), 0), (tracer, 0), segments=True)
    for x, y in zip(res, other):
        assert torch.equal(x, y)
    # without segments: the same pairs and counts
    _assert_equal(mesh_crossings(_mesh(*q), (tracer, 0)), ref, (builder, direction))


@gpu
def test_wave_edges():
    """Query meshes of 1, 63, 64, 65 and 129 faces: prefixes of the two meshes above."""
    from volsurfs_amd.mesh_intersect import mesh_crossings
    from volsurfs_amd.raytrace import RayTracer
    (va, fa), (vb, fb), ab, ba = _two_spheres()
    for (vq, fq), t, ref in (((va, fa), (vb, fb), ab), ((vb, fb), (va, fa), ba)):
        tracer = RayTracer([_mesh(*t)], builder="device")
        for n in (1, 63, 64, 65, 129):
            keep = ref["pairs"][:, 0] < n
            want = {"pairs": ref["pairs"][keep], "count_a": ref["count_a"][:n], "segments": ref["segments"][keep],
                    "count_b": np.bincount(ref["pairs"][keep][:, 1], minlength=len(t[1])).astype(np.int32)}
            _assert_equal(mesh_crossings(_mesh(vq, fq[:n]), (tracer, 0), segments=True), want, n)


@gpu
def test_ranges():
    """Against icosphere(3): one triangle 50 radii wide slicing it (94 pairs from one lane: about as many of its 1 280
    faces as one plane can cut), one of width 1e-3 piercing a single face, one 100 radii away."""
    from volsurfs_amd.mesh_intersect import mesh_crossings
    from volsurfs_amd.raytrace import RayTracer
    v, f = icosphere(3)
    c = v[f[7]].mean(0)
    t = v[f[7, 1]] - v[f[7, 0]]
    tiny = np.stack([c * np.float32(1 - 5e-4), c * np.float32(1 + 5e-4), c + t * np.float32(1e-3 / np.linalg.norm(t))])
    cases = {"wide": ([(-25, -20, 0.11), (25, -21, 0.13), (1, 29, 0.07)], lambda n: n > 80),
             "tiny": (tiny, lambda n: n == 1),
             "far": ([(100, 0, 0), (101, 0, 0), (100, 1, 0)], lambda n: n == 0)}
    one = [[0, 1, 2]]
    for builder in ("host", "device", "ploc"):
        tracer = RayTracer([_mesh(v, f)], builder=builder)
        for name, (tri, holds) in cases.items():
            tri = np.asarray(tri, np.float32)
            ref = R.mesh_crossings(tri, one, v, f)
            assert holds(len(ref["pairs"])), (name, len(ref["pairs"]))
            _assert_equal(mesh_crossings(_mesh(tri, one), (tracer, 0), segments=True), ref, (builder, name))
            # and the sphere as the query against the one triangle's tree
            back = mesh_crossings((tracer, 0), _mesh(tri, one), segments=True)
            _assert_equal(back, R.mesh_crossings(v, f, tri, one), (builder, name, "back"))


@functools.lru_cache(maxsize=None)
def _crossing_pair_as_one_mesh():
    (va, fa), (vb, fb), _, _ = _two_spheres()
    v, f = np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)])
    return v, f, R.self_crossings(v, f)


def _assert_self_equal(res, ref, what=""):
    assert np.array_equal(res.pairs.cpu().numpy(), ref["pairs"]), what
    assert np.array_equal(res.count.cpu().numpy(), ref["count"]), what
    if res.segments is not None:
        assert np.array_equal(res.segments.cpu().numpy(), ref["segments"]), what


@gpu
def test_self_crossings():
    from volsurfs_amd.mesh_intersect import self_crossings
    from volsurfs_amd.raytrace import RayTracer
    sphere = self_crossings(_mesh(*icosphere(3)), segments=True)
    assert sphere.pairs.shape == (0, 2) and sphere.segments.shape == (0, 2, 3) and int(sphere.count.sum()) == 0
    v, f, ref = _crossing_pair_as_one_mesh()
    assert len(ref["pairs"]) > 100 and (ref["pairs"][:, 0] < ref["pairs"][:, 1]).all()
    for builder in ("host", "device", "ploc"):
        res = self_crossings((RayTracer([_mesh(v, f)], builder=builder), 0), segments=True)
        _assert_self_equal(res, ref, builder)
        _assert_sorted(res.pairs)
        # the partner counts are symmetric: every pair counts once for each of its faces
        flat = res.pairs.flatten()
        assert torch.equal(torch.bincount(flat, minlength=len(f)).int(), res.count)
    # the same mesh as an unwelded soup: three vertices of its own per face
    soup = self_crossings(_mesh(v[f].reshape(-1, 3), np.arange(3 * len(f)).reshape(-1, 3)), segments=True)
    _assert_self_equal(soup, ref, "soup")
    # with its faces permuted: the permuted pairs
    perm = np.random.default_rng(3).permutation(len(f))
    res = self_crossings(_mesh(v, f[perm]))
    old = np.sort(perm[res.pairs.cpu().numpy()], axis=1)
    assert np.array_equal(old[np.lexsort(old.T[::-1])], ref["pairs"])
    assert np.array_equal(res.count.cpu().numpy(), ref["count"][perm])


@gpu
def test_degenerate_input():
    """Faces (i, i, i) and a duplicated face in both meshes, and a NaN vertex in the query mesh, mixed into the crossing
    pair of spheres: the restated answer, and the run ends clean.  (The NaN sits in the query mesh only: what a tree
    builder makes of a NaN vertex is not specified anywhere.)"""
    from volsurfs_amd.mesh_intersect import mesh_crossings
    (va, fa), (vb, fb), ab, _ = _two_spheres()
    busy_a, busy_b = ab["pairs"][0]
    va = va.copy()
    nan_vertex = fa[ab["pairs"][-1, 0], 1]
    va[nan_vertex, 1] = np.nan
    fa2 = np.concatenate([fa[:50], [[5, 5, 5], [9, 9, 9]], fa[50:], fa[busy_a:busy_a + 1], [[0, 0, 0]]]).astype(np.int32)
    fb2 = np.concatenate([[[3, 3, 3]], fb, fb[busy_b:busy_b + 1], [[600, 600, 600]]]).astype(np.int32)
    ref = R.mesh_crossings(va, fa2, vb, fb2)
    assert len(ref["pairs"]) > 100 and ref["count_a"][(fa2 == nan_vertex).any(1)].sum() == 0
    assert ref["count_a"][-2] == ref["count_a"][busy_a + 2 * (busy_a >= 50)] > 0        # the duplicate crosses too
    for a, b in ((_mesh(va, fa2), _mesh(vb, fb2)),):
        res = mesh_crossings(a, b, segments=True)
        _assert_equal(res, ref, "degenerate")
    torch.cuda.synchronize()


@gpu
def test_the_48_entry_stack():
    """The stack's size depends on the `max_depth` argument alone: a shallow tree walked with max_depth = 30 (the
    48-entry stack) gives the bytes it gives with its true depth (the 24-entry one), in both passes and in self mode."""
    from volsurfs_amd import mesh_intersect as MI
    from volsurfs_amd.raytrace import RayTracer
    (va, fa), (vb, fb), ab, _ = _two_spheres()
    tracer = RayTracer([_mesh(vb, fb)], builder="device")
    assert tracer.max_depth < 24
    tree = MI._tree((tracer, 0), "test")
    query = MI._query(_mesh(va, fa), tracer.device, "test")
    shallow = MI._cross(tree, query, False, True, True)
    deep = MI._cross(tree, query, False, True, True, max_depth=30)
    for x, y in zip(shallow[:4], deep[:4]):
        assert torch.equal(x, y)
    assert shallow[4] == deep[4] == len(ab["pairs"])
    v, f, ref = _crossing_pair_as_one_mesh()
    tracer = RayTracer([_mesh(v, f)], builder="device")
    tree = MI._tree((tracer, 0), "test")
    deep = MI._cross(tree, (tree[2], tree[3], MI._leaf_order(tracer, 0)), True, True, True, max_depth=30)
    _assert_self_equal(MI.SelfCrossings(deep[0], deep[1], deep[3]), ref, "deep")
    with pytest.raises(_lib.VolsurfsHipError):
        MI._cross(tree, (tree[2], tree[3], None), True, False, True, max_depth=48)


def _shell(radius, centre=(0.0, 0.0, 0.0), subdiv=3):
    v, f = icosphere(subdiv, radius)
    return v + np.asarray(centre, np.float32), f


def _shell_cases():
    two = (np.concatenate([_shell(0.3)[0], _shell(0.3, (3, 0, 0))[0]]),
           np.concatenate([_shell(0.3)[1], _shell(0.3)[1] + len(_shell(0.3)[0])]))
    return {"nested": [_shell(0.98), _shell(0.99), _shell(1.0)],
            "poking": [_shell(0.98), _shell(0.99, (0.05, 0.0, 0.0)), _shell(1.0)],
            "away": [_shell(0.98, (3, 0, 0)), _shell(0.99), _shell(1.0)],
            "two": [two, _shell(0.99), _shell(1.0)]}


@gpu
def test_shell_crossings_and_shells_nested():
    from volsurfs_amd.mesh_intersect import shell_crossings, shells_nested
    cases = {k: [_mesh(*m) for m in ms] for k, ms in _shell_cases().items()}
    res = shell_crossings(cases["nested"])
    assert res == [{"pair": (0, 1), "pairs": 0, "faces_inner": 0, "faces_outer": 0},
                   {"pair": (1, 2), "pairs": 0, "faces_inner": 0, "faces_outer": 0}]
    assert shells_nested(cases["nested"]) == [True, True]
    assert shells_nested(cases["nested"], sign="winding") == [True, True]
    res = shell_crossings(cases["poking"])
    for k, entry in enumerate(res):
        ref = R.mesh_crossings(*_shell_cases()["poking"][k], *_shell_cases()["poking"][k + 1])
        assert entry["pairs"] == len(ref["pairs"]) > 0
        assert entry["faces_inner"] == int((ref["count_a"] > 0).sum())
        assert entry["faces_outer"] == int((ref["count_b"] > 0).sum())
    assert shells_nested(cases["poking"]) == [False, False]
    # no crossing either way: the component check decides
    assert [e["pairs"] for e in shell_crossings(cases["away"])] == [0, 0]
    assert shells_nested(cases["away"]) == [False, True]
    assert [e["pairs"] for e in shell_crossings(cases["two"])] == [0, 0]
    assert shells_nested(cases["two"]) == [False, True]
    with pytest.raises(ValueError):
        shells_nested(cases["nested"], sign="parity")


@gpu
def test_check_shells(tmp_path):
    from volsurfs_amd.mesh import save_ply
    from volsurfs_amd.mesh_intersect import check_shells
    for name, m in zip(("0.01", "-0.01", "0.0"), (_shell(1.0), _shell(0.98), _shell(0.99, (0.05, 0.0, 0.0)))):
        save_ply(os.path.join(tmp_path, name + ".ply"), _mesh(*m))
    res = check_shells(str(tmp_path))
    assert [os.path.basename(p) for p in res["files"]] == ["-0.01.ply", "0.0.ply", "0.01.ply"]
    assert res["self_crossings"] == [0, 0, 0]
    assert [e["pair"] for e in res["crossings"]] == [(0, 1), (1, 2)] and all(e["pairs"] > 0 for e in res["crossings"])
    assert res["nested"] == [False, False]


@gpu
def test_crossing_stats():
    from volsurfs_amd.mesh_intersect import crossing_stats, mesh_crossings
    a, b, ab, _ = _two_spheres()
    res = mesh_crossings(_mesh(*a), _mesh(*b))
    want = (res.pairs.shape[0], int((res.count_a > 0).sum()), int((res.count_b > 0).sum()))
    assert crossing_stats(_mesh(*a), _mesh(*b)) == want
    assert want == (len(ab["pairs"]), int((ab["count_a"] > 0).sum()), int((ab["count_b"] > 0).sum()))
