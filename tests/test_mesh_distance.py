"""Mesh-to-mesh distance on the device (volsurfs_amd/mesh_distance.py, RayTracer.closest*, csrc/mesh_distance.hip,
csrc/closest_walk.h) against the restated rule (tests/mesh_distance_restated.py: brute force in numpy, in
the device's float32 operation order).  The reference has no such stage.  Comparisons are exact equality except the two
float64 sums, whose bound is derived where it is used."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import mesh_distance_restated as R
from volsurfs_amd import _lib

ERR_ARG = -1
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- CPU

def test_entry_points_declared_built_and_prototyped():
    names, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    P, I, LL, ULL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong
    expected = {
        "vsa_closest_point_q": (I, [P, P, P, P, I, I, P, LL, P, P, P, P]),
        "vsa_closest_point_q_stats": (I, [P, P, P, P, I, I, P, LL, P, P]),
        "vsa_closest_walk_config": (I, [I]),
        "vsa_surface_area_prefix_workspace_bytes": (LL, [LL]),
        "vsa_surface_area_prefix": (I, [P, LL, LL, P, LL, P, P]),
        "vsa_surface_sample": (I, [P, LL, LL, P, LL, ULL, P, P, P, P]),
        "vsa_surface_distance": (I, [P, LL, LL, P, P, P, I, P, I, LL, ULL, P, I, P, P, P]),
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
    p = ctypes.addressof(buf)                      # a non-null pointer; never dereferenced on the device
    roots, frames = (ctypes.c_int32 * 1)(0), (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)

    def closest(qnodes=p, tris=p, mesh_roots=roots, mesh_frames=frames, nr_meshes=1, max_depth=10, points=p,
                nr_points=5, dist=p, slot=p, bary=p):
        return L.vsa_closest_point_q(qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth, points, nr_points,
                                     dist, slot, bary, None)

    for name in ("qnodes", "tris", "mesh_roots", "mesh_frames", "points", "dist", "slot"):
        assert closest(**{name: None}) == ERR_ARG, name
    null = dict(qnodes=None, tris=None, points=None, dist=None, slot=None, bary=None)
    assert closest(**null) == ERR_ARG
    for kw in ({"nr_meshes": 0}, {"nr_meshes": 17}, {"nr_meshes": -1}, {"nr_points": 0}, {"nr_points": -4},
               {"max_depth": 48}, {"max_depth": 99}):
        assert closest(**kw) == ERR_ARG, kw
        assert closest(**dict(kw, **null)) == ERR_ARG, kw

    def counting(counters=p, nr_meshes=1, nr_points=5, max_depth=10, qnodes=p):
        return L.vsa_closest_point_q_stats(qnodes, p, roots, frames, nr_meshes, max_depth, p, nr_points, counters, None)

    for kw in ({"counters": None}, {"qnodes": None}, {"nr_meshes": 0}, {"nr_meshes": 17}, {"nr_points": 0},
               {"max_depth": 48}):
        assert counting(**kw) == ERR_ARG, kw

    assert L.vsa_closest_walk_config(-1) == ERR_ARG and L.vsa_closest_walk_config(3) == ERR_ARG
    assert L.vsa_closest_walk_config(1) == 0                      # (the default; host state only)
    assert L.vsa_surface_area_prefix_workspace_bytes(0) == ERR_ARG
    assert L.vsa_surface_area_prefix_workspace_bytes(-3) == ERR_ARG

    def prefix(tris=p, first=0, nr=4, ws=p, ws_bytes=1 << 20, out=p):
        return L.vsa_surface_area_prefix(tris, first, nr, ws, ws_bytes, out, None)

    for kw in ({"tris": None}, {"ws": None}, {"out": None}, {"first": -1}, {"nr": 0}, {"nr": -2}):
        assert prefix(**kw) == ERR_ARG, kw
        assert prefix(**dict(kw, tris=None, ws=None, out=None)) == ERR_ARG, kw

    def sample(tris=p, first=0, nr=4, pre=p, n=10, seed=0, points=p, slot=p, bary=p):
        return L.vsa_surface_sample(tris, first, nr, pre, n, seed, points, slot, bary, None)

    for kw in ({"tris": None}, {"pre": None}, {"points": None}, {"first": -1}, {"nr": 0}, {"n": 0}, {"n": -1}):
        assert sample(**kw) == ERR_ARG, kw
        assert sample(**dict(kw, tris=None, pre=None, points=None, slot=None, bary=None)) == ERR_ARG, kw

    def tau(*values):
        return (ctypes.c_float * len(values))(*values)

    def distance(src=p, first=0, nr=4, pre=p, qnodes=p, tris=p, root=0, frame=frames, depth=10, n=10, seed=0,
                 th=tau(0.1), nr_th=1, stats=p, partials=p):
        return L.vsa_surface_distance(src, first, nr, pre, qnodes, tris, root, frame, depth, n, seed, th, nr_th, stats,
                                      partials, None)

    null = dict(src=None, pre=None, qnodes=None, tris=None, stats=None, partials=None)
    for name in ("src", "pre", "qnodes", "tris", "frame", "stats", "partials", "th"):
        assert distance(**{name: None}) == ERR_ARG, name
    assert distance(**null) == ERR_ARG
    for kw in ({"first": -1}, {"nr": 0}, {"n": 0}, {"n": -7}, {"root": -1}, {"depth": 48}, {"nr_th": -1},
               {"nr_th": 9, "th": tau(*[0.1] * 9)}, {"th": tau(-0.5)}, {"th": tau(float("nan"))},
               {"th": tau(0.1, -1e-9), "nr_th": 2}):
        assert distance(**kw) == ERR_ARG, kw
        assert distance(**dict(kw, **null)) == ERR_ARG, kw


# the triangle (0,0,0), (4,0,0), (0,4,0) as a record, and one dyadic query in each of the seven regions, above and
# below the plane: (point, d2, u, v), worked by hand from the rule
TRIANGLE = np.array([[0, 0, 0, 0, 4, 0, 0, 0, 0, 4, 0, 0]], np.float32)
REGIONS = [
    ("A", (-1.0, -2.0, 2.0), 9.0, 0.0, 0.0), ("A", (-1.0, -2.0, -2.0), 9.0, 0.0, 0.0),
    ("B", (6.0, -1.0, 2.0), 9.0, 1.0, 0.0), ("B", (6.0, -1.0, -2.0), 9.0, 1.0, 0.0),
    ("AB", (1.0, -2.0, 1.0), 5.0, 0.25, 0.0), ("AB", (1.0, -2.0, -1.0), 5.0, 0.25, 0.0),
    ("C", (-1.0, 6.0, 2.0), 9.0, 0.0, 1.0), ("C", (-1.0, 6.0, -2.0), 9.0, 0.0, 1.0),
    ("AC", (-2.0, 1.0, 1.0), 5.0, 0.0, 0.25), ("AC", (-2.0, 1.0, -1.0), 5.0, 0.0, 0.25),
    ("BC", (3.0, 3.0, 1.0), 3.0, 0.5, 0.5), ("BC", (3.0, 3.0, -1.0), 3.0, 0.5, 0.5),
    ("in", (1.0, 1.0, 2.0), 4.0, 0.25, 0.25), ("in", (1.0, 1.0, -2.0), 4.0, 0.25, 0.25),
]
REGION_POINTS = np.array([r[1] for r in REGIONS], np.float32)
REGION_EXPECTED = np.array([r[2:] for r in REGIONS], np.float32)


def test_restatement_seven_regions_by_hand():
    d2, u, v = R.closest_on_triangles(REGION_POINTS, TRIANGLE)
    got = np.stack([d2[:, 0], u[:, 0], v[:, 0]], 1)
    assert np.array_equal(got, REGION_EXPECTED), got
    # the zero-area record: its v0, whatever the query
    point = np.array([[1, 2, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.float32)
    d2, u, v = R.closest_on_triangles(np.array([[1, 2, 5], [1, 2, 3], [-1, 2, 3]], np.float32), point)
    assert np.array_equal(d2[:, 0], np.array([4, 0, 4], np.float32)) and not u.any() and not v.any()
    # a record with one zero edge (v1 = v0): the closest point lies on the edge v0 v2
    sliver = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0]], np.float32)
    d2, u, v = R.closest_on_triangles(np.array([[3, 1, 0]], np.float32), sliver)
    assert (d2[0, 0], u[0, 0], v[0, 0]) == (9.0, 0.0, 0.25)
    # brute force: the minimum over (d2, id) -- two coincident records, the smaller id wins wherever it stands
    two = np.concatenate([TRIANGLE, TRIANGLE])
    two[:, 3] = np.array([7, 2], np.int32).view(np.float32)
    res = R.closest(REGION_POINTS, two)
    assert (res["face"] == 2).all() and (res["slot"] == 1).all()
    assert np.array_equal(res["dist"], np.sqrt(REGION_EXPECTED[:, 0]))
    st = R.statistics(np.array([3, 4], np.float32), (3.0, 3.5, 4.0))
    assert st["within"] == (1, 1, 2) and st["mean"] == 3.5 and st["rms"] == math.sqrt(12.5) and st["max"] == 4.0


# ---------------------------------------------------------------------------------------------------------- GPU

def _mesh(v, f):
    from volsurfs_amd.mesh import TensorMesh
    return TensorMesh(np.asarray(v, np.float32), np.asarray(f, np.int32), device="cuda")


def _records(mesh):
    """The mesh's triangle records in face order ([F, 12] f32 numpy: v0, id | e1 | e2), as every builder forms them."""
    v = mesh.vertices.cpu().numpy()
    f = mesh.faces.cpu().numpy().astype(np.int64)
    rec = np.zeros((f.shape[0], 12), np.float32)
    rec[:, 0:3] = v[f[:, 0]]
    rec[:, 3] = np.arange(f.shape[0], dtype=np.int32).view(np.float32)
    rec[:, 4:7] = v[f[:, 1]] - v[f[:, 0]]
    rec[:, 8:11] = v[f[:, 2]] - v[f[:, 0]]
    return rec


def _assert_equals_restated(res, ref, what=""):
    assert np.array_equal(res["dist"].cpu().numpy(), ref["dist"]), what
    assert np.array_equal(res["face"].cpu().numpy(), ref["face"]), what
    assert np.array_equal(res["bary"].cpu().numpy(), np.stack([ref["u"], ref["v"]], 1)), what


@gpu
def test_seven_regions_on_the_device():
    from volsurfs_amd.raytrace import RayTracer
    far = np.float32(100.0)
    v = [[0, 0, 0], [4, 0, 0], [0, 4, 0], [far, far, far], [far + 4, far, far], [far, far + 4, far]]
    tracer = RayTracer([_mesh(v, [[0, 1, 2], [3, 4, 5]])], builder="device")
    res = tracer.closest(torch.from_numpy(REGION_POINTS).cuda())
    assert np.array_equal(res["dist"].cpu().numpy(), np.sqrt(REGION_EXPECTED[:, 0]))
    assert np.array_equal(res["bary"].cpu().numpy(), REGION_EXPECTED[:, 1:])
    assert (res["face"] == 0).all()
    assert torch.equal(tracer.slot_face_id[res["slot"].long()].long(), res["face"])


@functools.lru_cache(maxsize=None)
def _three_shells():
    from volsurfs_amd.mesh import icosphere
    return tuple(_mesh(*icosphere(s, r)) for s, r in ((1, 0.30), (2, 0.32), (3, 0.34)))


@functools.lru_cache(maxsize=None)
def _three_shell_queries():
    """1037 random points of [-0.5, 0.5]^3, every vertex of the largest shell, every edge midpoint of the smallest, the
    centre (all faces tie, or nearly: the deepest walk and the tie rule) and one point 10 extents away; with the
    restated answer per shell, computed once."""
    small, _, large = _three_shells()
    rng = np.random.default_rng(11)
    v, f = small.vertices.cpu().numpy(), small.faces.cpu().numpy()
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.unique(np.sort(e, axis=1), axis=0)
    mid = ((v[e[:, 0]] + v[e[:, 1]]) * np.float32(0.5)).astype(np.float32)
    pts = np.concatenate([rng.uniform(-0.5, 0.5, (1037, 3)).astype(np.float32), large.vertices.cpu().numpy(), mid,
                          np.zeros((1, 3), np.float32), np.array([[6.8, 0.1, -0.2]], np.float32)])
    assert e.shape[0] == 120 and pts.shape[0] == 1037 + 642 + 120 + 2
    ref = tuple(R.closest(pts, _records(m)) for m in _three_shells())
    return pts, ref


@gpu
@pytest.mark.parametrize("leaf_size", [1, 4, 8])
@pytest.mark.parametrize("builder", ["host", "device", "ploc"])
def test_equals_brute_force(builder, leaf_size):
    """dist, face and bary of all three shells equal the restated brute force exactly, for every builder and leaf size
    (so the nine combinations are equal to one another), through closest_all and through closest."""
    from volsurfs_amd.raytrace import RayTracer
    meshes = _three_shells()
    pts, ref = _three_shell_queries()
    tracer = RayTracer(list(meshes), leaf_size=leaf_size, builder=builder)
    q = torch.from_numpy(pts).cuda()
    res = tracer.closest_all(q)
    assert res["dist"].shape == (3, pts.shape[0]) and res["bary"].shape == (3, pts.shape[0], 2)
    for k in range(3):
        _assert_equals_restated({n: res[n][k] for n in ("dist", "face", "bary")}, ref[k], (builder, leaf_size, k))
        lo, nr = tracer.mesh_tri_offset[k], tracer.mesh_nr_tris[k]
        assert bool(((res["slot"][k] >= lo) & (res["slot"][k] < lo + nr)).all())
    assert torch.equal(tracer.slot_face_id[res["slot"].long()].long(), res["face"])
    one = tracer.closest(q, mesh_id=1)
    for n in ("dist", "face", "slot", "bary"):
        assert torch.equal(one[n], res[n][1]), n
    st = tracer.closest_stats(q)
    assert st["queries"] == 3 * pts.shape[0] and st["tri_tests"] >= st["queries"]
    assert st["tri_tests"] < st["queries"] * (80 + 320 + 1280) / 3          # the walk prunes


def _same_bits(a, b):
    """torch.equal on the bits: a float result with a NaN (the NaN query's) equals itself, and -0 is not +0."""
    if a.is_floating_point():
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@gpu
@pytest.mark.parametrize("builder", ["device", "ploc"])
def test_single_shell_queries_equal_their_row_of_the_all_shell_query(builder):
    """closest, signed_distance and winding_number of shell k are row k of their *_all form, every key, bit for bit:
    257 queries (four full waves and one lane of a fifth, where a [K, N] / [N] mix-up shows), one with a NaN."""
    from volsurfs_amd.mesh import icosphere
    from volsurfs_amd.raytrace import RayTracer
    K, N = 3, 257
    tracer = RayTracer([_mesh(*icosphere(2, 0.30 + 0.04 * k)) for k in range(K)], builder=builder)
    assert tracer.mesh_nr_tris == [320] * K
    pts = np.random.default_rng(29).uniform(-0.6, 0.6, (N, 3)).astype(np.float32)
    pts[100, 1] = np.nan
    q = torch.from_numpy(pts).cuda()
    every = tracer.closest_all(q)
    assert every["dist"].shape == (K, N) and every["bary"].shape == (K, N, 2) and bool((every["slot"][:, 100] == -1).all())
    signed = {s: tracer.signed_distance_all(q, sign=s) for s in ("pseudonormal", "winding")}
    wind = {b: tracer.winding_number_all(q, beta=b) for b in (2.0, math.inf)}
    assert wind[2.0].shape == (K, N) and bool(wind[2.0][:, 100].isnan().all())
    for k in range(K):
        pairs = [("closest", tracer.closest(q, k), every)]
        pairs += [(s, tracer.signed_distance(q, k, sign=s), signed[s]) for s in signed]
        for what, one, rows in pairs:
            assert sorted(one) == sorted(rows) == ["bary", "dist", "face", "slot"]
            for key in rows:
                assert _same_bits(one[key], rows[key][k]), (what, k, key)
        for b in wind:
            assert _same_bits(tracer.winding_number(q, k, beta=b), wind[b][k]), (b, k)
    for bad in (-1, K):
        for call in (tracer.closest, tracer.signed_distance, tracer.winding_number):
            with pytest.raises(_lib.VolsurfsHipError):
                call(q, bad)


@gpu
def test_non_convex_shells_equal_brute_force():
    """Lobed shells; half of the queries at radii between the lobes' troughs and crests, i.e. inside the concavities."""
    from volsurfs_amd import mesh_distance as MD
    from volsurfs_amd.mesh import stress_shells
    from volsurfs_amd.raytrace import RayTracer
    meshes = stress_shells(K=2, subdiv=4)
    rng = np.random.default_rng(5)
    radius = np.linalg.norm(meshes[0].vertices.cpu().numpy(), axis=1)
    d = rng.standard_normal((518, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    between = d * rng.uniform(radius.min(), radius.max(), (518, 1))
    pts = np.concatenate([rng.uniform(-0.5, 0.5, (519, 3)), between]).astype(np.float32)
    tracer = RayTracer(meshes, builder="device")
    q = torch.from_numpy(pts).cuda()
    res = tracer.closest_all(q)
    for k in range(2):
        ref = R.closest(pts, _records(meshes[k]), chunk=128)
        _assert_equals_restated({n: res[n][k] for n in ("dist", "face", "bary")}, ref, k)
    pos = MD.closest_positions(q, (tracer, 1)).cpu().numpy()
    assert np.array_equal(pos, R.sample_positions(tracer.tris.cpu().numpy(), res["slot"][1].cpu().numpy(),
                                                  res["bary"][1].cpu().numpy()))


@gpu
def test_point_cloud():
    """A scan as zero-area faces: index and distance equal the restatement, and the index is numpy's arg-min of the
    restated d2 (ties to the smallest index: ten points of the cloud are repeated and queried)."""
    from volsurfs_amd import mesh_distance as MD
    rng = np.random.default_rng(3)
    cloud = rng.uniform(-1.0, 1.0, (3000, 3)).astype(np.float32)
    cloud[2000:2010] = cloud[40:50]
    pts = rng.uniform(-1.1, 1.1, (1037, 3)).astype(np.float32)
    pts[:10] = cloud[40:50]
    mesh = MD.point_cloud_mesh(cloud)
    res = MD.closest_points(torch.from_numpy(pts).cuda(), mesh)
    rec = _records(mesh)
    ref = R.closest(pts, rec)
    assert np.array_equal(res["dist"].cpu().numpy(), ref["dist"])
    assert np.array_equal(res["face"].cpu().numpy(), ref["face"])
    d2, _, _ = R.closest_on_triangles(pts, rec)
    assert np.array_equal(res["face"].cpu().numpy(), d2.argmin(axis=1))
    assert np.array_equal(res["face"][:10].cpu().numpy(), np.arange(40, 50)) and not res["dist"][:10].any()
    # sampling a cloud is uniform over its points: n = P gives every point once
    p, face, _ = MD.sample_surface(mesh, 3000, seed=1)
    assert np.array_equal(np.sort(face.cpu().numpy()), np.arange(3000))
    assert np.array_equal(p.cpu().numpy(), cloud[face.cpu().numpy()])


@gpu
@pytest.mark.parametrize("n", [10000, 10037])
def test_sampler(n):
    from volsurfs_amd import mesh_distance as MD
    from volsurfs_amd.mesh import icosphere
    from volsurfs_amd.raytrace import RayTracer
    v, f = icosphere(3, 0.3)
    v = (v * np.array([1.0, 0.6, 0.3], np.float32)).astype(np.float32)          # unequal areas
    f = np.concatenate([f[:700], [[0, 0, 5]], f[700:]]).astype(np.int32)           # and one zero-area face, id 700
    tracer = RayTracer([_mesh(v, f)], builder="device")
    mesh = (tracer, 0)
    p, face, bary = MD.sample_surface(mesh, n, seed=7)
    p2, face2, bary2 = MD.sample_surface(mesh, n, seed=7)
    assert torch.equal(p, p2) and torch.equal(face, face2) and torch.equal(bary, bary2)      # same bytes
    p3, _, _ = MD.sample_surface(mesh, n, seed=8)
    assert not torch.equal(p, p3)
    u, w = bary[:, 0], bary[:, 1]
    assert bool((u >= 0).all()) and bool((w >= 0).all()) and bool((u + w <= 1).all())
    # the point is (v0 + u e1) + v e2 of the face's record, recomputed in numpy float32
    tris = tracer.tris.cpu().numpy()
    slot_of_face = np.empty(tris.shape[0], np.int64)
    slot_of_face[tracer.slot_face_id.cpu().numpy()] = np.arange(tris.shape[0])
    slot = slot_of_face[face.cpu().numpy()]
    assert np.array_equal(p.cpu().numpy(), R.sample_positions(tris, slot, bary.cpu().numpy()))
    # stratification: every face receives its share of the n samples to within 2 (one from the strata's ends, the rest
    # for the weights' quantisation and rounding)
    area = np.empty(tris.shape[0])
    area[tracer.slot_face_id.cpu().numpy()] = R.face_areas(tris)
    count = np.bincount(face.cpu().numpy(), minlength=tris.shape[0])
    assert area[700] == 0.0 and count[700] == 0
    assert count.sum() == n
    assert np.abs(count - n * area / area.sum()).max() < 2


@gpu
def test_fused_equals_unfused():
    from volsurfs_amd import mesh_distance as MD
    from volsurfs_amd.raytrace import RayTracer
    tracer = RayTracer(list(_three_shells()), builder="device")
    src, dst = (tracer, 0), (tracer, 2)
    n, th = 10037, (0.005, 0.02, 0.05)
    got = MD.surface_distance(src, dst, n=n, seed=3, thresholds=th)
    p, _, _ = MD.sample_surface(src, n, seed=3)
    ref = R.statistics(MD.closest_points(p, dst)["dist"].cpu().numpy(), th)
    assert got.n == n and got.min == ref["min"] and got.max == ref["max"] and got.within == ref["within"]
    assert 0 < got.within[2] and got.within[0] < n                     # the thresholds cut somewhere
    # n non-negative float64 terms added in another order: each partial sum is off by at most 2^-53 of the total per
    # addition, n - 1 additions: n 2^-52 with room
    tol = n * 2.0 ** -52
    assert abs(got.mean - ref["mean"]) <= tol * ref["mean"]
    assert abs(got.rms - ref["rms"]) <= tol * ref["rms"]
    composed = MD.surface_distance_unfused(src, dst, n=n, seed=3, thresholds=th)
    assert (composed.min, composed.max, composed.within) == (got.min, got.max, got.within)
    assert abs(composed.mean - got.mean) <= tol * got.mean
    assert MD.surface_distance(src, dst, n=n, seed=3, thresholds=th) == got                  # same bytes again


def _square(side, z):
    h = side / 2.0
    return _mesh([[-h, -h, z], [h, -h, z], [h, h, z], [-h, h, z]], [[0, 1, 2], [0, 2, 3]])


@gpu
def test_meaning():
    from volsurfs_amd import mesh_distance as MD
    from volsurfs_amd.mesh import icosphere, nested_shells
    # a mesh against itself
    sphere = _mesh(*icosphere(3, 0.3))
    res = MD.mesh_distance(sphere, sphere, n=10037, seed=1, thresholds=(1e-5,))
    extent = 0.6
    assert res["ab"].max <= 4 * 2.0 ** -24 * math.sqrt(3.0) * extent
    assert res["f_score"] == [1.0] and res["precision"] == [1.0] and res["recall"] == [1.0]
    # two parallel squares: from the small one every sample is exactly 0.25 below the large one
    small, large = _square(1.0, 0.0), _square(3.0, 0.25)
    st = MD.surface_distance(small, large, n=5037, seed=2, thresholds=(0.25,))
    assert (st.min, st.mean, st.rms, st.max) == (0.25, 0.25, 0.25, 0.25) and st.within == (5037,)
    back = MD.surface_distance(large, small, n=5037, seed=2)
    assert back.min == 0.25 and back.max > 1.0                          # the large square's corners are far
    # symmetry under swapping the arguments
    a, b = MD.mesh_distance(small, large, n=5037, seed=4), MD.mesh_distance(large, small, n=5037, seed=4)
    assert a["chamfer"] == b["chamfer"] and a["hausdorff"] == b["hausdorff"] and a["ab"] == b["ba"]
    ev = MD.evaluate_mesh(small, large, n=5037, seed=4)
    assert ev["accuracy"] == a["ab"].mean and ev["completeness"] == a["ba"].mean
    assert ev["overall"] == 0.5 * (a["ab"].mean + a["ba"].mean)
    # nested shells dr apart: neither pair touches, and no sample is farther than dr from its neighbour's vertices' shell
    dr = 0.01
    pairs = MD.shell_clearance(nested_shells(K=3, subdiv=3, dr=dr), n=5037, seed=0)
    assert [c["pair"] for c in pairs] == [(0, 1), (1, 2)]
    for c in pairs:
        assert 0.0 < c["out"].min <= dr and 0.0 < c["in"].min <= dr
    err = MD.simplification_error(sphere, _mesh(*icosphere(2, 0.3)), n=5037, seed=0)
    assert err["hausdorff_rel"] == err["hausdorff"] / err["diagonal"] and 0.0 < err["hausdorff_rel"] < 0.01
    assert abs(err["diagonal"] - 0.6 * math.sqrt(3.0)) < 1e-3


@gpu
def test_errors():
    from volsurfs_amd import mesh_distance as MD
    from volsurfs_amd.raytrace import RayTracer
    meshes = list(_three_shells())
    q = torch.zeros(5, 3, device="cuda")
    f32 = RayTracer(meshes[:1], node_format="f32")
    with pytest.raises(_lib.VolsurfsHipError, match="q16"):
        f32.closest_all(q)
    with pytest.raises(_lib.VolsurfsHipError, match="q16"):
        f32.closest(q)
    with pytest.raises(_lib.VolsurfsHipError, match="q16"):
        MD.surface_distance((f32, 0), meshes[1], n=100)
    tracer = RayTracer(meshes[:1], builder="device")
    for bad in (torch.zeros(5, 2, device="cuda"), torch.zeros(15, device="cuda"), torch.zeros(0, 3, device="cuda"),
                torch.zeros(5, 3, device="cuda", dtype=torch.float64), torch.zeros(5, 3, device="cuda", dtype=torch.int32)):
        with pytest.raises(_lib.VolsurfsHipError):
            tracer.closest_all(bad)
        with pytest.raises(_lib.VolsurfsHipError):
            MD.closest_points(bad, (tracer, 0))
    with pytest.raises(_lib.VolsurfsHipError):
        tracer.closest(q, mesh_id=1)
    for n in (0, -5):
        with pytest.raises(ValueError):
            MD.sample_surface(meshes[0], n)
        with pytest.raises(ValueError):
            MD.surface_distance(meshes[0], meshes[1], n=n)
        with pytest.raises(ValueError):
            MD.mesh_distance(meshes[0], meshes[1], n=n)
    with pytest.raises(ValueError):
        MD.surface_distance(meshes[0], meshes[1], n=10, thresholds=(-1.0,))
    with pytest.raises(ValueError):
        MD.surface_distance(meshes[0], meshes[1], n=10, thresholds=[0.1] * 9)
    with pytest.raises(TypeError):
        MD.surface_distance("mesh", meshes[1], n=10)
