"""Signed distance to a mesh on the device (volsurfs_amd/mesh_sdf.py, RayTracer.signed_distance*, csrc/mesh_sdf.hip;
DESIGN §29) against the restated rule (tests/mesh_sdf_restated.py) and, for the sign, against an independent one (the
float64 winding number).  The reference has no such stage.  Comparisons are exact equality unless a bound is derived
where it is used."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import mesh_sdf_restated as S
from volsurfs_amd import _lib

ERR_ARG = -1
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- CPU

def test_entry_points_declared_built_and_prototyped():
    names, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    P, I, LL, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    expected = {
        "vsa_mesh_pseudonormals_workspace_bytes": (LL, [LL, LL]),
        "vsa_mesh_pseudonormals": (I, [P, LL, P, LL, P, LL, P, P]),
        "vsa_signed_distance_q": (I, [P, P, P, P, I, I, P, P, P, LL, P, P, P, P]),
        "vsa_mesh_sdf_grid_workspace_bytes": (LL, [I, I, I]),
        "vsa_mesh_sdf_grid": (I, [P, P, I, P, I, P, LL, P, P, P, I, I, I, F, P, P, LL, P, P]),
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
    roots, frames = (ctypes.c_int32 * 1)(0), (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    base = (ctypes.c_longlong * 1)(0)

    for v, f in ((0, 4), (-1, 4), (4, 0), (4, -2)):
        assert L.vsa_mesh_pseudonormals_workspace_bytes(v, f) == ERR_ARG, (v, f)

    def tables(vertices=p, V=4, faces=p, F=4, ws=p, ws_bytes=1 << 20, table=p):
        return L.vsa_mesh_pseudonormals(vertices, V, faces, F, ws, ws_bytes, table, None)

    for kw in ({"vertices": None}, {"faces": None}, {"ws": None}, {"table": None}, {"V": 0}, {"V": -3}, {"F": 0},
               {"F": -1}):
        assert tables(**kw) == ERR_ARG, kw
        assert tables(**dict(kw, vertices=None, faces=None, ws=None, table=None)) == ERR_ARG, kw

    def signed(qnodes=p, tris=p, mesh_roots=roots, mesh_frames=frames, nr_meshes=1, max_depth=10, table=p,
               table_base=base, points=p, nr_points=5, dist=p, slot=p, bary=p):
        return L.vsa_signed_distance_q(qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth, table, table_base,
                                       points, nr_points, dist, slot, bary, None)

    for name in ("qnodes", "tris", "mesh_roots", "mesh_frames", "table", "table_base", "points", "dist", "slot"):
        assert signed(**{name: None}) == ERR_ARG, name
    null = dict(qnodes=None, tris=None, table=None, points=None, dist=None, slot=None, bary=None)
    assert signed(**null) == ERR_ARG
    for kw in ({"nr_meshes": 0}, {"nr_meshes": 17}, {"nr_meshes": -1}, {"nr_points": 0}, {"nr_points": -4},
               {"max_depth": 48}, {"max_depth": 99}, {"table_base": (ctypes.c_longlong * 1)(-1)}):
        assert signed(**kw) == ERR_ARG, kw
        assert signed(**dict(kw, **null)) == ERR_ARG, kw

    for shape in ((0, 4, 4), (4, 0, 4), (4, 4, -1)):
        assert L.vsa_mesh_sdf_grid_workspace_bytes(*shape) == ERR_ARG, shape

    def grid(qnodes=p, tris=p, root=0, frame=frames, depth=10, table=p, table_base=0, x=p, y=p, z=p, nx=5, ny=6, nz=7,
             band=0.1, out=p, ws=p, ws_bytes=1 << 20, counts=p):
        return L.vsa_mesh_sdf_grid(qnodes, tris, root, frame, depth, table, table_base, x, y, z, nx, ny, nz, band, out,
                                   ws, ws_bytes, counts, None)

    for name in ("qnodes", "tris", "frame", "table", "x", "y", "z", "out", "ws", "counts"):
        assert grid(**{name: None}) == ERR_ARG, name
    null = dict(qnodes=None, tris=None, table=None, x=None, y=None, z=None, out=None, ws=None)
    assert grid(**null) == ERR_ARG
    for kw in ({"root": -1}, {"depth": 48}, {"table_base": -1}, {"nx": 0}, {"ny": -2}, {"nz": 0}, {"band": 0.0},
               {"band": -0.5}, {"band": float("nan")}):
        assert grid(**kw) == ERR_ARG, kw
        assert grid(**dict(kw, **null)) == ERR_ARG, kw


# the triangle (0,0,0), (4,0,0), (0,4,0), and one dyadic query in each of the seven regions, above and below the plane:
# (region, point, d2, u, v), worked by hand from the rule (the table of tests/test_mesh_distance.py)
TRIANGLE_V = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
TRIANGLE_F = np.array([[0, 1, 2]], np.int32)
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
REGION_SIGN = np.where(REGION_POINTS[:, 2] > 0, 1.0, -1.0).astype(np.float32)


def test_restatement_fourteen_queries_by_hand():
    res = S.signed_distance(REGION_POINTS, TRIANGLE_V, TRIANGLE_F)
    assert [S.REGION_NAMES[c] for c in res["region"]] == [r[0] for r in REGIONS]
    assert np.array_equal(np.stack([res["d2"], res["u"], res["v"]], 1), REGION_EXPECTED)
    assert np.array_equal(res["dist"], REGION_SIGN * np.sqrt(REGION_EXPECTED[:, 0]))
    # the lone triangle's table: every edge has one face, every vertex one angle (pi/2, pi/4, pi/4) of the normal +z
    table = S.pseudonormal_table(TRIANGLE_V, TRIANGLE_F)[0]
    angles = np.array([np.pi / 2, np.pi / 4, np.pi / 4])
    assert not table[:, :2].any()
    assert np.allclose(table[:3, 2], angles, rtol=0, atol=2.0 ** -23) and np.array_equal(table[3:, 2], np.ones(4, np.float32))
    # a point of the surface: +0
    on = S.signed_distance(np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [2.0, 0.0, 0.0]], np.float32), TRIANGLE_V, TRIANGLE_F)
    assert not on["dist"].any() and not np.signbit(on["dist"]).any()


def _cpu_stress_shell():
    from volsurfs_amd.mesh import stress_shells
    m = stress_shells(K=1, subdiv=4, device="cpu")[0]
    return m.vertices.numpy(), m.faces.numpy()


def test_restated_sign_equals_winding_number_parity():
    """The restated sign against a rule that shares nothing with it, on closed outward-wound meshes: 1037 seeded
    uniform queries of [-0.5, 0.5]^3 each; no mismatch, and the cosine between the residual and the chosen
    pseudonormal stays away from 0 (the sign is no rounding decision)."""
    from volsurfs_amd.mesh import icosphere
    meshes = {"icosphere(1, 0.30)": icosphere(1, 0.30), "icosphere(3, 0.34)": icosphere(3, 0.34), "cube": S.cube(0.25),
              "stress_shells(K=1, subdiv=4)[0]": _cpu_stress_shell()}
    pts = np.random.default_rng(11).uniform(-0.5, 0.5, (1037, 3)).astype(np.float32)
    for name, (v, f) in meshes.items():
        assert S.signed_volume(v, f) > 0, name
        res = S.signed_distance(pts, v, f)
        w = S.winding_number(pts, v, f)
        assert np.abs(w - np.round(w)).max() < 1e-6 and set(np.round(w).astype(int)) <= {0, 1}, name
        inside = np.round(w).astype(int) == 1
        print(name, "min |cos|", np.abs(res["cos"]).min(), "inside", inside.sum(), "regions",
              np.bincount(res["region"], minlength=7))
        assert np.array_equal(res["dist"] < 0, inside), (name, int(((res["dist"] < 0) != inside).sum()))
        assert np.abs(res["cos"]).min() >= 0.5, name
        assert 0 < inside.sum() < 1037


def test_needle_needs_the_vertex_pseudonormal():
    """Off the apex of a thin tetrahedron, along each side face's normal: the apex is the closest point, the point is
    outside, and the face normal of another incident face says otherwise."""
    v, f = S.needle(0.05, 0.6)
    assert S.signed_volume(v, f) > 0
    fn = S.face_normals(v, f)
    apex = v[3].astype(np.float64)
    pts = np.stack([apex + 0.1 * fn[i] for i in (1, 2, 3)]).astype(np.float32)
    res = S.signed_distance(pts, v, f)
    closest = pts - res["r"]
    assert np.abs(closest - v[3]).max() <= 1e-6
    assert (res["dist"] > 0).all() and np.allclose(res["dist"], 0.1, rtol=0, atol=1e-6)
    for i in range(3):
        against = [float(res["r"][i].astype(np.float64) @ fn[j]) for j in (1, 2, 3)]
        assert min(against) < -0.01, against            # a face-normal rule that met this face would answer "inside"


# ---------------------------------------------------------------------------------------------------------- GPU

def _mesh(v, f):
    from volsurfs_amd.mesh import TensorMesh
    return TensorMesh(np.asarray(v, np.float32), np.asarray(f, np.int32), device="cuda")


def _vf(mesh):
    return mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()


@gpu
def test_fourteen_queries_on_the_device():
    from volsurfs_amd.raytrace import RayTracer
    far = np.float32(100.0)
    v = [[0, 0, 0], [4, 0, 0], [0, 4, 0], [far, far, far], [far + 4, far, far], [far, far + 4, far]]
    tracer = RayTracer([_mesh(v, [[0, 1, 2], [3, 4, 5]])], builder="device")
    res = tracer.signed_distance(torch.from_numpy(REGION_POINTS).cuda())
    assert np.array_equal(res["dist"].cpu().numpy(), REGION_SIGN * np.sqrt(REGION_EXPECTED[:, 0]))
    assert np.array_equal(res["bary"].cpu().numpy(), REGION_EXPECTED[:, 1:])
    assert (res["face"] == 0).all()
    nan = tracer.signed_distance(torch.tensor([[float("nan"), 0.0, 0.0]], device="cuda"))
    assert int(nan["slot"][0]) == -1 and float(nan["dist"][0]) == math.inf


def _open_mesh():
    """A square of two faces plus one zero-area face (three collinear vertices, id 2) hung on its edge 1-2: the edges
    0-1, 0-3, 2-3 and 1-4, 4-2 are boundaries, the diagonal 0-2 has two faces, 1-2 has two of which one is null."""
    v = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [1, 0.5, 0]]
    return np.array(v, np.float32), np.array([[0, 1, 2], [0, 2, 3], [1, 4, 2]], np.int32)


@gpu
@pytest.mark.parametrize("name", ["icosphere", "cube", "needle", "open"])
def test_tables_equal_restated(name):
    """Each vector within 4 x 2^-24 of its own length of the restated one: both are float64 sums of at most a ring's
    length of terms whose roundings (and the two atan2) differ by ~2^-50, so the float32 roundings differ by a unit at
    the most.  The face's own normal, two roundings of the same value, is equal."""
    from volsurfs_amd import mesh_sdf as MS
    from volsurfs_amd.mesh import icosphere
    v, f = {"icosphere": lambda: icosphere(2, 0.32), "cube": S.cube, "needle": S.needle, "open": _open_mesh}[name]()
    mesh = _mesh(v, f)
    got = MS.pseudonormals(mesh)
    assert got.shape == (f.shape[0], 7, 3) and got.dtype == torch.float32
    assert torch.equal(got, MS.pseudonormals(mesh))                                      # same bytes
    ref = S.pseudonormal_table(v, f)
    g = got.cpu().numpy()
    err = np.abs(g.astype(np.float64) - ref).max(-1)
    assert (err <= 4 * 2.0 ** -24 * np.linalg.norm(ref.astype(np.float64), axis=-1)).all(), err.max()
    if name == "open":
        null = g[2]                                            # the null face (1, 4, 2): no normal of its own, none on
        assert not null[[S.IN, S.AB, S.BC, S.B]].any()         # the edges and the vertex that only it names, ...
        assert np.array_equal(null[S.AC], g[0, S.IN])          # ... face 0's on the edge 1-2 it hangs on, ...
        assert np.array_equal(g[0, S.BC], g[0, S.IN])          # ... to which it adds nothing
        assert np.array_equal(g[0, S.AB], g[0, S.IN])          # a boundary edge: its one face
        assert np.array_equal(g[0, S.AC], g[0, S.IN] + g[1, S.IN])


@functools.lru_cache(maxsize=None)
def _three_shells():
    from volsurfs_amd.mesh import icosphere
    return tuple(_mesh(*icosphere(s, r)) for s, r in ((1, 0.30), (2, 0.32), (3, 0.34)))


@functools.lru_cache(maxsize=None)
def _three_shell_queries():
    """1037 random points of [-0.5, 0.5]^3, every vertex of the largest shell (on it: +0), the centre and one point 10
    extents away, with the restated answer per shell, computed once."""
    large = _three_shells()[2]
    rng = np.random.default_rng(11)
    pts = np.concatenate([rng.uniform(-0.5, 0.5, (1037, 3)).astype(np.float32), large.vertices.cpu().numpy(),
                          np.zeros((1, 3), np.float32), np.array([[6.8, 0.1, -0.2]], np.float32)])
    return pts, tuple(S.signed_distance(pts, *_vf(m)) for m in _three_shells())


@functools.lru_cache(maxsize=None)
def _lobed_shells():
    from volsurfs_amd.mesh import stress_shells
    return tuple(stress_shells(K=2, subdiv=4))


@functools.lru_cache(maxsize=None)
def _lobed_queries():
    meshes = _lobed_shells()
    rng = np.random.default_rng(5)
    radius = np.linalg.norm(meshes[0].vertices.cpu().numpy(), axis=1)
    d = rng.standard_normal((518, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    between = d * rng.uniform(radius.min(), radius.max(), (518, 1))
    pts = np.concatenate([rng.uniform(-0.5, 0.5, (519, 3)), between]).astype(np.float32)
    return pts, tuple(S.signed_distance(pts, *_vf(m), chunk=128) for m in meshes)


def _assert_signed_equals(tracer, pts, ref, what):
    q = torch.from_numpy(pts).cuda()
    res, plain = tracer.signed_distance_all(q), tracer.closest_all(q)
    for n in ("face", "slot", "bary"):
        assert torch.equal(res[n], plain[n]), (what, n)
    assert torch.equal(res["dist"].abs(), plain["dist"]), what
    for k in range(tracer.nr_meshes):
        d = res["dist"][k].cpu().numpy()
        assert np.array_equal(np.abs(d), ref[k]["unsigned"]), (what, k)
        sure = np.abs(ref[k]["cos"]) >= 0.01
        assert (~sure).sum() <= 0.01 * pts.shape[0], (what, k, int((~sure).sum()))
        assert np.array_equal(np.signbit(d)[sure], np.signbit(ref[k]["dist"])[sure]), (what, k)
        on = ref[k]["d2"] == 0
        assert not d[on].any() and not np.signbit(d[on]).any(), (what, k)
    one = tracer.signed_distance(q, mesh_id=1)
    for n in ("dist", "face", "slot", "bary"):
        assert torch.equal(one[n], res[n][1]), (what, n)
    return res


@gpu
@pytest.mark.parametrize("builder,leaf_size", [("host", 4), ("device", 1), ("ploc", 8)])
def test_signed_equals_closest_and_restated_sign(builder, leaf_size):
    from volsurfs_amd.raytrace import RayTracer
    pts, ref = _three_shell_queries()
    tracer = RayTracer(list(_three_shells()), leaf_size=leaf_size, builder=builder)
    res = _assert_signed_equals(tracer, pts, ref, (builder, leaf_size))
    on = res["dist"][2][1037:1037 + 642]                        # the largest shell's own vertices
    assert not on.any() and not torch.signbit(on).any()
    assert float(res["dist"][0][-2]) < 0 < float(res["dist"][0][-1])       # the centre, the far point
    lobed_pts, lobed_ref = _lobed_queries()
    _assert_signed_equals(RayTracer(list(_lobed_shells()), leaf_size=leaf_size, builder=builder), lobed_pts, lobed_ref,
                          (builder, leaf_size, "lobed"))


@gpu
def test_needle_and_cube_features_on_the_device():
    from volsurfs_amd import mesh_sdf as MS
    v, f = S.needle(0.05, 0.6)
    fn = S.face_normals(v, f)
    pts = np.stack([v[3].astype(np.float64) + 0.1 * fn[i] for i in (1, 2, 3)]).astype(np.float32)
    ref = S.signed_distance(pts, v, f)
    res = MS.signed_distance(torch.from_numpy(pts).cuda(), _mesh(v, f))
    assert np.array_equal(res["dist"].cpu().numpy(), ref["dist"]) and (res["dist"] > 0).all()
    # the cube: off every corner along the diagonal and off every edge's midpoint along its bisector, outside and inside
    cv, cf = S.cube(0.25)
    corners = cv.astype(np.float64)
    mids = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)
                     if (x == 0) + (y == 0) + (z == 0) == 1], np.float64) * 0.25
    q = np.concatenate([corners * 1.5, corners * 0.75, mids * 1.5, mids * 0.75]).astype(np.float32)
    ref = S.signed_distance(q, cv, cf)
    assert set(ref["region"][:8]) <= {S.A, S.B, S.C} and S.IN not in set(ref["region"][16:28])
    assert np.abs(ref["cos"]).min() > 0.5
    got = MS.signed_distance(torch.from_numpy(q).cuda(), _mesh(cv, cf))["dist"].cpu().numpy()
    assert np.array_equal(got, ref["dist"])
    outside = np.concatenate([np.ones(8, bool), np.zeros(8, bool), np.ones(12, bool), np.zeros(12, bool)])
    assert np.array_equal(got > 0, outside)
    inside = MS.contains(torch.from_numpy(q).cuda(), _mesh(cv, cf)).cpu().numpy()
    assert np.array_equal(inside, ~outside)


@gpu
@pytest.mark.parametrize("shape", ["sphere", "lobed"])
def test_grid_equals_point_queries(shape):
    """The lattice kernel against `sample_grid` of the point query, bit for bit; n = 22 leaves a partial brick on every
    axis.  The banded grid is the clamp of the full one, with some bricks far and some near."""
    from volsurfs_amd import mesh_sdf as MS
    from volsurfs_amd.isosurface import sample_grid
    from volsurfs_amd.mesh import icosphere
    from volsurfs_amd.raytrace import RayTracer
    mesh = _mesh(*icosphere(3, 0.34)) if shape == "sphere" else _lobed_shells()[0]
    handle = (RayTracer([mesh], builder="device"), 0)
    n, r = 22, (1.0 if shape == "sphere" else 0.6)
    full, counts = MS.mesh_to_sdf_grid(handle, n, r)
    assert counts == {"near_bricks": 6 ** 3, "far_bricks": 0}
    ref = sample_grid(lambda p: MS.signed_distance(p, handle)["dist"], n, r)
    assert torch.equal(full, ref)
    assert bool((full < 0).any()) and bool((full > 0).any())
    band = 0.1
    banded, counts = MS.mesh_to_sdf_grid(handle, n, r, band=band)
    assert torch.equal(banded, full.clamp(-band, band))
    assert 0 < counts["far_bricks"] < 6 ** 3 and counts["near_bricks"] + counts["far_bricks"] == 6 ** 3
    again, counts2 = MS.mesh_to_sdf_grid(handle, n, r, band=band)
    assert torch.equal(again, banded) and counts2 == counts                               # same bytes


@gpu
def test_grid_with_three_different_axes():
    from volsurfs_amd import mesh_sdf as MS
    from volsurfs_amd.mesh import icosphere
    from volsurfs_amd.raytrace import RayTracer
    handle = (RayTracer([_mesh(*icosphere(2, 0.3))], builder="device"), 0)
    x = torch.linspace(-0.5, 0.4, 9, device="cuda")
    y = torch.tensor([-0.45, -0.2, -0.1, 0.05, 0.3, 0.31], device="cuda")
    z = torch.linspace(-0.6, 0.6, 14, device="cuda")
    pts = torch.stack(torch.meshgrid(x, y, z, indexing="ij"), -1).reshape(-1, 3)
    ref = MS.signed_distance(pts, handle)["dist"].reshape(9, 6, 14)
    full, counts = MS.sdf_grid(handle, x, y, z)
    assert torch.equal(full, ref) and counts == {"near_bricks": 3 * 2 * 4, "far_bricks": 0}
    banded, counts = MS.sdf_grid(handle, x, y, z, band=0.05)
    assert torch.equal(banded, ref.clamp(-0.05, 0.05)) and counts["near_bricks"] + counts["far_bricks"] == 24


def _closed(mesh):
    """One cluster, every edge on exactly two faces."""
    from volsurfs_amd.mesh_clean import cluster_connected_triangles
    f = mesh.faces.cpu().numpy().astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, count = np.unique(e, axis=0, return_counts=True)
    return bool((count == 2).all()) and int(cluster_connected_triangles(mesh)[1].numel()) == 1


@gpu
def test_round_trip_through_marching_cubes():
    """Level 0 of the field of a mesh is the mesh again, to within a cell's diagonal: the field is 1-Lipschitz and a
    marching-cubes vertex lies on a grid edge whose ends have different signs, so the surface crosses that edge, and
    the vertex is within the edge's length of the crossing; the other way every surface point lies in a cell with a
    sign change, whose extracted vertices are within its diagonal."""
    from volsurfs_amd import mesh_sdf as MS
    from volsurfs_amd.isosurface import _lattice, marching_cubes
    from volsurfs_amd.mesh import icosphere
    from volsurfs_amd.mesh_distance import mesh_distance
    src = _mesh(*icosphere(3, 0.34))
    n, r = 48, 0.5
    grid, _ = MS.mesh_to_sdf_grid(src, n, r)
    origin, spacing = _lattice(n, r)
    out = marching_cubes(grid, [0.0], origin, spacing)[0]
    assert out.faces.shape[0] > 0 and _closed(out)
    res = mesh_distance(out, src, n=20037, seed=1)
    print("hausdorff", res["hausdorff"], "cell diagonal", math.sqrt(3.0) * spacing[0])
    assert res["hausdorff"] <= math.sqrt(3.0) * spacing[0]


@gpu
def test_offset_shells_are_nested(tmp_path):
    from volsurfs_amd import mesh_sdf as MS
    from volsurfs_amd.mesh import icosphere, level_files, load_ply, save_ply
    src = _mesh(*icosphere(3, 0.30))
    n, r, delta = 48, 0.5, 0.05
    diag = math.sqrt(3.0) * 2.0 * r / (n - 1)
    meshes, levels = MS.offset_shells(src, 3, delta_surfs=delta, nr_points_per_dim=n, scene_radius=r)
    assert levels == [-0.05, 0.0, 0.05] and len(meshes) == 3
    nesting = MS.shell_nesting(meshes, n=5037, seed=0)
    assert [c["pair"] for c in nesting] == [(0, 1), (1, 2)]
    for c in nesting:
        print(c, "bound", delta - diag)
        assert c["outside"] == 0 and c["clearance"] >= delta - diag
    probe = torch.tensor([[0.0, 0.0, 0.0], [-r, -r, -r]], device="cuda")
    for m in meshes:
        assert MS.contains(probe, m).cpu().tolist() == [True, False]
    with pytest.raises(ValueError, match="band"):
        MS.offset_shells(src, 3, delta_surfs=delta, nr_points_per_dim=n, scene_radius=r, band=0.05)
    path = str(tmp_path / "source.ply")
    save_ply(path, src)
    paths, levels2 = MS.offset_meshes(path, str(tmp_path / "run"), 3, delta_surfs=delta, nr_points_per_dim=n,
                                      scene_radius=r)
    assert levels2 == levels
    names = level_files(str(tmp_path / "run" / "meshes"))
    assert names == ["-0.05.ply", "0.0.ply", "0.05.ply"] and [p.split("/")[-1] for p in paths] == names
    for name, m in zip(names, meshes):
        back = load_ply(str(tmp_path / "run" / "meshes" / name))
        assert torch.equal(back.vertices, m.vertices) and torch.equal(back.faces, m.faces)


@gpu
def test_errors_and_refit():
    from volsurfs_amd import mesh_sdf as MS
    from volsurfs_amd.mesh import icosphere
    from volsurfs_amd.raytrace import RayTracer
    meshes = list(_three_shells())
    q = torch.from_numpy(_three_shell_queries()[0][:300]).cuda()
    f32 = RayTracer(meshes[:1], node_format="f32")
    for call in (lambda: f32.signed_distance_all(q), lambda: f32.signed_distance(q),
                 lambda: MS.signed_distance(q, (f32, 0)), lambda: MS.mesh_to_sdf_grid((f32, 0), 8)):
        with pytest.raises(_lib.VolsurfsHipError, match="q16"):
            call()
    tracer = RayTracer(meshes[:1], builder="device")
    with pytest.raises(_lib.VolsurfsHipError):
        tracer.signed_distance(q, mesh_id=1)
    with pytest.raises(_lib.VolsurfsHipError):
        tracer.signed_distance_all(torch.zeros(5, 2, device="cuda"))
    for band in (0.0, -1.0):
        with pytest.raises(ValueError):
            MS.mesh_to_sdf_grid((tracer, 0), 8, band=band)
    with pytest.raises(TypeError):
        MS.signed_distance(q, "mesh")
    # refit: the tables follow the geometry
    for builder in ("host", "device"):
        tracer = RayTracer([_mesh(*icosphere(2, 0.2))], builder=builder)
        before = tracer.signed_distance(q)["dist"]
        moved = _mesh(*icosphere(2, 0.4))
        tracer.refit([moved])
        after = tracer.signed_distance(q)
        fresh = RayTracer([moved], builder=builder).signed_distance(q)
        assert torch.equal(after["dist"], fresh["dist"]) and torch.equal(after["face"], fresh["face"])
        assert not torch.equal(after["dist"], before) and bool(((after["dist"] < 0) != (before < 0)).any())
