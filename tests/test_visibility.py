"""Faces no view can see (volsurfs_amd/visibility.py, csrc/face_visibility.hip).  The reference leaves the
stage a stub, so the counts are checked against this library's own tested parts: the composition get_camera_rays +
RayTracer.trace_all + bincount, and the brute-force oracle.  Every comparison is exact equality."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from volsurfs_amd import _lib

ERR_ARG = -1
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- CPU

def test_entry_points_declared_built_and_prototyped():
    names, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("vsa_face_view_counts", "vsa_face_ring_dilate"):
        assert n in names, f"{n} is not declared in include/volsurfs_hip.h"
        assert hasattr(cdll, n), f"{n} is not in the built library"
        assert n in protos, f"{n} got no prototype"
    P, I, F, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    assert protos["vsa_face_view_counts"] == (I, [P, P, P, P, I, I, P, P, I, I, I, I, F, P, P, P])
    assert protos["vsa_face_ring_dilate"] == (I, [P, LL, LL, P, I, P, P])


def test_argument_errors_before_any_hip_call():
    """Every VSA_ERR_ARG case of the two entry points.  The "device" pointers are null or the address of a host buffer
    nothing reads: each call must return before it touches the GPU (this test runs without one)."""
    L = _lib.lib()
    buf = (ctypes.c_longlong * 16)()
    p = ctypes.addressof(buf)                      # a non-null pointer; never dereferenced on the device
    roots, frames = (ctypes.c_int32 * 1)(0), (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    base = (ctypes.c_longlong * 1)(0)

    def counts(qnodes=p, tris=p, mesh_roots=roots, mesh_frames=frames, nr_meshes=1, max_depth=10, c2w=p, kinv=p,
               nr_views=1, height=4, width=4, supersample=1, t_min=0.0, face_base=base, out=p):
        return L.vsa_face_view_counts(qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth, c2w, kinv, nr_views,
                                      height, width, supersample, t_min, face_base, out, None)

    for name in ("qnodes", "tris", "mesh_roots", "mesh_frames", "c2w", "kinv", "face_base", "out"):
        assert counts(**{name: None}) == ERR_ARG, name
    # with null device pointers throughout, as a caller without a GPU would have them
    assert counts(qnodes=None, tris=None, c2w=None, kinv=None, out=None) == ERR_ARG
    for kw in ({"nr_meshes": 0}, {"nr_meshes": -1}, {"nr_views": 0}, {"height": 0}, {"width": 0}, {"width": -3},
               {"supersample": 0}, {"supersample": 9}, {"max_depth": 48}, {"max_depth": 99},
               {"nr_views": 1024, "height": 2048, "width": 2048},                    # exactly 2^32 samples
               {"nr_views": 1, "height": 32768, "width": 32768, "supersample": 2},   # 2^30 pixels x 4
               {"nr_views": 1 << 20, "height": 1 << 20, "width": 1 << 20},           # beyond 64 bits if multiplied blindly
               {"nr_views": 65536, "height": 8192, "width": 8192, "supersample": 8}):
        assert counts(**kw) == ERR_ARG, kw
        null_kw = dict(kw, qnodes=None, tris=None, c2w=None, kinv=None, out=None)
        assert counts(**null_kw) == ERR_ARG, kw

    def dilate(faces=p, nr_faces=4, nr_verts=4, keep=p, rings=1, scratch=p):
        return L.vsa_face_ring_dilate(faces, nr_faces, nr_verts, keep, rings, scratch, None)

    for kw in ({"faces": None}, {"keep": None}, {"scratch": None}, {"nr_faces": 0}, {"nr_verts": 0}, {"rings": -1},
               {"rings": 17}):
        assert dilate(**kw) == ERR_ARG, kw
        assert dilate(**dict(kw, faces=None, keep=None, scratch=None)) == ERR_ARG, kw


# ---------------------------------------------------------------------------------------------------------- GPU

H, W = 37, 45                      # neither a multiple of 8 nor of 64


def _sphere(subdiv, radius):
    from volsurfs_amd.mesh import TensorMesh, icosphere
    v, f = icosphere(subdiv, radius)
    return TensorMesh(v, f, device="cuda")


def _cam(eye, target=(0.0, 0.0, 0.0), focal=40.0, height=H, width=W, up=(0.0, -1.0, 0.0)):
    from volsurfs_amd.camera import Camera
    return Camera.look_at(eye, target, up=up, focal=focal, height=height, width=width)


@functools.lru_cache(maxsize=None)
def _two_shells():
    return tuple(_sphere(2, r) for r in (0.30, 0.32))


@functools.lru_cache(maxsize=None)
def _three_views():
    """Outside with part of the image missing the shells; inside both shells; outside, off axis."""
    return (_cam((0.0, 0.0, -1.2)), _cam((0.05, 0.02, 0.10), target=(1.0, 0.3, 0.2)), _cam((0.9, 0.7, 0.5), focal=60.0))


def _six_axis_cameras(size=64, focal=120.0, dist=1.5):
    cams = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            eye = [0.0, 0.0, 0.0]
            eye[axis] = sign * dist
            cams.append(_cam(tuple(eye), focal=focal, height=size, width=size,
                             up=(0.0, 0.0, 1.0) if axis == 1 else (0.0, -1.0, 0.0)))
    return cams


def _composition(tracer, nr_faces, cameras):
    """The counts from the existing calls: rays to memory, trace_all, original face ids gathered, bincount per view."""
    from volsurfs_amd.camera import get_camera_rays
    out = [torch.zeros(n, dtype=torch.int64, device="cuda") for n in nr_faces]
    for cam in cameras:
        o, d, _ = get_camera_rays(cam)
        _, slot, _ = tracer.trace_all(o, d)
        for k, n in enumerate(nr_faces):
            s = slot[k]
            ids = tracer.slot_face_id[s[s >= 0].long()].long()
            out[k] += torch.bincount(ids, minlength=n)
    return out


@functools.lru_cache(maxsize=None)
def _reference_counts():
    """Composition counts of the two shells from the three views (host-built tracer), computed once."""
    from volsurfs_amd.raytrace import RayTracer
    meshes = _two_shells()
    tracer = RayTracer(list(meshes), builder="host")
    return tuple(_composition(tracer, [int(m.faces.shape[0]) for m in meshes], _three_views()))


@gpu
@pytest.mark.parametrize("builder", ["host", "device", "ploc"])
def test_equals_the_composition(builder):
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.visibility import face_view_counts
    meshes, cams = list(_two_shells()), list(_three_views())
    tracer = RayTracer(meshes, builder=builder)
    assert tracer.node_format == "q16"
    got = face_view_counts(meshes, cams, tracer=tracer)
    want = _composition(tracer, [320, 320], cams)
    assert len(got) == 2
    for k in range(2):
        assert got[k].dtype == torch.int64 and tuple(got[k].shape) == (320,)
        assert torch.equal(got[k], want[k]), (builder, k)
        assert torch.equal(got[k], _reference_counts()[k]), (builder, k)
        assert torch.equal(tracer.face_view_counts(cams)[k], want[k])
    total = int(sum(int(g.sum()) for g in got))
    assert 0 < total < 2 * 3 * H * W                    # some rays hit, some miss
    assert int(got[0].sum()) >= H * W                   # the camera inside hits with every pixel


@gpu
def test_default_tracer_and_f32_nodes_refused():
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.visibility import face_view_counts
    meshes, cams = list(_two_shells()), list(_three_views())
    got = face_view_counts(meshes, cams)
    for k in range(2):
        assert torch.equal(got[k], _reference_counts()[k])
    with pytest.raises(_lib.VolsurfsHipError, match="q16"):
        face_view_counts(meshes, cams, tracer=RayTracer(meshes, node_format="f32"))


@gpu
def test_equals_the_bruteforce_oracle():
    from oracle.raytrace import trace_bruteforce
    from volsurfs_amd.camera import get_camera_rays
    from volsurfs_amd.visibility import face_view_counts
    mesh = _two_shells()[1]
    cam = _cam((0.3, -0.2, -1.0), focal=30.0, height=20, width=24)
    o, d, _ = get_camera_rays(cam)
    hit = trace_bruteforce(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), o.cpu().numpy(), d.cpu().numpy(), 0.0)
    tri = hit["tri"]
    want = np.bincount(tri[tri >= 0], minlength=320)
    got = face_view_counts([mesh], [cam])[0].cpu().numpy()
    assert 0 < want.sum() < 20 * 24
    assert np.array_equal(got, want)


@gpu
def test_supersampling_equals_the_doubled_image():
    from volsurfs_amd.visibility import face_view_counts
    mesh = _two_shells()[0]
    h, w = 20, 18
    small = _cam((0.4, 0.3, -1.0), focal=22.0, height=h, width=w)
    big = _cam((0.4, 0.3, -1.0), focal=44.0, height=2 * h, width=2 * w)
    # Kinv . diag(1/2, 1/2, 1): halving is exact in fp32, so the doubled image's pixel centres are the same rays
    big.intrinsics_inv = (small.intrinsics_inv * torch.tensor([0.5, 0.5, 1.0], device="cuda")).contiguous()
    big.c2w = small.c2w.clone()
    a = face_view_counts([mesh], [small], supersample=2)[0]
    b = face_view_counts([mesh], [big], supersample=1)[0]
    assert 0 < int(a.sum()) < 4 * h * w
    assert torch.equal(a, b)
    assert not torch.equal(a, face_view_counts([mesh], [small], supersample=1)[0])


def _outward_normals_and_centroids(mesh):
    v, f = mesh.vertices.double(), mesh.faces.long()
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = torch.linalg.cross(p1 - p0, p2 - p0)
    c = (p0 + p1 + p2) / 3.0
    n = n * torch.sign((n * c).sum(1, keepdim=True))          # a sphere about the origin: outward is along the centroid
    return n, c


@gpu
def test_meaning_one_camera_sees_only_faces_that_face_it():
    from volsurfs_amd.visibility import face_view_counts
    mesh = _sphere(1, 0.3)
    eye = (0.0, 0.0, -1.5)
    counts = face_view_counts([mesh], [_cam(eye, focal=120.0, height=64, width=64)])[0]
    assert tuple(counts.shape) == (80,)
    n, c = _outward_normals_and_centroids(mesh)
    facing = (n * (torch.tensor(eye, dtype=torch.float64, device="cuda") - c)).sum(1) > 0
    assert bool((counts > 0).any()) and bool((counts == 0).any())
    assert bool(facing[counts > 0].all())


@gpu
def test_meaning_six_cameras_see_every_face_and_never_the_inner_sphere():
    from volsurfs_amd.mesh import TensorMesh, icosphere
    from volsurfs_amd.visibility import face_view_counts, remove_invisible_faces
    cams = _six_axis_cameras()
    outer = _sphere(1, 0.3)
    assert bool((face_view_counts([outer], cams)[0] > 0).all())
    vo, fo = icosphere(1, 0.3)
    vi, fi = icosphere(1, 0.15)
    both = TensorMesh(np.concatenate([vo, vi]), np.concatenate([fo, fi + vo.shape[0]]), device="cuda")
    counts = face_view_counts([both], cams)[0]
    assert bool((counts[:80] > 0).all()) and bool((counts[80:] == 0).all())
    culled, stats = remove_invisible_faces([both], cams, rings=0, return_stats=True)
    assert torch.equal(culled[0].vertices, outer.vertices) and torch.equal(culled[0].faces, outer.faces)
    assert stats[0] == {"faces_in": 160, "faces_out": 80, "vertices_in": 84, "vertices_out": 42, "faces_seen": 80,
                        "hits": int(counts.sum())}


def _dilate_numpy(faces, nr_verts, mask, rings):
    mask = mask.copy()
    for _ in range(rings):
        flagged = np.zeros(nr_verts, bool)
        flagged[faces[mask].reshape(-1)] = True
        mask = flagged[faces].any(1)
    return mask


@gpu
def test_ring_dilation():
    from volsurfs_amd.visibility import visible_face_mask
    mesh = _two_shells()[0]
    faces, nv = mesh.faces.cpu().numpy(), int(mesh.vertices.shape[0])
    rng = np.random.default_rng(11)
    for density in (0.02, 0.3):
        mask = rng.random(320) < density
        assert mask.any()
        grown = []
        for rings in (0, 1, 2, 3):
            got = visible_face_mask(mesh, torch.from_numpy(mask.astype(np.int64)).cuda(), min_hits=1, rings=rings)
            assert got.dtype == torch.bool
            assert np.array_equal(got.cpu().numpy(), _dilate_numpy(faces, nv, mask, rings)), (density, rings)
            grown.append(int(got.sum()))
        assert grown[0] == int(mask.sum()) and grown[0] < grown[1] <= grown[2] <= grown[3]
    none = torch.zeros(320, dtype=torch.int64, device="cuda")
    for rings in (0, 1, 3):
        assert not bool(visible_face_mask(mesh, none, rings=rings).any())
    # min_hits is a threshold on the counts
    c = torch.arange(320, device="cuda")
    assert torch.equal(visible_face_mask(mesh, c, min_hits=100, rings=0), c >= 100)
    with pytest.raises(ValueError):
        visible_face_mask(mesh, none, rings=17)


@gpu
def test_attributes_are_carried():
    from volsurfs_amd import mesh_clean
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.visibility import face_view_counts, remove_invisible_faces, visible_face_mask
    mesh = nested_shells(K=1, subdiv=2, atlas_charts=8)[0]
    cams = [_cam((0.0, 0.0, -1.2))]
    colors = torch.from_numpy(np.random.default_rng(3).random((mesh.vertices.shape[0], 3)).astype(np.float32)).cuda()
    got, got_colors = remove_invisible_faces([mesh], cams, vertex_colors=[colors])
    mask = visible_face_mask(mesh, face_view_counts([mesh], cams)[0])
    assert 0 < int(mask.sum()) < 320
    want = mesh_clean.remove_unreferenced_vertices(mesh_clean.remove_triangles_by_mask(mesh, ~mask))
    assert torch.equal(got[0].vertices, want.vertices) and torch.equal(got[0].faces, want.faces)
    assert got[0].has_uvs and torch.equal(got[0].faces_uvs, want.faces_uvs)
    assert torch.equal(got[0].faces_uvs, mesh.faces_uvs[mask])
    referenced = torch.zeros(mesh.vertices.shape[0], dtype=torch.bool, device="cuda")
    referenced[mesh.faces[mask].long().reshape(-1)] = True
    assert torch.equal(got_colors[0], colors[referenced])
    assert torch.equal(got[0].vertices, mesh.vertices[referenced])


@gpu
def test_culling_keeps_every_pixel_centre_hit():
    from volsurfs_amd.camera import get_camera_rays
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.visibility import remove_invisible_faces
    meshes, cams = list(_two_shells()), list(_three_views())
    culled, stats = remove_invisible_faces(meshes, cams, min_hits=1, rings=0, return_stats=True)
    full_tracer, culled_tracer = RayTracer(meshes, builder="device"), RayTracer(culled, builder="device")
    kept = [torch.nonzero(c >= 1).reshape(-1) for c in _reference_counts()]      # culled face -> original face
    for k in range(2):
        assert culled[k].faces.shape[0] == kept[k].shape[0] == stats[k]["faces_out"] < 320
    for cam in cams:
        o, d, _ = get_camera_rays(cam)
        t_full, slot_full, _ = full_tracer.trace_all(o, d)
        t_cull, slot_cull, _ = culled_tracer.trace_all(o, d)
        assert torch.equal(t_full.view(torch.int32), t_cull.view(torch.int32))
        assert torch.equal(slot_full >= 0, slot_cull >= 0)
        for k in range(2):
            hit = slot_full[k] >= 0
            id_full = full_tracer.slot_face_id[slot_full[k][hit].long()].long()
            id_cull = culled_tracer.slot_face_id[slot_cull[k][hit].long()].long()
            assert torch.equal(kept[k][id_cull], id_full)


@gpu
def test_deterministic_and_stream_independent():
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.visibility import face_view_counts, set_tile
    meshes, cams = list(_two_shells()), list(_three_views())
    tracer = RayTracer(meshes, builder="device")
    a = face_view_counts(meshes, cams, tracer=tracer)
    b = face_view_counts(meshes, cams, tracer=tracer)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = face_view_counts(meshes, cams, tracer=tracer)
    side.synchronize()
    try:
        set_tile("row")
        r = face_view_counts(meshes, cams, tracer=tracer)
    finally:
        set_tile("8x8")
    for k in range(2):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) and torch.equal(a[k], r[k])
        assert torch.equal(a[k], _reference_counts()[k])


@gpu
def test_directory_stage(tmp_path):
    from volsurfs_amd.mesh import TensorMesh, load_mesh, nested_shells, save_obj, save_ply
    from volsurfs_amd.visibility import cull_meshes, remove_invisible_faces
    src, dst = tmp_path / "meshes_cleaned", tmp_path / "meshes_visible"
    os.makedirs(src)
    for name, m in zip(("0.30.ply", "0.32.ply"), _two_shells()):
        save_ply(str(src / name), TensorMesh(m.vertices, m.faces, None, device="cuda"))
    save_obj(str(src / "0.34.obj"), nested_shells(K=1, subdiv=2, r0=0.34, atlas_charts=8)[0])
    cams = [_cam((0.0, 0.0, -1.2)), _cam((0.9, 0.7, 0.5), focal=60.0)]
    paths = cull_meshes(str(src), cams, str(dst))
    names = ["0.30.ply", "0.32.ply", "0.34.obj"]
    assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(dst)) == names
    inputs = [load_mesh(str(src / n)) for n in names]
    assert [m.has_uvs for m in inputs] == [False, False, True]
    want = remove_invisible_faces(inputs, cams)
    for n, w, m in zip(names, want, inputs):
        got = load_mesh(str(dst / n))
        assert 0 < got.faces.shape[0] < m.faces.shape[0], n
        assert torch.equal(got.vertices, w.vertices) and torch.equal(got.faces, w.faces), n
        assert got.has_uvs == w.has_uvs and torch.equal(got.faces_uvs, w.faces_uvs), n
    away = [_cam((0.0, 0.0, -1.5), target=(0.0, 0.0, -3.0))]
    with pytest.raises(ValueError, match="shell 0"):
        cull_meshes(str(src), away, str(tmp_path / "nothing"))
