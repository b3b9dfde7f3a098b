"""Shell rasterization (`volsurfs_amd.rasterize`, csrc/shell_raster.hip; include/volsurfs_hip.h "Shell
rasterization"): camera hits by screen-space bins.  The acceptance is exact equality of hit_t, hit_slot and
hit_uv bits with `trace_all` on the rays of the same samples; the bin rule is checked against its numpy restatement
(tests/rasterize_restated.py) and the restatement against brute force."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import rasterize_restated as R
import shell_untangle_restated as SU
from volsurfs_amd import _lib

ERR_ARG, ERR_UNSUPPORTED = -1, -2
gpu = pytest.mark.gpu
H, W = 37, 45                      # neither a multiple of 8 nor of 64
BUILDERS = ["host", "device", "ploc"]
NAMES = ("vsa_shell_raster_workspace_bytes", "vsa_shell_raster_setup", "vsa_shell_raster_draw")


# ---------------------------------------------------------------------------------------------------------- fixtures

def _cam(eye, target=(0.0, 0.0, 0.0), focal=40.0, height=H, width=W, up=(0.0, -1.0, 0.0), device="cuda"):
    from volsurfs_amd.camera import Camera
    return Camera.look_at(eye, target, up=up, focal=focal, height=height, width=width, device=device)


def _skew_cam(device="cuda", height=H, width=W):
    """Skew and an off-centre principal point."""
    from volsurfs_amd.camera import Camera
    pose = _cam((0.7, -0.4, -0.9), device="cpu").c2w
    return Camera([[52.0, 3.5, 0.37 * width], [0.0, 47.0, 0.61 * height], [0.0, 0.0, 1.0]], pose, height, width,
                  device=device)


@functools.lru_cache(maxsize=None)
def _sphere_arrays():
    from volsurfs_amd.mesh import icosphere
    return tuple(icosphere(2, r) for r in (0.30, 0.32))


def _near_eye():
    """0.0005 in front of face 0 of the outer sphere."""
    v, f = _sphere_arrays()[1]
    a, b, c = (np.asarray(v, np.float64)[i] for i in np.asarray(f)[0])
    centre = (a + b + c) / 3.0
    return tuple(centre + 0.0005 * centre / np.linalg.norm(centre))


def _four_views(device="cuda"):
    """The three views of tests/test_visibility.py (outside, inside both shells, off axis) and one 0.0005 in front of
    the surface."""
    return (_cam((0.0, 0.0, -1.2), device=device), _cam((0.05, 0.02, 0.10), target=(1.0, 0.3, 0.2), device=device),
            _cam((0.9, 0.7, 0.5), focal=60.0, device=device), _cam(_near_eye(), device=device))


def _lobed_views(device="cuda"):
    return _cam((0.3, 0.2, -1.4), device=device), _cam((0.05, -0.08, 0.1), target=(-1.0, 0.4, 0.3), device=device)


SOUP_EYE = (0.0, 0.0, -1.2)


def _np(t):
    return t.detach().cpu().numpy()


# --------------------------------------------------------------------------------------------------------------- CPU

def test_entry_points_declared_built_and_prototyped():
    names, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in names, f"{n} is not declared in include/volsurfs_hip.h"
        assert hasattr(cdll, n), f"{n} is not in the built library"
        assert n in protos, f"{n} got no prototype"
    P, I, F, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    head = [P, LL, P, P, I, P, P, P, I, I, I, F, P, LL]
    assert protos[NAMES[0]] == (LL, [LL, I, I, I, I])
    assert protos[NAMES[1]] == (I, head + [P, P])
    assert protos[NAMES[2]] == (I, head + [LL, P, P, P, P, P, P, P])


def test_argument_errors_before_any_hip_call():
    """Every VSA_ERR_ARG case.  The "device" pointers are null or the address of a host buffer nothing reads: each call
    must return before it touches the GPU (this test runs without one)."""
    L = _lib.lib()
    buf = (ctypes.c_longlong * 16)()
    p = ctypes.addressof(buf)
    first, count = (ctypes.c_int32 * 16)(*([0] * 16)), (ctypes.c_int32 * 16)(*([4] * 16))
    stats = (ctypes.c_longlong * 4)()
    big = 1 << 40

    def setup(tris=p, nr_slots=4, first=first, count=count, nr_meshes=1, c2w=p, k=p, kinv=p, height=4, width=4,
              supersample=1, t_min=0.0, ws=p, ws_bytes=big, stats=stats):
        return L.vsa_shell_raster_setup(tris, nr_slots, first, count, nr_meshes, c2w, k, kinv, height, width,
                                        supersample, t_min, ws, ws_bytes, stats, None)

    def draw(tris=p, nr_slots=4, first=first, count=count, nr_meshes=1, c2w=p, k=p, kinv=p, height=4, width=4,
             supersample=1, t_min=0.0, ws=p, ws_bytes=big, nr_pairs=1, pairs=p, hit_t=p, hit_slot=p, hit_uv=p,
             rays_d=None):
        return L.vsa_shell_raster_draw(tris, nr_slots, first, count, nr_meshes, c2w, k, kinv, height, width,
                                       supersample, t_min, ws, ws_bytes, nr_pairs, pairs, hit_t, hit_slot, hit_uv,
                                       rays_d, None, None)

    shared = ("tris", "first", "count", "c2w", "k", "kinv", "ws")
    for name in shared + ("stats",):
        assert setup(**{name: None}) == ERR_ARG, name
    for name in shared + ("pairs", "hit_t", "hit_slot", "hit_uv"):
        assert draw(**{name: None}) == ERR_ARG, name
    null = dict(tris=None, c2w=None, k=None, kinv=None, ws=None)
    assert setup(**null) == ERR_ARG and draw(**null, pairs=None, hit_t=None, hit_slot=None, hit_uv=None) == ERR_ARG
    outside = (ctypes.c_int32 * 16)(*([2] * 16))          # slots 2 .. 5 of 4
    negative = (ctypes.c_int32 * 16)(*([-1] * 16))
    for kw in ({"nr_meshes": 0}, {"nr_meshes": 17}, {"nr_meshes": -1}, {"height": 0}, {"width": 0}, {"width": -3},
               {"supersample": 0}, {"supersample": 9}, {"t_min": -1e-6}, {"t_min": math.inf}, {"t_min": math.nan},
               {"nr_slots": 0}, {"first": outside}, {"first": negative}, {"count": negative},
               {"height": 32768, "width": 65536},                                  # exactly 2^31 samples
               {"height": 16384, "width": 32768, "supersample": 2},                # 2^29 pixels x 4
               {"height": 1 << 30, "width": 1 << 30, "supersample": 8},            # beyond 64 bits if multiplied blindly
               {"ws_bytes": 16}):
        assert setup(**kw) == ERR_ARG, kw
        assert draw(**kw) == ERR_ARG, kw
        if "first" not in kw and "count" not in kw:
            assert setup(**dict(kw, **null)) == ERR_ARG, kw
    assert draw(nr_pairs=-1) == ERR_ARG
    assert draw(nr_pairs=1 << 31) == ERR_UNSUPPORTED
    q = L.vsa_shell_raster_workspace_bytes
    for args in ((0, 1, 4, 4, 1), (4, 0, 4, 4, 1), (4, 17, 4, 4, 1), (4, 1, 0, 4, 1), (4, 1, 4, 0, 1), (4, 1, 4, 4, 0),
                 (4, 1, 4, 4, 9), (4, 1, 32768, 65536, 1)):
        assert q(*args) == ERR_ARG, args


def _assert_lists_hold_every_accepted_pair(tris, cam, s, what):
    c2w, k, kinv = _np(cam.c2w), _np(cam.intrinsics), _np(cam.intrinsics_inv)
    cls, box = R.classify(tris, c2w, k, cam.height, cam.width, s)
    x, y, X, Y = R.sample_points(cam.height, cam.width, s)
    o, d = R.pinhole_rays(c2w, kinv, x, y)
    ray, rec = R.accepted_pairs(tris, o, d)
    assert ray.size > 0 or "behind" in what, what
    assert not (cls[rec] == R.BEHIND).any(), f"{what}: a face classed behind is accepted"
    assert not (cls[rec] == R.DROPPED).any(), what
    tx, ty = X[ray] // R.TILE, Y[ray] // R.TILE
    b = box[rec]
    inside = (b[:, 0] <= tx) & (tx <= b[:, 2]) & (b[:, 1] <= ty) & (ty <= b[:, 3])
    missing = ~(inside | (cls[rec] == R.STRADDLING))
    assert not missing.any(), f"{what}: {int(missing.sum())} accepted (sample, face) pairs outside the face's tiles"
    return cls, box


@pytest.mark.parametrize("s", [1, 2, 3])
def test_restated_lists_hold_every_accepted_pair_spheres(s):
    tris = np.concatenate([R.records(v, f) for v, f in _sphere_arrays()])
    for i, cam in enumerate(_four_views("cpu")):
        cls, _ = _assert_lists_hold_every_accepted_pair(tris, cam, s, f"spheres view {i} s {s}")
        if i == 1:                                        # from inside, faces straddle and lie behind
            assert (cls == R.STRADDLING).sum() > 0 and (cls == R.BEHIND).sum() > 0


@pytest.mark.parametrize("s", [1, 2])
def test_restated_lists_hold_every_accepted_pair_lobed_stack(s):
    tris = np.concatenate([R.records(v, f) for v, f in SU.lobed_stack(**SU.STACK_B)])
    for i, cam in enumerate(_lobed_views("cpu")):
        _assert_lists_hold_every_accepted_pair(tris, cam, s, f"lobed view {i} s {s}")


@pytest.mark.parametrize("size,s", [((37, 45), 1), ((37, 45), 2), ((37, 45), 3), ((128, 128), 1)])
def test_restated_lists_hold_every_accepted_pair_soup(size, s):
    tris = R.records(*R.adversarial_soup(SOUP_EYE))
    cam = _cam(SOUP_EYE, height=size[0], width=size[1], focal=1.1 * size[1], device="cpu")
    cls, box = _assert_lists_hold_every_accepted_pair(tris, cam, s, f"soup {size} s {s}")
    assert (cls == R.STRADDLING).sum() > 20 and (cls == R.BEHIND).sum() > 0 and (cls == R.FRONT).sum() > 300


def test_restated_lists_skew_camera_and_a_shell_behind():
    tris = np.concatenate([R.records(v, f) for v, f in _sphere_arrays()])
    _assert_lists_hold_every_accepted_pair(tris, _skew_cam("cpu"), 2, "skew")
    cam = _cam((0.0, 0.0, -1.2), target=(0.0, 0.0, -3.0), device="cpu")
    cls, box = _assert_lists_hold_every_accepted_pair(tris, cam, 1, "behind")
    assert (cls == R.BEHIND).all() and R.stats(cls, box) == (tris.shape[0], 0, 0, 0)


def test_restated_hit_over_a_tile_list_is_the_hit_over_all_faces():
    """The reference hit: tri_test over the tile's list and the straddling faces gives the record of tri_test over
    every face, for samples spread over the image, from outside and from inside."""
    tris = np.concatenate([R.records(v, f) for v, f in _sphere_arrays()])
    everything = np.arange(tris.shape[0])
    for cam in _four_views("cpu")[:2]:
        c2w, k, kinv = _np(cam.c2w), _np(cam.intrinsics), _np(cam.intrinsics_inv)
        cls, box = R.classify(tris, c2w, k, H, W, 2)
        lists, straddling = R.tile_lists(cls, box, H, W, 2)
        x, y, X, Y = R.sample_points(H, W, 2)
        o, d = R.pinhole_rays(c2w, kinv, x, y)
        hits = 0
        for n in range(0, x.shape[0], 97):
            mine = lists.get((int(X[n]) // R.TILE, int(Y[n]) // R.TILE), []) + straddling
            got, want = R.closest_hit(tris, mine[::-1], o[n], d[n]), R.closest_hit(tris, everything, o[n], d[n])
            assert got[1] == want[1] and np.array_equal(np.array(got, np.float32).view(np.int32),
                                                        np.array(want, np.float32).view(np.int32)), n
            hits += want[1] >= 0
        assert hits > 10


def test_python_argument_errors_before_any_hip_call():
    from volsurfs_amd.rasterize import check_hits_mode, grid_side, tracer_rasterize

    class Tracer:
        device, nr_meshes = torch.device("cpu"), 1
    cam = _cam((0.0, 0.0, -1.2), device="cpu")
    for kw in ({"supersample": 0}, {"supersample": 9}, {"t_min": -0.5}, {"t_min": math.nan}):
        with pytest.raises(ValueError):
            tracer_rasterize(Tracer(), cam, **kw)
    with pytest.raises(_lib.VolsurfsHipError, match="on the GPU"):
        tracer_rasterize(Tracer(), cam)
    for bad in (2, 3, 5, 8, 0, 81):
        with pytest.raises(ValueError, match="square"):
            grid_side(bad)
    assert [grid_side(r) for r in (1, 4, 9, 64)] == [1, 2, 3, 8]
    with pytest.raises(ValueError):
        check_hits_mode("rays")


# --------------------------------------------------------------------------------------------------------------- GPU

def _mesh(v, f):
    from volsurfs_amd.mesh import TensorMesh
    return TensorMesh(np.asarray(v, np.float32), np.asarray(f), device="cuda")


@functools.lru_cache(maxsize=None)
def _tracer(name, builder="device"):
    from volsurfs_amd.raytrace import RayTracer
    if name == "spheres":
        meshes = [_mesh(v, f) for v, f in _sphere_arrays()]
    elif name == "lobed":
        meshes = [_mesh(v, f) for v, f in SU.lobed_stack(**SU.STACK_B)]
    elif name == "soup":
        meshes = [_mesh(*R.adversarial_soup(SOUP_EYE))]
    elif name == "sixteen":
        from volsurfs_amd.mesh import icosphere
        meshes = [_mesh(*icosphere(1, 0.20 + 0.01 * k)) for k in range(16)]
    elif name == "wall":                       # one face far larger than the view, and a small one in a corner
        v = np.array([[-50, -50, 1], [50, -50, 1], [0, 80, 1], [0.30, 0.30, 0.5], [0.34, 0.30, 0.5], [0.30, 0.34, 0.5]])
        meshes = [_mesh(v, np.array([[0, 1, 2], [3, 4, 5]], np.int32))]
    return RayTracer(meshes, builder=builder)


def _sample_rays(cam, s):
    """The rays of the sample grid, in output order: `get_camera_rays` at s = 1, the restated pinhole ray uploaded."""
    if s == 1:
        from volsurfs_amd.camera import get_camera_rays
        o, d, _ = get_camera_rays(cam)
        return o, d
    x, y, _, _ = R.sample_points(cam.height, cam.width, s)
    o, d = R.pinhole_rays(_np(cam.c2w), _np(cam.intrinsics_inv), x, y)
    return torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_equals_the_trace(tracer, cam, s, what, t_min=0.0):
    got = tracer.rasterize(cam, supersample=s, t_min=t_min)
    stats = tracer.raster_stats
    o, d = _sample_rays(cam, s)
    want = tracer.trace_all(o, d, t_min=t_min)
    for name, g, w in zip(("hit_t", "hit_slot", "hit_uv"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        diff = int((_bits(g) != _bits(w)).sum())
        print(f"{what}: {name} differs in {diff} of {g.numel()}; hits {int((want[1] >= 0).sum())}; {stats}")
        assert diff == 0, f"{what}: {name} differs from trace_all in {diff} of {g.numel()} words"
    cls, box = R.classify(_np(tracer.tris), _np(cam.c2w), _np(cam.intrinsics), cam.height, cam.width, s)
    assert tuple(stats) == R.stats(cls, box), f"{what}: RasterStats {tuple(stats)} != restated {R.stats(cls, box)}"
    return want, stats


@gpu
@pytest.mark.parametrize("builder", BUILDERS)
def test_spheres_equal_the_trace(builder):
    tracer = _tracer("spheres", builder)
    for i, cam in enumerate(_four_views()):
        for s in (1, 2, 3):
            want, stats = _assert_equals_the_trace(tracer, cam, s, f"{builder} view {i} s {s}")
            assert int((want[1] >= 0).sum()) > 0
            if i == 1:
                assert stats.straddling > 0 and stats.behind > 0


@gpu
def test_f32_nodes_give_the_same_records():
    from volsurfs_amd.raytrace import RayTracer
    tracer = RayTracer([_mesh(v, f) for v, f in _sphere_arrays()], node_format="f32")
    _assert_equals_the_trace(tracer, _four_views()[2], 2, "f32 nodes")


@gpu
@pytest.mark.parametrize("s", [1, 2])
def test_lobed_stack_equals_the_trace(s):
    tracer = _tracer("lobed")
    assert tracer.nr_meshes == 5
    for i, cam in enumerate(_lobed_views()):
        want, _ = _assert_equals_the_trace(tracer, cam, s, f"lobed view {i} s {s}")
        assert int((want[1] >= 0).sum()) > 1000


@gpu
@pytest.mark.parametrize("size,s", [((37, 45), 1), ((37, 45), 2), ((37, 45), 3), ((128, 128), 1)])
def test_adversarial_soup_equals_the_trace(size, s):
    cam = _cam(SOUP_EYE, height=size[0], width=size[1], focal=1.1 * size[1])
    _, stats = _assert_equals_the_trace(_tracer("soup"), cam, s, f"soup {size} s {s}")
    assert stats.straddling > 20 and stats.behind > 0 and stats.binned > 300


@gpu
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 7), (64, 1), (1, 65)])
def test_image_shapes_at_the_tile_and_wave_edges(size):
    for s in (1, 3):
        cam = _cam((0.0, 0.0, -1.2), height=size[0], width=size[1], focal=30.0)
        _assert_equals_the_trace(_tracer("spheres"), cam, s, f"image {size} s {s}")


@gpu
def test_a_shell_wholly_behind_the_camera_is_all_misses():
    tracer = _tracer("spheres")
    cam = _cam((0.0, 0.0, -1.2), target=(0.0, 0.0, -3.0))
    want, stats = _assert_equals_the_trace(tracer, cam, 2, "behind")
    assert int((want[1] >= 0).sum()) == 0 and tuple(stats) == (640, 0, 0, 0)
    hit_t, hit_slot, hit_uv = tracer.rasterize(cam)
    assert (hit_slot == -1).all() and (hit_t == 0).all() and (hit_uv == 0).all()


@gpu
def test_one_face_covers_every_tile_and_a_tile_list_is_empty():
    tracer = _tracer("wall")
    cam = _cam((0.0, 0.0, -1.2))
    want, stats = _assert_equals_the_trace(tracer, cam, 1, "wall")
    tiles = ((H + 7) // 8) * ((W + 7) // 8)
    assert stats.binned == 2 and tiles < stats.pairs < 2 * tiles and bool((want[1] >= 0).all())
    # the same view without the wall: most tiles have an empty list and no straddler
    from volsurfs_amd.raytrace import RayTracer
    v = np.array([[0.30, 0.30, 0.5], [0.34, 0.30, 0.5], [0.30, 0.34, 0.5]])
    small = RayTracer([_mesh(v, np.array([[0, 1, 2]], np.int32))], builder="device")
    want, stats = _assert_equals_the_trace(small, cam, 2, "one small face")
    assert stats.straddling == 0 and 0 < stats.pairs < tiles and int((want[1] >= 0).sum()) > 0


@gpu
def test_one_shell_and_sixteen():
    cam = _cam((0.4, 0.1, -0.9))
    tracer = _tracer("sixteen")
    assert tracer.nr_meshes == 16
    want, _ = _assert_equals_the_trace(tracer, cam, 2, "K = 16")
    assert all(int((want[1][k] >= 0).sum()) > 0 for k in range(16))
    _assert_equals_the_trace(_tracer("soup"), cam, 1, "K = 1")


@gpu
def test_skew_and_off_centre_principal_point():
    want, _ = _assert_equals_the_trace(_tracer("spheres"), _skew_cam(), 2, "skew")
    assert int((want[1] >= 0).sum()) > 100
    _assert_equals_the_trace(_tracer("lobed"), _skew_cam(), 1, "skew lobed")


@gpu
def test_t_min_is_the_trace_s():
    _assert_equals_the_trace(_tracer("spheres"), _four_views()[1], 1, "t_min", t_min=0.25)


@gpu
def test_want_dirs_out_and_rasterize_shells():
    from volsurfs_amd.camera import get_camera_rays
    from volsurfs_amd.rasterize import RasterStats, rasterize_shells
    tracer = _tracer("spheres")
    cam = _four_views()[2]
    assert _lib.workspace_bytes("vsa_shell_raster_workspace_bytes", 640, 2, H, W, 3) > 20 * 640
    hit_t, hit_slot, hit_uv, dirs = tracer.rasterize(cam, want_dirs=True)
    _, d, _ = get_camera_rays(cam)
    assert torch.equal(_bits(dirs), _bits(d))
    assert isinstance(tracer.raster_stats, RasterStats)
    x, y, _, _ = R.sample_points(H, W, 3)
    _, d3 = R.pinhole_rays(_np(cam.c2w), _np(cam.intrinsics_inv), x, y)
    assert torch.equal(_bits(tracer.rasterize(cam, 3, want_dirs=True)[3]), _bits(torch.from_numpy(d3).cuda()))
    K, N = 2, H * W
    out = (torch.full((K, N), 7.0, device="cuda"), torch.full((K, N), 7, dtype=torch.int32, device="cuda"),
           torch.full((K, N, 2), 7.0, device="cuda"))
    back = tracer.rasterize(cam, out=out)
    assert all(b is o for b, o in zip(back, out)) and torch.equal(out[1], hit_slot) and torch.equal(out[0], hit_t)
    with pytest.raises(_lib.VolsurfsHipError):
        tracer.rasterize(cam, out=(out[0], out[1].long(), out[2]))
    meshes = [_mesh(v, f) for v, f in _sphere_arrays()]
    again = rasterize_shells(meshes, cam, tracer=tracer)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, (hit_t, hit_slot, hit_uv)))
    fresh = rasterize_shells(meshes, cam)                 # (its own device-built tracer: other slots, the same faces)
    assert torch.equal(fresh[0], hit_t)
    with pytest.raises(ValueError):
        rasterize_shells(meshes[:1], cam, tracer=tracer)


@gpu
def test_python_argument_errors_on_the_device():
    from volsurfs_amd.mesh import TensorMesh, nested_shells
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.rasterize import rasterize_shells
    from volsurfs_amd.raytrace import RayTracer
    cam = _cam((0.0, 0.0, -1.5))
    m = VolSurfs(nested_shells(K=2, subdiv=2), max_rays=4 * H * W, textures_res=(64, 32, 16, 8), bg_color=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="jitter"):
        m.render_camera(cam, jitter_pixels=True, hits="raster")
    with pytest.raises(ValueError, match="square"):
        m.render_camera(cam, nr_rays_per_pixel=2, hits="raster")
    with pytest.raises(ValueError):
        m.render_camera(cam, hits="bins")
    with pytest.raises(ValueError):
        m.raytracer.rasterize(cam, t_min=-1.0)
    v, f = _sphere_arrays()[0]
    cpu_mesh = TensorMesh(np.asarray(v, np.float32), np.asarray(f), device="cpu")
    with pytest.raises(_lib.VolsurfsHipError, match="on the GPU"):
        rasterize_shells([cpu_mesh], cam)
    with pytest.raises(_lib.VolsurfsHipError, match="on the GPU"):
        RayTracer([cpu_mesh], builder="host").rasterize(cam)


def _baked_method(K=2):
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.methods import VolSurfs
    m = VolSurfs(nested_shells(K=K, subdiv=3), max_rays=4096, textures_res=(64, 32, 16, 8))
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        m.bank.tables.copy_((torch.rand(m.bank.tables.shape, generator=g) * 2 - 1).cuda())
    m.bank.refresh_half_params()
    m.bake()
    return m


def _assert_same_dict(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if a[k] is None:
            assert b[k] is None, (what, k)
            continue
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), (what, k)


@gpu
def test_render_baked_camera_equals_render_baked(tmp_path):
    from volsurfs_amd.camera import get_camera_rays
    from volsurfs_amd.renderers import VolsurfsRenderer
    from volsurfs_amd.texture_export import extract_textures
    m = _baked_method()
    cam = _cam((0.5, 0.2, -1.4), focal=60.0, height=48, width=56)
    o, d, _ = get_camera_rays(cam)
    want = m.render_baked(o, d)
    assert int((want["surfs_alpha"].sum((1, 2)) > 0).sum()) > 200
    _assert_same_dict(m.render_baked_camera(cam, hits="raster"), want, "raster")
    _assert_same_dict(m.render_baked_camera(cam), want, "trace")
    _assert_same_dict(VolsurfsRenderer(m).render_baked_camera(cam, hits="raster"), want, "renderer")
    ss = m.render_baked_camera(cam, supersample=2, hits="raster")
    assert ss["rgb"].shape == want["rgb"].shape and bool(torch.isfinite(ss["rgb"]).all())
    assert m.render_baked_camera(cam, supersample=2)["rgb"].shape == want["rgb"].shape
    out = str(tmp_path / "scene")
    extract_textures(m, out, compress_level=1)
    r = VolsurfsRenderer.from_scene(out)
    _assert_same_dict(r.render_baked_camera(cam, hits="raster"), r.method.render_baked(o, d), "from_scene")
    _assert_same_dict(r.render_baked_camera(cam, hits="raster"), r.render_baked_camera(cam), "from_scene trace")


@gpu
def test_render_camera_raster_equals_trace_at_one_ray_per_pixel():
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.methods import VolSurfs
    torch.manual_seed(0)
    cam = _cam((0.4, 0.3, -1.5), focal=60.0, height=40, width=52)
    m = VolSurfs(nested_shells(K=3, subdiv=3), max_rays=4096, textures_res=(64, 32, 16, 8), bg_color=(1.0, 1.0, 1.0))
    want = m.render_camera(cam)
    assert not torch.allclose(want["rgb"][20, 26].float(), torch.ones(3, device="cuda"))
    _assert_same_dict(m.render_camera(cam, hits="raster"), want, "one chunk")
    _assert_same_dict(m.render_camera(cam, hits="raster", chunk=700), want, "chunks")
    ss = m.render_camera(cam, nr_rays_per_pixel=4, hits="raster", chunk=4096)
    assert ss["rgb"].shape == (40, 52, 3) and bool(torch.isfinite(ss["rgb"].float()).all())
