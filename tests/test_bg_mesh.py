"""The background mesh: TSDF fusion of depth maps (volsurfs_amd/bg_mesh.py, csrc/tsdf_fuse.hip).  The
restatement of the rule against the fixture recorded from the reference's own `MeshExtractor`
(tools/make_bg_mesh_golden.py), the two device entry points against the fixture, their agreement with each other, the
extraction built from its pieces, an analytic sphere end to end, the baker stage on a small Surf, and the vertex
colours of `mesh.save_ply` / `load_ply`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bg_mesh_restated as BG

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "bg_mesh.npz")
# Conditions, not measurements.  The kernel is a second, independent float32 rounding of the quantity
# whose first float32 rounding (the reference on the CPU) sits within `maxdiff` of float64: 2 x maxdiff is expected,
# 4 x leaves slack without admitting a wrong tap or weight (1e-2 and above).
BOUND_FACTOR = 4.0
MAX_FLIP_SHARE = 0.001           # of the touched points: a mask comparison may round the other way on the device


def _fixture():
    d = np.load(GOLDEN)
    return d, float(d["maxdiff"]) * BOUND_FACTOR, 5 * (2.0 / int(d["resolution"]))


def _lattice_points(n, device="cpu"):
    ax = torch.linspace(-1.0, 1.0, n, dtype=torch.float32)
    return torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).to(device)


def _restated_weights(d, points, order=None):
    t = lambda k: torch.from_numpy(d[k])
    return BG.fuse_restated(points, t("depths"), t("rgbs"), t("proj"), 5 * (2.0 / int(d["resolution"])), order=order)


def _assert_within(got, ref, weights, bound, what, touched):
    """Every value within `bound` of the reference, except at most MAX_FLIP_SHARE of the `touched` points (the number
    of points whose reference tsdf is not 1), where one sample may have entered or left the mean: |delta| <=
    2 / (w + 1) there."""
    got, ref, weights = (np.asarray(a, np.float64) for a in (got, ref, weights))
    if got.ndim == 2:
        weights = weights[:, None]
    diff = np.abs(got - ref)
    over = diff > bound
    print(f"{what}: max |got - reference| = {diff.max():.3e} (bound {bound:.3e}), {int(over.sum())} of {touched} "
          f"touched points beyond it")
    assert np.isfinite(got).all()
    assert over.sum() <= MAX_FLIP_SHARE * touched, what
    assert (diff[over] <= (2.0 / (weights + 1.0) * np.ones_like(diff))[over]).all(), what


# ---- CPU

def test_fixture_is_the_recipe():
    d, bound, trunc = _fixture()
    depths, rgbs, c2ws, ixts, query, rgb_points = BG.fixture_scene()
    for key, val in (("depths", depths), ("rgbs", rgbs), ("c2ws", c2ws), ("intrinsics", ixts)):
        assert np.array_equal(d[key], torch.stack(val).numpy()), key
    assert np.array_equal(d["rgb_points"], rgb_points.numpy())
    assert torch.equal(query, _lattice_points(int(d["query_n"])))
    assert np.array_equal(d["proj"], BG.projection_matrices(c2ws, ixts).numpy())
    assert int(d["flips"]) == 0 and 0 < float(d["maxdiff"]) < 1e-4
    assert int(d["touched"]) == int((d["tsdf"] != 1).sum()) > 5000
    for a, b in (("tsdf", "tsdf_f64"), ("tsdf_points", "tsdf_points_f64"), ("rgb", "rgb_f64")):
        assert float(np.abs(d[a].astype(np.float64) - d[b]).max()) <= float(d["maxdiff"])


def test_restatement_reproduces_the_reference_fixture_on_cpu():
    """tests/bg_mesh_restated.py on the CPU against the float32 values the reference's own closure gave: every point
    within 4 x maxdiff, no flips (measured here: equal bits)."""
    d, bound, trunc = _fixture()
    tsdf, _, w = _restated_weights(d, _lattice_points(int(d["query_n"])))
    diff = np.abs(tsdf.numpy().astype(np.float64) - d["tsdf"])
    print(f"restatement against the reference: max {diff.max():.3e}, bound {bound:.3e}")
    assert (diff <= bound).all() and int((diff > 1e-3).sum()) == 0 == int(d["flips"])
    assert int((w > 1).sum()) >= int(d["touched"])
    tsdf, rgb, _ = _restated_weights(d, torch.from_numpy(d["rgb_points"]))
    assert float(np.abs(tsdf.numpy() - d["tsdf_points"]).max()) <= bound
    assert float(np.abs(rgb.numpy() - d["rgb"]).max()) <= bound


def test_host_matrices_are_the_reference_matrices():
    from volsurfs_amd.bg_mesh import full_proj_transforms
    d, _, _ = _fixture()
    got = full_proj_transforms(list(torch.from_numpy(d["c2ws"])), list(torch.from_numpy(d["intrinsics"])))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), d["proj"])


_V = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.5, -1.5]]
_F = [[0, 1, 2], [1, 3, 2]]
# written by save_ply as it was before vertex colours existed, for the mesh above with per-corner UVs k / 16
# (binary) and without UVs (ascii)
_PLY_BINARY_UVS = bytes.fromhex(
    "706c790a666f726d61742062696e6172795f6c6974746c655f656e6469616e20312e300a636f6d6d656e7420766f6c73757266735f616d64"
    "0a656c656d656e742076657274657820340a70726f706572747920666c6f617420780a70726f706572747920666c6f617420790a70726f70"
    "6572747920666c6f6174207a0a656c656d656e74206661636520320a70726f7065727479206c69737420756368617220696e742076657274"
    "65785f696e64696365730a70726f7065727479206c69737420756368617220666c6f617420746578636f6f72640a656e645f686561646572"
    "0a0000000000000000000000000000803f0000000000000000000000000000803f000000000000803e0000003f0000c0bf03000000000100"
    "00000200000006000000000000803d0000003e0000403e0000803e0000a03e03010000000300000002000000060000c03e0000e03e000000"
    "3f0000103f0000203f0000303f")
_PLY_ASCII_PLAIN = (b"ply\nformat ascii 1.0\ncomment volsurfs_amd\nelement vertex 4\nproperty float x\nproperty float y\n"
                    b"property float z\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n"
                    b"0 0 0\n1 0 0\n0 1 0\n0.25 0.5 -1.5\n3 0 1 2\n3 1 3 2\n")


def test_save_ply_defaults_write_the_bytes_they_wrote_before(tmp_path):
    from volsurfs_amd.mesh import TensorMesh, load_ply, save_ply
    uv = torch.arange(12, dtype=torch.float32).reshape(2, 3, 2) / 16
    p = str(tmp_path / "a.ply")
    save_ply(p, TensorMesh(_V, _F, uv, device="cpu"))
    assert open(p, "rb").read() == _PLY_BINARY_UVS
    m = load_ply(p, device="cpu")
    assert isinstance(m, TensorMesh) and m.has_uvs and torch.equal(m.faces_uvs, uv)
    save_ply(p, TensorMesh(_V, _F, None, device="cpu"), binary=False)
    assert open(p, "rb").read() == _PLY_ASCII_PLAIN
    mesh, colors = load_ply(p, device="cpu", return_colors=True)
    assert colors is None and not mesh.has_uvs


@pytest.mark.parametrize("binary", [True, False])
def test_ply_vertex_colours_round_trip(tmp_path, binary):
    """uchar red / green / blue by the 8-bit rule u8 = trunc(clamp(x, 0, 1) * 255), read back as u8 / 255."""
    from volsurfs_amd.mesh import TensorMesh, load_ply, save_ply
    c = torch.tensor([[0.0, 0.5, 1.0], [1.2, -0.1, 0.999], [0.2, 0.4, 0.6], [1 / 255, 2 / 255, 254.5 / 255]])
    want = torch.tensor([[0, 127, 255], [255, 0, 254], [51, 102, 153], [1, 2, 254]], dtype=torch.float32) / 255.0
    uv = torch.arange(12, dtype=torch.float32).reshape(2, 3, 2) / 16
    for fuv in (None, uv):
        p = str(tmp_path / "c.ply")
        save_ply(p, TensorMesh(_V, _F, fuv, device="cpu"), binary=binary, vertex_colors=c)
        assert b"property uchar red\nproperty uchar green\nproperty uchar blue\n" in open(p, "rb").read()
        mesh, got = load_ply(p, device="cpu", return_colors=True)
        assert torch.equal(got, want)
        assert torch.equal(mesh.vertices, torch.tensor(_V)) and torch.equal(mesh.faces, torch.tensor(_F, dtype=torch.int32))
        assert mesh.has_uvs == (fuv is not None) and (fuv is None or torch.equal(mesh.faces_uvs, uv))
        assert torch.equal(load_ply(p, device="cpu").vertices, mesh.vertices)      # colours skipped by default
        save_ply(p, mesh, binary=binary, vertex_colors=got)                          # stored values are fixed points
        assert torch.equal(load_ply(p, device="cpu", return_colors=True)[1], want)
    with pytest.raises(ValueError):
        save_ply(str(tmp_path / "bad.ply"), TensorMesh(_V, _F, None, device="cpu"), vertex_colors=c[:3])


def test_argument_errors_are_status_codes_and_raise():
    """Checked without a GPU, through the paths that return before any launch."""
    from volsurfs_amd import _lib
    L = _lib.lib()
    null, ERR_ARG = ctypes.c_void_p(0), -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    lattice = lambda proj=p, depth=p, V=1, H=4, W=4, axis=p, n=4, trunc=0.1, out=p: \
        L.vsa_tsdf_fuse_lattice(proj, depth, V, H, W, axis, n, trunc, 0, out, null)
    assert lattice(proj=null) == ERR_ARG and lattice(depth=null) == ERR_ARG and lattice(axis=null) == ERR_ARG
    assert lattice(out=null) == ERR_ARG
    assert lattice(V=0) == ERR_ARG and lattice(n=1) == ERR_ARG and lattice(n=4097) == ERR_ARG
    assert lattice(trunc=0.0) == ERR_ARG and lattice(trunc=-1.0) == ERR_ARG and lattice(trunc=float("inf")) == ERR_ARG
    assert lattice(trunc=float("nan")) == ERR_ARG and lattice(H=0) == ERR_ARG and lattice(W=0) == ERR_ARG
    points = lambda proj=p, depth=p, rgb=null, V=1, pts=p, P=4, trunc=0.1, out=p, out_rgb=null: \
        L.vsa_tsdf_fuse_points(proj, depth, rgb, V, 4, 4, pts, P, trunc, 0, out, out_rgb, null)
    assert points(proj=null) == ERR_ARG and points(depth=null) == ERR_ARG and points(pts=null) == ERR_ARG
    assert points(out=null) == ERR_ARG and points(V=0) == ERR_ARG and points(P=-1) == ERR_ARG
    assert points(trunc=0.0) == ERR_ARG
    assert points(rgb=p) == ERR_ARG and points(out_rgb=p) == ERR_ARG                  # one without the other
    assert points(P=0, pts=null, out=null) == 0                                         # no points is fine
    assert L.vsa_tsdf_uncontract_points(null, 4, 32.0, p, null) == ERR_ARG
    assert L.vsa_tsdf_uncontract_points(p, 4, 0.0, p, null) == ERR_ARG
    assert L.vsa_tsdf_uncontract_points(null, 0, 32.0, null, null) == 0
    with pytest.raises(_lib.VolsurfsHipError):
        _lib.call("vsa_tsdf_fuse_lattice", None, None, 1, 4, 4, None, 4, 0.1, 0, None, None)


# ---- GPU

def _extractor(d, reverse=False, with_vertex_colors=False):
    from volsurfs_amd.bg_mesh import MeshExtractor
    t = lambda k: list(torch.from_numpy(d[k][::-1].copy() if reverse else d[k]))
    return MeshExtractor(t("depths"), t("rgbs"), t("c2ws"), t("intrinsics"), with_vertex_colors=with_vertex_colors)


@pytest.mark.gpu
def test_device_fusion_against_the_reference_fixture():
    """vsa_tsdf_fuse_lattice and vsa_tsdf_fuse_points against the reference's float32 tsdf and rgb.  Bound 4 x the
    fixture's maxdiff (see BOUND_FACTOR), at most 0.1 % of the touched points beyond it and those by no more than one
    sample, untouched points exactly 1."""
    d, bound, trunc = _fixture()
    ex = _extractor(d)
    n = int(d["query_n"])
    assert torch.equal(ex.full_proj_transform.cpu(), torch.from_numpy(d["proj"]))
    _, _, w = _restated_weights(d, _lattice_points(n))
    grid = ex.fuse_lattice(n, sdf_trunc=trunc)
    assert grid.shape == (n, n, n) and grid.dtype == torch.float32 and grid.is_contiguous()
    got = grid.reshape(-1).cpu().numpy()
    touched, touched_pts = int((d["tsdf"] != 1).sum()), int((d["tsdf_points"] != 1).sum())
    _assert_within(got, d["tsdf"], w, bound, "lattice tsdf", touched)
    assert (got[d["tsdf"] == 1] == 1).all()
    pts = torch.from_numpy(d["rgb_points"]).cuda()
    _, _, wp = _restated_weights(d, pts.cpu())
    tsdf, rgb = ex.fuse_points(pts, return_rgb=True, sdf_trunc=trunc)
    _assert_within(tsdf.cpu().numpy(), d["tsdf_points"], wp, bound, "points tsdf", touched_pts)
    _assert_within(rgb.cpu().numpy(), d["rgb"], wp, bound, "points rgb", touched_pts)
    assert (tsdf.cpu().numpy()[d["tsdf_points"] == 1] == 1).all()
    assert torch.equal(ex.fuse_points(pts, sdf_trunc=trunc), tsdf)                        # without the colours
    got = ex.fuse_points(_lattice_points(n, "cuda"), sdf_trunc=trunc).cpu().numpy()
    _assert_within(got, d["tsdf"], w, bound, "points tsdf on the lattice", touched)


@pytest.mark.gpu
@pytest.mark.parametrize("uncontract", [False, True])
def test_lattice_entry_equals_points_entry_bit_for_bit(uncontract):
    d, bound, trunc = _fixture()
    ex = _extractor(d)
    for n in (33, 48):                                   # 33: bricks that hang over the lattice's end
        grid = ex.fuse_lattice(n, uncontract_samples=uncontract, sdf_trunc=trunc)
        pts = _lattice_points(n, "cuda")
        flat = ex.fuse_points(pts, sdf_trunc=trunc, uncontract_samples=uncontract)
        assert torch.equal(grid.reshape(-1), flat), n
        assert torch.equal(ex.fuse_lattice(n, uncontract_samples=uncontract, sdf_trunc=trunc), grid)   # same bytes
        assert int((flat != 1).sum()) > 1000
    if uncontract:
        # outside the contraction's image the lattice keeps 1; inside, the query position is the restated inverse
        q, inside = BG.uncontract_restated(pts)
        assert bool((flat[~inside] == 1).all()) and int((~inside).sum()) > 0
        want = ex.fuse_points(q[inside].contiguous(), sdf_trunc=trunc)
        # (torch's own rounding of the position may differ in the last bit, which moves a value far less than the
        # bound unless a mask comparison flips)
        assert float(((flat[inside] - want).abs() <= bound).float().mean()) >= 1.0 - MAX_FLIP_SHARE
        assert not torch.equal(flat, ex.fuse_points(pts, sdf_trunc=trunc))


@pytest.mark.gpu
def test_view_order_is_respected():
    """The running mean is taken in the views' order: reversed views change the result within rounding only, and
    give the restated rule run in the reversed order."""
    d, bound, trunc = _fixture()
    n = int(d["query_n"])
    V = d["depths"].shape[0]
    fwd = _extractor(d).fuse_lattice(n, sdf_trunc=trunc).reshape(-1).cpu().numpy()
    rev = _extractor(d, reverse=True).fuse_lattice(n, sdf_trunc=trunc).reshape(-1).cpu().numpy()
    want, _, w = _restated_weights(d, _lattice_points(n), order=range(V - 1, -1, -1))
    touched = int((d["tsdf"] != 1).sum())
    _assert_within(rev, want.numpy(), w, bound, "reversed views against the restated rule reversed", touched)
    _assert_within(rev, fwd, w, bound, "reversed against forward", touched)
    pts = torch.from_numpy(d["rgb_points"]).cuda()
    _, rgb_want, wp = _restated_weights(d, pts.cpu(), order=range(V - 1, -1, -1))
    _, rgb = _extractor(d, reverse=True).fuse_points(pts, return_rgb=True, sdf_trunc=trunc)
    _assert_within(rgb.cpu().numpy(), rgb_want.numpy(), wp, bound, "reversed rgb",
                   int((d["tsdf_points"] != 1).sum()))


@pytest.mark.gpu
def test_extract_mesh_unbounded_is_its_pieces():
    from volsurfs_amd.bg_mesh import uncontract_points
    from volsurfs_amd.isosurface import marching_cubes
    d, _, _ = _fixture()
    ex = _extractor(d, with_vertex_colors=True)
    n = 64
    for unc in (False, True):
        mesh, colors = ex.extract_mesh_unbounded(resolution=n, uncontract_samples=unc, max_range=3.0)
        ref = marching_cubes(ex.fuse_lattice(n, uncontract_samples=unc), 0.0, [-1.0] * 3, [2.0 / (n - 1)] * 3)[0]
        assert ref.vertices.shape[0] > 500 and torch.equal(mesh.faces, ref.faces)
        q, inside = BG.uncontract_restated(ref.vertices)
        assert bool(inside.all())
        verts = uncontract_points(ref.vertices, 3.0)
        assert torch.equal(mesh.vertices, verts)
        # against torch's evaluation of the same expression: four roundings of 2^-24 each, amplified by at most
        # 1 / (2 - norm) <= 6 inside the clip box of 3 -> 1.4e-6 relative; 1e-5 asked
        assert torch.allclose(verts, q.clamp(-3.0, 3.0), rtol=1e-5, atol=1e-7)
        assert torch.equal(colors, ex.fuse_points(mesh.vertices, return_rgb=True, resolution=n)[1])
        assert bool(torch.isfinite(colors).all()) and float(colors.min()) >= 0 and float(colors.max()) <= 1
    plain = _extractor(d).extract_mesh_unbounded(resolution=n)
    assert torch.equal(plain.faces, ex.extract_mesh_unbounded(resolution=n)[0].faces)
    kept = ex.extract_mesh_unbounded(resolution=n, inv_contraction=None)[0]
    custom = ex.extract_mesh_unbounded(resolution=n, inv_contraction=lambda v: v * 100.0, max_range=32.0)[0]
    assert torch.equal(custom.vertices, (kept.vertices * 100.0).clamp(-32.0, 32.0))
    # the vertex step beyond the contraction's image: finite, on the clip box
    far = torch.tensor([[1.0, 0.0, 0.0], [-1.0, 1.0, 0.0], [0.99, 0.0, 0.0], [0.3, 0.2, 0.1]], device="cuda")
    out = uncontract_points(far, 32.0)
    assert torch.equal(out[0], torch.tensor([32.0, 0.0, 0.0], device="cuda"))
    assert torch.equal(out[1], torch.tensor([-32.0, 32.0, 0.0], device="cuda"))
    assert bool(torch.isfinite(out).all()) and torch.equal(out[3], far[3]) and 20.0 < float(out[2, 0]) <= 32.0


E2E_VIEWS, E2E_SIZE, E2E_RESOLUTION = 32, 128, 128


@pytest.mark.gpu
def test_end_to_end_on_an_analytic_sphere():
    """32 views of 128 x 128 of a sphere of radius 0.5, resolution 128: every one of 300 Fibonacci points of the true
    sphere has a mesh vertex within 1.5 voxels.  One-directional on purpose: the inward sheet that the rule leaves
    sdf_trunc behind the surface is expected.  (32 views and not 12: the initial tsdf = 1 counts as a sample, which
    moves the zero crossing inwards by sdf_trunc / n = 5 / n voxels where n views see a point; a camera sees less
    than half of the sphere, so 32 views give n of about 9 to 12.)"""
    from volsurfs_amd.bg_mesh import MeshExtractor
    depths, rgbs, c2ws, ixts = BG.e2e_scene(E2E_VIEWS, E2E_SIZE)
    ex = MeshExtractor(depths, rgbs, c2ws, ixts, with_vertex_colors=True)
    mesh, colors = ex.extract_mesh_unbounded(resolution=E2E_RESOLUTION)
    V = mesh.vertices
    assert V.shape[0] > 1000 and mesh.faces.shape[0] > 1000 and bool(torch.isfinite(V).all())
    assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < V.shape[0]
    assert colors.shape == V.shape and bool(torch.isfinite(colors).all())
    target = torch.from_numpy(BG.fibonacci_sphere(300, 0.5)).float().cuda()
    nearest = torch.cdist(target, V).min(1).values
    voxel = 2.0 / E2E_RESOLUTION
    print(f"{V.shape[0]} vertices; nearest vertex to the sphere's points: max {float(nearest.max()) / voxel:.3f} voxels")
    assert float(nearest.max()) <= 1.5 * voxel
    # the outer sheet's colours are the views' c = 0.5 + 0.5 normal, darkened to c n / (n + 1) because the initial
    # rgb = 0 counts as a sample: with n >= 4 views the mean error stays below 0.5 / 5 = 0.1, while a swapped or missing
    # channel gives 0.2 and more
    outer = (V.norm(dim=1) - 0.5).abs() < voxel
    err = (colors[outer] - (0.5 + 0.5 * torch.nn.functional.normalize(V[outer], dim=1))).abs()
    print(f"colour error on the outer sheet: mean {float(err.mean()):.3f}")
    assert int(outer.sum()) > 1000 and float(err.mean()) < 0.1


@pytest.fixture(scope="module")
def small_surf():
    """A Surf with a background model whose SDF went through 150 sphere-init iterations to radius 0.3, so that its
    rendered depth holds a surface to fuse."""
    from test_surf_method import _cameras, _gt_images, _method
    from volsurfs_amd.camera import TensorReel
    from volsurfs_amd.trainer import train
    torch.manual_seed(0)
    iters = 150
    m = _method(init_sphere_radius=0.3, hp={"lr": 3e-3, "init_phase_end_iter": iters + 1, "sdf_nr_iters_for_c2f": 0})
    assert m.models["bg"] is not None
    cams = _cameras(4)
    train(TensorReel(cams, _gt_images(cams)), m, 0, iters, nr_training_rays=512)
    m.is_training = False
    return m


@pytest.mark.gpu
def test_extract_bg_mesh_stage(small_surf, tmp_path):
    from test_surf_method import _cameras, _method
    from volsurfs_amd.bg_mesh import extract_bg_mesh
    from volsurfs_amd.mesh import load_ply
    cams = _cameras(3, H=32)
    out = str(tmp_path / "run")
    mesh, colors = extract_bg_mesh(small_surf, cams, out, resolution=48)
    files = {"depths_fg": 1, "depths_bg": 1, "fg_mask": 1, "rgbs": 3}
    for name, ch in files.items():
        with np.load(os.path.join(out, "tmp_renders", f"{name}.npz")) as data:
            assert sorted(data.keys()) == ["0", "1", "2"], name
            assert all(data[k].shape == (32, 32, ch) and data[k].dtype == np.float32 for k in data), name
    ply = os.path.join(out, "meshes", "bg.ply")
    loaded, lc = load_ply(ply, return_colors=True)
    assert mesh.faces.shape[0] > 0 and torch.equal(loaded.vertices, mesh.vertices) and torch.equal(loaded.faces, mesh.faces)
    # (the expected values on the CPU, where load_ply divides: torch's device kernels multiply by 1 / 255 instead)
    assert torch.equal(lc.cpu(), (colors.cpu().clamp(0, 1) * 255.0).to(torch.uint8).float() / 255.0)
    assert bool(torch.isfinite(mesh.vertices).all()) and float(mesh.vertices.abs().max()) <= 32.0
    first = open(ply, "rb").read()
    stamps = {n: os.path.getmtime(os.path.join(out, "tmp_renders", f"{n}.npz")) for n in files}
    small_surf.render_rays = None                          # a second call must not render
    try:
        mesh2, _ = extract_bg_mesh(small_surf, cams, out, resolution=48)
    finally:
        del small_surf.render_rays
    assert open(ply, "rb").read() == first and torch.equal(mesh2.vertices, mesh.vertices)
    assert stamps == {n: os.path.getmtime(os.path.join(out, "tmp_renders", f"{n}.npz")) for n in files}
    # the other depth choices run through the same stage
    for kw in ({"depth": "composed"}, {"depth_is_ray_length": False}):
        m3, c3 = extract_bg_mesh(small_surf, cams, None, resolution=48, **kw)
        assert bool(torch.isfinite(m3.vertices).all()) and c3.shape == m3.vertices.shape
    with pytest.raises(ValueError):
        extract_bg_mesh(small_surf, cams, out, depth="nope")
    no_bg = _method(bg_color=(0.0, 0.0, 0.0), init_sphere_radius=0.3)
    assert no_bg.models["bg"] is None
    with pytest.raises(ValueError):
        extract_bg_mesh(no_bg, cams, str(tmp_path / "none"))
    assert not os.path.exists(str(tmp_path / "none"))


@pytest.mark.gpu
def test_host_layer_raises_on_bad_arguments():
    from volsurfs_amd import _lib
    from volsurfs_amd.bg_mesh import MeshExtractor
    d, _, _ = _fixture()
    ex = _extractor(d)
    with pytest.raises(_lib.VolsurfsHipError):
        ex.fuse_lattice(1)
    with pytest.raises(_lib.VolsurfsHipError):
        ex.fuse_lattice(16, sdf_trunc=0.0)
    with pytest.raises(_lib.VolsurfsHipError):
        ex.fuse_points(torch.zeros(5, 2, device="cuda"))
    with pytest.raises(_lib.VolsurfsHipError):
        ex.fuse_points(torch.zeros(5, 3, device="cuda").double())
    assert ex.fuse_points(torch.zeros(0, 3, device="cuda")).shape == (0,)
    with pytest.raises(ValueError):
        MeshExtractor([], [], [], [])
    with pytest.raises(ValueError):
        ex.extract_mesh_unbounded(resolution=16, inv_contraction="mvdatasets")
