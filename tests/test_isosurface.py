"""Marching cubes on the GPU (csrc/isosurface.hip, volsurfs_amd/isosurface.py).

`restate` below is the numpy restatement of the rules in include/volsurfs_hip.h: the same table (read from
volsurfs_amd.isosurface), the same fp32 operations in the same order and the same output order, so the kernel is held
to it bit for bit.  Topology, geometry, determinism, the reference's sampling / filtering / level rules, the files and
the path into RayTracer and VolSurfs are checked on top."""
import os
import zlib

import numpy as np
import pytest
import torch

from volsurfs_amd import isosurface as iso


# ------------------------------------------------------------------------------------------------- restatement

def restate(f, levels, origin, spacing, inside_above=False):
    """[(V [V,3] f32, F [F,3] i32)] per level, in the kernel's order."""
    f = np.ascontiguousarray(f, np.float32)
    nx, ny, nz = f.shape
    origin, spacing = np.asarray(origin, np.float32), np.asarray(spacing, np.float32)
    tab = iso.MC_TABLE
    out = []
    for lev in levels:
        lev = np.float32(lev)
        ins = (f > lev) if inside_above else (f < lev)
        cross = np.zeros((nx, ny, nz, 3), bool)
        cross[:-1, :, :, 0] = ins[:-1] != ins[1:]
        cross[:, :-1, :, 1] = ins[:, :-1] != ins[:, 1:]
        cross[:, :, :-1, 2] = ins[:, :, :-1] != ins[:, :, 1:]
        flat = cross.reshape(-1)
        ids = (np.cumsum(flat) - flat).reshape(nx, ny, nz, 3)      # by owning point in C order, then axis
        pi, pj, pk, pa = np.nonzero(cross)
        idx = np.stack([pi, pj, pk], 1)
        bidx = idx.copy()
        bidx[np.arange(len(pa)), pa] += 1
        fa = f[pi, pj, pk]
        fb = f[bidx[:, 0], bidx[:, 1], bidx[:, 2]]
        t = (lev - fa) / (fb - fa)
        V = np.empty((len(pa), 3), np.float32)
        for a in range(3):
            fi = idx[:, a].astype(np.float32)
            V[:, a] = np.where(pa == a, origin[a] + (fi + t) * spacing[a], origin[a] + fi * spacing[a])
        cells = (nx - 1) * (ny - 1) * (nz - 1)
        case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
        for c, o in enumerate(iso.CORNER_OFFSETS):
            case |= ins[o[0]:nx - 1 + o[0], o[1]:ny - 1 + o[1], o[2]:nz - 1 + o[2]].astype(np.int64) << c
        E = np.empty((12, cells), np.int64)
        for e, (o, a) in enumerate(zip(iso.EDGE_OWNERS, iso.EDGE_AXES)):
            E[e] = ids[o[0]:nx - 1 + o[0], o[1]:ny - 1 + o[1], o[2]:nz - 1 + o[2], a].reshape(-1)
        tri = tab[case.reshape(-1)][:, :15].astype(np.int64).reshape(cells, 5, 3)
        valid = tri[:, :, 0] >= 0
        F = E[np.maximum(tri, 0), np.arange(cells)[:, None, None]][valid]      # by cell, then table order
        out.append((V, F.astype(np.int32)))
    return out


def _topology(V, F):
    """Asserts every undirected edge lies in exactly two faces, in opposite directions; returns V - E + F."""
    F = np.asarray(F, np.int64)
    n = max(len(V), 1)
    d = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], 0)
    fwd, rev = d[:, 0] * n + d[:, 1], d[:, 1] * n + d[:, 0]
    assert len(np.unique(fwd)) == len(fwd), "a directed edge is used twice"
    assert np.isin(rev, fwd).all(), "an edge has no opposite twin: not watertight"
    return len(V) - len(fwd) // 2 + len(F)


def _signed_volume(V, F):
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64)
    return np.einsum("ij,ij->i", V[F[:, 0]], np.cross(V[F[:, 1]], V[F[:, 2]])).sum() / 6.0


def _lattice(shape, lo=-1.0, hi=1.0):
    axes = [np.linspace(lo, hi, n, dtype=np.float32) for n in shape]
    return np.meshgrid(*axes, indexing="ij")


def _sphere(shape, r, c=(0.0, 0.0, 0.0)):
    X, Y, Z = _lattice(shape)
    return (np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r).astype(np.float32)


def _torus(shape, R=0.5, r=0.2):
    X, Y, Z = _lattice(shape)
    return (np.sqrt((np.sqrt(X ** 2 + Y ** 2) - R) ** 2 + Z ** 2) - r).astype(np.float32)


def _lobed(shape, seed=0, noise=0.0):
    X, Y, Z = _lattice(shape)
    rad = np.sqrt(X ** 2 + Y ** 2 + Z ** 2)
    phi = np.arctan2(Y, X)
    f = rad - 0.45 * (1.0 + 0.25 * np.sin(4.0 * phi) * np.cos(3.0 * Z))
    if noise:
        f = f + noise * np.random.default_rng(seed).standard_normal(f.shape)
    return f.astype(np.float32)


def _noisy_closed(n, seed):
    """White noise inside, a ramp to well above every level near the boundary: closed surfaces, many ambiguous
    faces and cells."""
    X, Y, Z = _lattice((n, n, n))
    box = np.maximum(np.abs(X), np.maximum(np.abs(Y), np.abs(Z)))
    noise = np.random.default_rng(seed).standard_normal((n, n, n)).astype(np.float32)
    return np.where(box > 0.85, np.float32(10.0), noise).astype(np.float32)


def _h(n):
    return 2.0 / (n - 1)


# ------------------------------------------------------------------------------------------------ no GPU needed

def test_table_header_matches_the_python_table():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_mc_table.py")
    spec = importlib.util.spec_from_file_location("gen_mc_table", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.OUT) as f:
        assert f.read() == gen.render(iso.MC_TABLE)


def test_compiled_table_equals_the_python_table():
    tab = iso.MC_TABLE
    assert tab.shape == (256, 16) and tab.dtype == np.int8
    assert np.array_equal(iso.device_mc_table(), tab)
    # complementary cases cross the same edges
    for c in range(256):
        e = set(tab[c][tab[c] >= 0].tolist())
        assert e == set(tab[255 - c][tab[255 - c] >= 0].tolist())


@pytest.mark.parametrize("inside_above", [False, True])
def test_restatement_is_watertight_on_noise(inside_above):
    """The table's ambiguity rule on a field where a large share of the faces is ambiguous."""
    f = _noisy_closed(40, seed=5)
    if inside_above:
        f = -f
    V, F = restate(f, [0.0], [-1.0] * 3, [_h(40)] * 3, inside_above)[0]
    assert len(F) > 20000
    _topology(V, F)
    assert _signed_volume(V, F) > 0


def test_baker_level_rule():
    import torch as T
    for K in (3, 5):
        off = 0.0025 * (K // 2)
        ref = [round(x.item(), 4) for x in T.linspace(-off, off, K)]
        assert iso.level_set_values(K, 0.0025) == ref
    assert iso.level_set_values(5, 0.0025) == [-0.005, -0.0025, 0.0, 0.0025, 0.005]
    assert iso.level_set_values(1, 0.0025, extract_level_set=0.012345) == [0.0123]


def test_bounding_primitive_point_tests():
    from volsurfs_amd.background import BoundingBox, BoundingSphere
    p = torch.tensor([[0.5, 0.0, 0.0], [0.5001, 0.0, 0.0], [0.3, 0.3, 0.3], [0.0, -0.49, 0.49]])
    assert BoundingBox(1.0).check_points_inside(p).tolist() == [True, False, True, True]
    assert BoundingSphere(0.5).check_points_inside(p).tolist() == [True, False, False, False]


# ------------------------------------------------------------------------------------------------------- GPU

def _mc(f, levels, origin, spacing, inside="below"):
    return iso.marching_cubes(torch.from_numpy(np.ascontiguousarray(f)).cuda(), levels, origin, spacing, inside)


def _np(m):
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy()


def _assert_exact(meshes, ref):
    assert len(meshes) == len(ref)
    for m, (V, F) in zip(meshes, ref):
        v, f = _np(m)
        assert f.shape == F.shape and np.array_equal(f, F)
        assert v.shape == V.shape and np.array_equal(v.view(np.int32), V.view(np.int32))
        assert m.faces.dtype == torch.int32 and m.faces_uvs.shape == (F.shape[0], 3, 2)
        assert not m.has_uvs and not m.faces_uvs.any()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 2, 2), (17, 23, 31), (40, 40, 40), (33, 5, 300)])
@pytest.mark.parametrize("field", ["random", "smooth_noise", "sdf"])
@pytest.mark.parametrize("inside", ["below", "above"])
def test_exact_vs_restatement(shape, field, inside):
    rng = np.random.default_rng(zlib.crc32(repr((shape, field)).encode()))
    if field == "random":
        f = rng.standard_normal(shape).astype(np.float32)
    elif field == "smooth_noise":
        X, Y, Z = _lattice(shape)
        f = (np.sin(3 * X) * np.cos(2 * Y) + 0.5 * Z + 0.05 * rng.standard_normal(shape)).astype(np.float32)
    else:
        f = _sphere(shape, 0.6, c=(0.1, -0.05, 0.02))
    origin, spacing = [-0.3, 0.2, -1.0], [0.05, 0.031, 0.0123]
    for levels in ([0.1], [0.3, -0.2, 0.0, 0.25, -0.4]):
        got = _mc(f, levels, origin, spacing, inside)
        _assert_exact(got, restate(f, levels, origin, spacing, inside == "above"))


@pytest.mark.gpu
def test_exact_with_grid_values_at_the_level():
    """Corners exactly at the level are outside (strict test) and zero-area faces are kept."""
    f = np.round(np.random.default_rng(3).standard_normal((21, 19, 26)) * 2).astype(np.float32) / 2
    levels = [0.0, 0.5, -1.0]
    got = _mc(f, levels, [0.0] * 3, [1.0] * 3)
    ref = restate(f, levels, [0.0] * 3, [1.0] * 3)
    _assert_exact(got, ref)
    V, F = ref[0]
    area = np.linalg.norm(np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]), axis=1)
    assert (area == 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name,field,euler", [
    ("sphere", lambda n: _sphere((n, n, n), 0.5), 2),
    ("torus", lambda n: _torus((n, n, n)), 0),
    ("two_spheres", lambda n: np.minimum(_sphere((n, n, n), 0.3, (0.45, 0, 0)), _sphere((n, n, n), 0.3, (-0.45, 0, 0))), 4),
])
def test_topology(name, field, euler):
    n = 64
    for inside in ("below", "above"):
        f = field(n) if inside == "below" else -field(n)
        V, F = _np(_mc(f, [0.0], [-1.0] * 3, [_h(n)] * 3, inside)[0])
        assert _topology(V, F) == euler, name
        assert _signed_volume(V, F) > 0


@pytest.mark.gpu
def test_topology_noisy_closed_field():
    n = 112
    f = _noisy_closed(n, seed=11)
    meshes = _mc(f, [0.0, 0.7, -0.9], [-1.0] * 3, [_h(n)] * 3)
    for m in meshes:
        V, F = _np(m)
        assert len(F) > 100000
        _topology(V, F)


@pytest.mark.gpu
def test_geometry_sphere():
    n, r = 128, 0.3
    h = _h(n)
    V, F = _np(_mc(_sphere((n, n, n), r), [0.0], [-1.0] * 3, [h] * 3)[0])
    assert np.abs(np.linalg.norm(V.astype(np.float64), axis=1) - r).max() <= 0.5 * h
    vol = _signed_volume(V, F)
    assert vol > 0 and abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1.0) < 0.01


@pytest.mark.gpu
def test_determinism_and_level_split():
    f = _lobed((48, 52, 44), noise=0.02)
    levels = [0.02, -0.03, 0.0, 0.05, -0.01]
    a = _mc(f, levels, [-1.0] * 3, [0.04] * 3)
    b = _mc(f, levels, [-1.0] * 3, [0.04] * 3)
    singles = [_mc(f, [lv], [-1.0] * 3, [0.04] * 3)[0] for lv in levels]
    for x, y, z in zip(a, b, singles):
        for other in (y, z):
            assert torch.equal(x.faces, other.faces)
            assert torch.equal(x.vertices.view(torch.int32), other.vertices.view(torch.int32))


def _lobed_fn(pts):
    rad = torch.linalg.vector_norm(pts, dim=-1)
    phi = torch.atan2(pts[:, 1], pts[:, 0])
    return (rad - 0.45 * (1.0 + 0.25 * torch.sin(4.0 * phi) * torch.cos(3.0 * pts[:, 2])))[:, None]


@pytest.mark.gpu
def test_extract_level_sets_equals_one_extraction_per_level():
    n = 56
    meshes, levels = iso.extract_level_sets(_lobed_fn, n, 5, delta_surfs=0.01)
    assert levels == sorted(levels) and len(meshes) == 5
    for m, lv in zip(meshes, levels):
        one = iso.extract_mesh_from_fn(_lobed_fn, n, level_set=lv, threshold=0.0)
        assert torch.equal(m.faces, one.faces)
        # the crossing is interpolated on f at `lv` instead of on f - lv at 0: only that rounding differs
        assert torch.allclose(m.vertices, one.vertices, rtol=0, atol=1e-5)
    # the same grid through the kernel directly: bit-identical
    grid = iso.sample_grid(_lobed_fn, n)
    direct = iso.marching_cubes(grid, levels, [-1.0] * 3, [2.0 / (n - 1)] * 3)
    for m, d in zip(meshes, direct):
        assert torch.equal(m.faces, d.faces) and torch.equal(m.vertices, d.vertices)


@pytest.mark.gpu
def test_sample_grid_order_and_tuple_outputs():
    n, r = 37, 0.8
    fn = lambda p: (torch.stack([p[:, 0] + 10 * p[:, 1] + 100 * p[:, 2] ** 3, -p[:, 0]], -1), None)
    g = iso.sample_grid(fn, n, scene_radius=r, out_idx=0, chunk=16)
    ax = torch.linspace(-r, r, n, dtype=torch.float32)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    want = X + 10 * Y + 100 * Z ** 3
    assert torch.equal(g.cpu(), want)
    seen = []
    g2 = iso.sample_grid(lambda p, iter_nr: (seen.append(iter_nr), p[:, :1])[1], 9, iter_nr=7)
    assert set(seen) == {7} and torch.equal(g2.cpu(), torch.meshgrid(*[torch.linspace(-1, 1, 9)] * 3, indexing="ij")[0])


@pytest.mark.gpu
@pytest.mark.parametrize("prim", ["box", "sphere"])
def test_bounding_primitive_filter(prim):
    from volsurfs_amd.background import BoundingBox, BoundingSphere
    bp = BoundingBox(1.4) if prim == "box" else BoundingSphere(0.7)
    n, r = 48, bp.get_radius()
    fn = lambda p: (torch.linalg.vector_norm(p - torch.tensor([0.3, 0.0, 0.0], device=p.device), dim=-1) - 0.5)[:, None]
    got = iso.extract_mesh_from_fn(fn, n, bounding_primitive=bp)
    full = iso.marching_cubes(iso.sample_grid(fn, n, scene_radius=r), [0.0], [-r] * 3, [2 * r / (n - 1)] * 3)[0]
    V, F = _np(full)
    inside = (np.abs(V).max(1) <= np.float32(0.7)) if prim == "box" else \
        (np.linalg.norm(V, axis=1) <= np.float32(0.7))
    keep = inside[F].all(1)
    used = np.zeros(len(V), bool)
    used[F[keep].reshape(-1)] = True
    remap = np.cumsum(used) - 1
    v, f = _np(got)
    assert 0 < keep.sum() < len(F)
    assert np.array_equal(f, remap[F[keep]]) and np.array_equal(v, V[used])


@pytest.mark.gpu
def test_empty_and_invalid_inputs():
    from volsurfs_amd._lib import VolsurfsHipError
    m = iso.extract_mesh_from_fn(lambda p: torch.linalg.vector_norm(p, dim=-1)[:, None] + 5.0, 16)
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.faces_uvs.shape == (0, 3, 2)
    empty = iso.marching_cubes(torch.ones(8, 8, 8, device="cuda"), [0.0, 1.0, 2.0], [0.0] * 3, [1.0] * 3)
    assert [tuple(x.faces.shape) for x in empty] == [(0, 3)] * 3 and empty[0].vertices.shape == (0, 3)
    bad = torch.zeros(8, 8, 8, device="cuda")
    bad[3, 4, 5] = float("nan")
    with pytest.raises(VolsurfsHipError):
        iso.marching_cubes(bad, [0.0], [0.0] * 3, [1.0] * 3)
    bad[3, 4, 5] = float("inf")
    with pytest.raises(VolsurfsHipError):
        iso.marching_cubes(bad, [0.0], [0.0] * 3, [1.0] * 3)
    with pytest.raises(VolsurfsHipError):
        iso.marching_cubes(torch.zeros(8, 8, 8, device="cuda"), [0.0] * 17, [0.0] * 3, [1.0] * 3)
    with pytest.raises(VolsurfsHipError):
        iso.marching_cubes(torch.zeros(8, 1, 8, device="cuda"), [0.0], [0.0] * 3, [1.0] * 3)
    with pytest.raises(VolsurfsHipError):
        iso.marching_cubes(torch.zeros(8, 8, 8, device="cuda"), [0.0], [0.0] * 3, [0.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        iso.save_level_sets([empty[0]], [0.0], "/nonexistent")
    with pytest.raises(VolsurfsHipError):
        iso.workspace_bytes((8, 1, 8), 1)


@pytest.mark.gpu
def test_end_to_end_files_raytracer_and_volsurfs(tmp_path):
    from tests.bvh_builder_cases import assert_same_hits as _assert_same_hits
    from volsurfs_amd.camera import pinhole_rays
    from volsurfs_amd.mesh import load_meshes_indexed_from_path
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.raytrace import RayTracer
    meshes, levels = iso.extract_level_sets(_lobed_fn, 72, 5, delta_surfs=0.01)
    out = str(tmp_path / "meshes")
    paths = iso.save_level_sets(meshes, levels, out)
    assert sorted(os.listdir(out)) == sorted(f"{round(lv, 4)}.ply" for lv in levels) and len(paths) == 5
    with open(paths[0], "rb") as fh:
        assert b"texcoord" not in fh.read(400)
    loaded = load_meshes_indexed_from_path(None, out)
    for m, l in zip(meshes, loaded):                        # inner -> outer
        assert not l.has_uvs
        assert torch.equal(m.faces, l.faces) and torch.equal(m.vertices, l.vertices)
    o, d = pinhole_rays(96, 96, focal=120.0, cam_pos=(0.0, 0.0, -1.6))
    host, ploc = RayTracer(loaded), RayTracer(loaded, builder="ploc")
    ref = [x.clone() for x in host.trace_all(o, d)]
    assert (ref[1] >= 0).sum().item() > 1000
    _assert_same_hits(ploc.trace_all(o, d), ref, ploc, host)
    # sphere shells: hit t within h of the analytic ray-sphere t
    n, radii = 96, [0.3, 0.35, 0.4]
    sph = iso.marching_cubes(iso.sample_grid(lambda p: torch.linalg.vector_norm(p, dim=-1)[:, None], n), radii,
                             [-1.0] * 3, [_h(n)] * 3)
    t, slot, _ = RayTracer(sph, builder="ploc").trace_all(o, d)
    oo, dd = o.double(), torch.nn.functional.normalize(d.double(), dim=-1)
    scale = torch.linalg.vector_norm(d.double(), dim=-1)
    for k, r in enumerate(radii):
        b = (oo * dd).sum(-1)
        disc = b * b - ((oo * oo).sum(-1) - r * r)
        hit = (slot[k] >= 0) & (disc > (4 * _h(n)) ** 2)
        t_ref = (-b - disc.clamp(min=0).sqrt()) / scale
        assert hit.sum() > 500
        assert ((t[k].double() - t_ref)[hit].abs() * scale[hit]).max() <= _h(n)
    # the legacy appearance branch trains on the extracted shells
    m = VolSurfs.from_meshes_path(out, str(tmp_path / "ckpt"), using_neural_textures=False, max_rays=4096,
                                  rgb_mlp_layers_dims=(64, 32), bb_sides=1.0, sh_degree=3)
    o2, d2 = pinhole_rays(32, 32, focal=40.0, cam_pos=(0.0, 0.0, -1.6))
    gt = torch.rand(o2.shape[0], 3, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    loss = m(o2, d2, gt, iter_nr=0, is_first_iter=True)[0]["loss"]
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)


@pytest.mark.gpu
def test_scale_n1000_five_levels():
    n, K = 1000, 5
    assert iso.workspace_bytes((n, n, n), K) < 1 << 30
    grid = iso.sample_grid(lambda p: torch.linalg.vector_norm(p, dim=-1)[:, None], n, chunk=128)
    levels = [0.3, 0.32, 0.34, 0.36, 0.38]
    meshes = iso.marching_cubes(grid, levels, [-1.0] * 3, [_h(n)] * 3)
    for m, lv in zip(meshes, levels):
        ins = grid < lv
        crossed = (int((ins[1:] != ins[:-1]).sum()) + int((ins[:, 1:] != ins[:, :-1]).sum()) +
                   int((ins[:, :, 1:] != ins[:, :, :-1]).sum()))
        assert m.vertices.shape[0] == crossed > 300000
        assert int(m.faces.max()) == crossed - 1 and int(m.faces.min()) == 0
