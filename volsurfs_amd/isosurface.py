"""Nested level-set shells from a field on the device: the mesh-extraction half of the reference's baker
(volsurfs_py/baker.py:324-452, utils/mesh_extraction.py:224-373) with marching cubes in HIP
(csrc/isosurface.hip, rules in include/volsurfs_hip.h and DESIGN §14).

* `marching_cubes` — K level sets of one fp32 device grid in one count pass and one emit pass; the
  output order and bits depend on the grid and the levels only.
* `sample_grid` — a torch callable evaluated on the reference's `linspace` lattice straight into a
  device grid (no host copy).
* `extract_mesh_from_fn` — `extract_o3d_mesh_from_fn` on top of the two: shift, threshold, range
  check and the bounding-primitive filter, on the device.
* `extract_level_sets` / `save_level_sets` — the baker's `--extract_meshes` rule for K shells (one
  grid, one kernel call) and its `meshes/<level>.ply` files, which `mesh.load_meshes_indexed_from_path`
  reads back inner to outer.

The triangle table `MC_TABLE` is built here by `build_mc_table` and compiled into the library from
`csrc/mc_table.h` (tools/gen_mc_table.py writes it; `vsa_mc_table` hands the compiled copy back).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .mesh import TensorMesh, save_ply

MAX_LEVELS = 16

# Cube corner c sits at offset (c & 1, c >> 1 & 1, c >> 2 & 1) along (x, y, z).
CORNER_OFFSETS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.int64)
# Edge e = 4 * axis + q: the grid edge along `axis` owned by (starting at) the corner at EDGE_OWNERS[e].
EDGE_OWNERS = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 1],      # x edges
                        [0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1],      # y edges
                        [0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]],     # z edges
                       np.int64)
EDGE_AXES = np.repeat(np.arange(3), 4)


def _corner(o):
    return int(o[0]) | int(o[1]) << 1 | int(o[2]) << 2


def _edge_corners():
    out = []
    for o, a in zip(EDGE_OWNERS, EDGE_AXES):
        b = o.copy()
        b[a] += 1
        out.append((_corner(o), _corner(b)))
    return out


def _cube_faces():
    """The six faces as corner lists, counter-clockwise seen from outside the cube."""
    faces = []
    for ax in range(3):
        for side in (0, 1):
            n = np.zeros(3)
            n[ax] = 1.0 if side else -1.0
            cs = [c for c in range(8) if CORNER_OFFSETS[c][ax] == side]
            cen = CORNER_OFFSETS[cs].mean(0)
            u = np.zeros(3)
            u[(ax + 1) % 3] = 1.0
            v = np.cross(n, u)
            ang = [np.arctan2((CORNER_OFFSETS[c] - cen) @ v, (CORNER_OFFSETS[c] - cen) @ u) for c in cs]
            faces.append([cs[i] for i in np.argsort(ang)])
    return faces


def build_mc_table():
    """The 256-case triangle table, int8 [256, 16]: up to five triangles of edge ids, -1 padded.

    Built from one rule, so that neighbouring cells agree on every shared face and closed surfaces come out
    watertight:
      * on each cube face, the crossed edges are joined by segments with the inside on their left seen from
        outside the cube; a face with four crossings (two diagonal inside corners) cuts each inside corner off
        on its own (inside corners are never joined across a face);
      * the segments chain into loops, and each loop is fanned from the first of its edges (in loop order,
        starting from its smallest edge id) whose diagonals join no two edges that share a cube face, so a
        fan diagonal never coincides with a segment or diagonal of the neighbouring cell;
      * triangles are wound so that (v1 - v0) x (v2 - v0) points out of the inside region."""
    ev = _edge_corners()
    edge_of = {frozenset(p): e for e, p in enumerate(ev)}
    faces = _cube_faces()
    face_sets = [set(f) for f in faces]

    def share_face(a, b):
        return any(set(ev[a]) <= s and set(ev[b]) <= s for s in face_sets)

    tab = np.full((256, 16), -1, np.int8)
    for case in range(256):
        ins = [(case >> c) & 1 for c in range(8)]
        nxt = {}
        for fc in faces:
            crossings = [(edge_of[frozenset((fc[q], fc[(q + 1) % 4]))], ins[fc[q]])
                         for q in range(4) if ins[fc[q]] != ins[fc[(q + 1) % 4]]]
            if len(crossings) == 2:
                leave = next(e for e, was_in in crossings if was_in)
                enter = next(e for e, was_in in crossings if not was_in)
                nxt[leave] = enter
            elif len(crossings) == 4:
                for q in range(4):
                    if ins[fc[q]]:
                        nxt[edge_of[frozenset((fc[q], fc[(q + 1) % 4]))]] = \
                            edge_of[frozenset((fc[(q - 1) % 4], fc[q]))]
        seen, tris = set(), []
        for e0 in sorted(nxt):
            if e0 in seen:
                continue
            loop, e = [e0], nxt[e0]
            seen.add(e0)
            while e != e0:
                loop.append(e)
                seen.add(e)
                e = nxt[e]
            for s in range(len(loop)):
                fan = loop[s:] + loop[:s]
                if not any(share_face(fan[0], fan[j]) for j in range(2, len(fan) - 1)):
                    break
            else:
                raise AssertionError(f"marching-cubes case {case}: no fan without a face diagonal")
            tris += [(fan[0], fan[j + 1], fan[j]) for j in range(1, len(fan) - 1)]
        assert len(tris) <= 5
        for t, tri in enumerate(tris):
            tab[case, 3 * t:3 * t + 3] = tri
    return tab


MC_TABLE = build_mc_table()


def device_mc_table():
    """The table compiled into the library (vsa_mc_table), int8 [256, 16]."""
    out = np.zeros(256 * 16, np.int8)
    _lib.call("vsa_mc_table", out.ctypes.data_as(ctypes.c_void_p))
    return out.reshape(256, 16)


def _ptr_array(ptrs):
    arr = (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def workspace_bytes(shape, nr_levels):
    """Device workspace of one `marching_cubes` call on a grid of `shape` with `nr_levels` levels."""
    nx, ny, nz = (int(s) for s in shape)
    n = _lib.lib().vsa_isosurface_workspace_bytes(nx, ny, nz, int(nr_levels))
    if n < 0:
        raise _lib.VolsurfsHipError(f"vsa_isosurface_workspace_bytes failed with status {n}")
    return int(n)


def _empty_mesh(device):
    return _uvless(torch.zeros(0, 3, device=device), torch.zeros(0, 3, dtype=torch.int32, device=device))


def _uvless(vertices, faces):
    """A TensorMesh as load_ply returns a file without texcoords: zero per-corner UVs, has_uvs False."""
    m = TensorMesh(vertices, faces, torch.zeros(faces.shape[0], 3, 2, device=faces.device), device=faces.device)
    m.has_uvs = False
    return m


@torch.no_grad()
def marching_cubes(grid, levels, origin, spacing, inside="below"):
    """Level sets of a C-contiguous fp32 device grid [nx, ny, nz] (value (i, j, k) = f(x_i, y_j, z_k)) with grid
    point (i, j, k) at origin + (i, j, k) * spacing.  `levels`: one float or a list of 1..16 (any order).
    `inside`: "below" (a corner is inside when value < level, an SDF's convention) or "above" (value > level).
    Returns one TensorMesh per level, in the order given: vertices [V, 3] f32 (one per crossed grid edge), faces
    [F, 3] i32 wound outward from the inside region, zero UVs with has_uvs False."""
    if inside not in ("below", "above"):
        raise ValueError(f"inside must be 'below' or 'above', got {inside!r}")
    levels = [float(levels)] if np.isscalar(levels) else [float(x) for x in levels]
    K = len(levels)
    if grid.dim() != 3:
        raise _lib.VolsurfsHipError(f"marching_cubes: expected a 3-D grid, got shape {tuple(grid.shape)}")
    grid = _lib.check_f32(grid)
    nx, ny, nz = (int(s) for s in grid.shape)
    if not 1 <= K <= MAX_LEVELS or min(nx, ny, nz) < 2:
        raise _lib.VolsurfsHipError(f"marching_cubes: 1..{MAX_LEVELS} levels on a grid of at least 2^3 points, "
                                    f"got {K} levels on {tuple(grid.shape)}")
    if not bool(torch.isfinite(grid).all()):
        raise _lib.VolsurfsHipError("marching_cubes: the grid holds NaN or inf (no inside / outside for them)")
    lv = (ctypes.c_float * K)(*levels)
    org = (ctypes.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(origin, np.float64), 3)])
    spc = (ctypes.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(spacing, np.float64), 3)])
    above = 1 if inside == "above" else 0
    ws = torch.empty(workspace_bytes(grid.shape, K), dtype=torch.uint8, device=grid.device)
    totals = (ctypes.c_longlong * (2 * K))()
    _lib.call("vsa_isosurface_count", grid, nx, ny, nz, ctypes.cast(lv, ctypes.c_void_p), K, above, ws, ws.numel(),
              ctypes.cast(totals, ctypes.c_void_p), _lib.stream_ptr())
    verts = [torch.empty(int(totals[2 * L]), 3, device=grid.device) for L in range(K)]
    faces = [torch.empty(int(totals[2 * L + 1]), 3, dtype=torch.int32, device=grid.device) for L in range(K)]
    _va, vp = _ptr_array([v.data_ptr() for v in verts])
    _fa, fp = _ptr_array([f.data_ptr() for f in faces])
    _lib.call("vsa_isosurface_emit", grid, nx, ny, nz, ctypes.cast(lv, ctypes.c_void_p), K, above,
              ctypes.cast(org, ctypes.c_void_p), ctypes.cast(spc, ctypes.c_void_p), ws, ws.numel(),
              ctypes.cast(totals, ctypes.c_void_p), vp, fp, _lib.stream_ptr())
    return [_uvless(v, f) for v, f in zip(verts, faces)]


@torch.no_grad()
def sample_grid(fn, nr_points_per_dim, scene_radius=1.0, out_idx=None, iter_nr=None, chunk=64, device="cuda",
                nr_columns=None):
    """mesh_extraction.py:248-305 without the host copy: fn evaluated on the lattice
    X, Y, Z = torch.linspace(-r, r, n) (fp32) with indexing "ij", in chunk^3 blocks, into a device grid
    [n, n, n] f32 (grid[i, j, k] = fn(X[i], Y[j], Z[k])).  fn takes points [P, 3] (and iter_nr= when given); a
    tuple output gives its first element, `out_idx` selects a column.  With `nr_columns` = K, all K output columns
    of fn ([P, K] or [P, K, 1]) from one pass into a grid [K, n, n, n]."""
    n, r = int(nr_points_per_dim), float(scene_radius)
    axis = torch.linspace(-r, r, n, dtype=torch.float32).to(device)
    K = None if nr_columns is None else int(nr_columns)
    grid = torch.empty(n, n, n, device=device) if K is None else torch.empty(K, n, n, n, device=device)
    for x0 in range(0, n, chunk):
        for y0 in range(0, n, chunk):
            for z0 in range(0, n, chunk):
                xs, ys, zs = axis[x0:x0 + chunk], axis[y0:y0 + chunk], axis[z0:z0 + chunk]
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1)
                pred = fn(pts) if iter_nr is None else fn(pts, iter_nr=iter_nr)
                if isinstance(pred, tuple):
                    pred = pred[0]
                if out_idx is not None:
                    pred = pred[:, out_idx]
                if K is None:
                    grid[x0:x0 + len(xs), y0:y0 + len(ys), z0:z0 + len(zs)] = \
                        pred.reshape(len(xs), len(ys), len(zs)).to(torch.float32)
                else:
                    grid[:, x0:x0 + len(xs), y0:y0 + len(ys), z0:z0 + len(zs)] = \
                        pred.reshape(pts.shape[0], K).t().reshape(K, len(xs), len(ys), len(zs)).to(torch.float32)
    return grid


@torch.no_grad()
def filter_inside(mesh, bounding_primitive):
    """mesh_extraction.py:354-371: keep the faces whose three vertices are all inside the primitive, then drop
    the vertices no kept face references; both orders are kept.  On the device."""
    V, F = mesh.vertices, mesh.faces.long()
    if F.shape[0] == 0:
        return mesh
    inside = bounding_primitive.check_points_inside(V).reshape(-1)
    F = F[inside[F].all(-1)]
    used = torch.zeros(V.shape[0], dtype=torch.bool, device=V.device)
    used[F.reshape(-1)] = True
    new_id = torch.cumsum(used.to(torch.int64), 0) - 1
    return _uvless(V[used], new_id[F].to(torch.int32))


def _radius(bounding_primitive):
    return 1.0 if bounding_primitive is None else float(bounding_primitive.get_radius())


def _lattice(n, r):
    """Origin and spacing of sample_grid's lattice, as the reference maps skimage's index-space vertices back:
    v / (n - 1) * (max - min) + min (mesh_extraction.py:325) with min = -r, max = r."""
    return [-r] * 3, [2.0 * r / (n - 1)] * 3


def _finish(grid, levels, n, bounding_primitive, threshold=None, inside="below"):
    origin, spacing = _lattice(n, _radius(bounding_primitive))
    if threshold is not None:
        lo, hi = torch.aminmax(grid)
        if not float(lo) <= threshold <= float(hi):
            return [_empty_mesh(grid.device)]
    meshes = marching_cubes(grid, levels, origin, spacing, inside=inside)
    if bounding_primitive is not None:
        meshes = [filter_inside(m, bounding_primitive) for m in meshes]
    return meshes


def extract_mesh_from_fn(fn, nr_points_per_dim, bounding_primitive=None, out_idx=None, level_set=0.0, threshold=0.0,
                         iter_nr=None):
    """extract_o3d_mesh_from_fn (mesh_extraction.py:224-373) on the device: the lattice of radius
    bounding_primitive.get_radius() (else 1), the grid shifted by `level_set` (fp32), marching cubes at
    `threshold`, an empty mesh when the threshold lies outside [min, max] of the grid, and the faces not wholly
    inside the bounding primitive dropped.  Returns a TensorMesh (no UVs)."""
    grid = sample_grid(fn, nr_points_per_dim, _radius(bounding_primitive), out_idx=out_idx, iter_nr=iter_nr)
    grid -= float(level_set)
    return _finish(grid, [float(threshold)], int(nr_points_per_dim), bounding_primitive, float(threshold))[0]


def level_set_values(nr_meshes, delta_surfs=0.0025, extract_level_set=0.0):
    """The baker's levels (baker.py:334-341, 363-369): torch.linspace(-d (K // 2), d (K // 2), K) rounded to 4
    decimals, or [extract_level_set] rounded for K = 1."""
    K = int(nr_meshes)
    if K > 1:
        off = delta_surfs * (K // 2)
        return [round(x.item(), 4) for x in torch.linspace(-off, off, K)]
    return [round(float(extract_level_set), 4)]


def extract_level_sets(fn, nr_points_per_dim, nr_meshes, delta_surfs=0.0025, extract_level_set=0.0,
                       bounding_primitive=None, out_idx=None, iter_nr=None):
    """The baker's `--extract_meshes` for the surf / nerf methods: the K level sets of one field, from ONE grid
    evaluation and ONE K-level marching-cubes call (the reference evaluates the field K times).  Each shell has the
    faces of extract_mesh_from_fn(..., level_set=level, threshold=0) exactly (fl(f - level) < 0 iff f < level);
    its vertices differ only by the rounding of that shift, since the crossing is interpolated on f at `level`
    instead of on f - level at 0.  A level the grid does not cross comes out with no faces.  Returns
    (meshes, levels), inner to outer (ascending level)."""
    levels = sorted(level_set_values(nr_meshes, delta_surfs, extract_level_set))
    if len(levels) > MAX_LEVELS:
        raise _lib.VolsurfsHipError(f"extract_level_sets: at most {MAX_LEVELS} levels, got {len(levels)}")
    n = int(nr_points_per_dim)
    grid = sample_grid(fn, n, _radius(bounding_primitive), out_idx=out_idx, iter_nr=iter_nr)
    return _finish(grid, levels, n, bounding_primitive), levels


NERF_DENSITY_SHIFT = 0.5      # mesh_extraction.py:473-483: level_set=0.5, threshold=<the baker's level>


def extract_nerf_level_sets(method, nr_points_per_dim, nr_meshes=1, delta_surfs=0.0025, extract_level_set=0.0,
                            iter_nr=None):
    """The baker's `--extract_meshes` for the nerf method (baker.py:325-369, mesh_extraction.py:473-483): the density
    field of `method.models["density"]` on the lattice of the method's bounding primitive, shifted by 0.5, cut at the
    baker's levels (level_set_values) with the inside where the density is ABOVE the level, so that the faces wind
    outward from the dense region; faces not wholly inside the bounding primitive are dropped.  One grid evaluation
    and one marching-cubes call for all levels.  Returns (meshes, levels) in ascending level, which for a density
    blob runs from the outer shell to the inner one (a higher density level lies inside a lower one)."""
    levels = sorted(level_set_values(nr_meshes, delta_surfs, extract_level_set))
    if len(levels) > MAX_LEVELS:
        raise _lib.VolsurfsHipError(f"extract_nerf_level_sets: at most {MAX_LEVELS} levels, got {len(levels)}")
    n = int(nr_points_per_dim)
    bp = method.bounding_primitive
    grid = sample_grid(method.models["density"], n, _radius(bp), iter_nr=iter_nr)
    grid -= NERF_DENSITY_SHIFT
    return _finish(grid, levels, n, bp, inside="above"), levels


def extract_surf_level_sets(method, nr_points_per_dim, nr_meshes=1, delta_surfs=0.0025, extract_level_set=0.0,
                            iter_nr=None):
    """The baker's `--extract_meshes` for the surf method (baker.py:325-369): column 0 of
    `method.models["sdf"].main_sdf` on the lattice of the method's bounding primitive, cut at the baker's levels
    (level_set_values) with the inside BELOW the level, faces not wholly inside the bounding primitive dropped.
    One grid evaluation and one marching-cubes call for all levels.  Returns (meshes, levels) in ascending level,
    inner to outer."""
    return extract_level_sets(method.models["sdf"].main_sdf, nr_points_per_dim, nr_meshes, delta_surfs,
                              extract_level_set, bounding_primitive=method.bounding_primitive, out_idx=0,
                              iter_nr=iter_nr)


def extract_offsets_surfs_meshes(method, nr_points_per_dim, nr_meshes_to_extract=1, delta_surfs=0.0025,
                                 extract_level_set=0.0, iter_nr=None):
    """The baker's `--extract_meshes` for the offsets_surfs method (baker.py:325-369).  nr_meshes_to_extract == 1:
    the zero level of each of the K sdfs of `method.models["sdfs"]` (all K columns from one pass over the lattice),
    inner to outer, levels [0.0] * K.  nr_meshes_to_extract > 1: the baker's level sets of the main surface, as
    extract_surf_level_sets.  Inside is below the level; faces not wholly inside the bounding primitive are dropped.
    Returns (meshes, levels)."""
    model = method.models["sdfs"]
    bp = method.bounding_primitive
    n = int(nr_points_per_dim)
    if int(nr_meshes_to_extract) > 1:
        return extract_level_sets(model.main_sdf, n, nr_meshes_to_extract, delta_surfs, extract_level_set,
                                  bounding_primitive=bp, out_idx=0, iter_nr=iter_nr)
    K = model.nr_surfs
    grid = sample_grid(model, n, _radius(bp), iter_nr=iter_nr, nr_columns=K)
    meshes = [_finish(grid[k].contiguous(), [0.0], n, bp)[0] for k in range(K)]
    return meshes, [0.0] * K


def save_offsets_surfs_meshes(meshes, out_dir):
    """The K-SDF mode's `meshes/<i>.ply` files (i = 0 the innermost); an empty surface raises.  Returns the paths."""
    for i, m in enumerate(meshes):
        if m.faces.shape[0] == 0:
            raise ValueError(f"surface {i} has no faces: nothing to save")
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for i, m in enumerate(meshes):
        path = os.path.join(out_dir, f"{i}.ply")
        save_ply(path, TensorMesh(m.vertices, m.faces, None, device=m.vertices.device))
        paths.append(path)
    return paths


def save_level_sets(meshes, levels, out_dir):
    """The baker's `meshes/<round(level, 4)>.ply` files (baker.py:375-390), without texcoords; an empty level
    raises (load_ply refuses a file without geometry).  Returns the paths."""
    if len(meshes) != len(levels):
        raise ValueError(f"{len(meshes)} meshes for {len(levels)} levels")
    for m, lv in zip(meshes, levels):
        if m.faces.shape[0] == 0:
            raise ValueError(f"level {round(float(lv), 4)} has no faces: nothing to save")
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for m, lv in zip(meshes, levels):
        path = os.path.join(out_dir, f"{round(float(lv), 4)}.ply")
        save_ply(path, TensorMesh(m.vertices, m.faces, None, device=m.vertices.device))
        paths.append(path)
    return paths
