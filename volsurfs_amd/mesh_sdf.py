"""On which side of a mesh a point is, on the device: the signed distance to a mesh, the field on `sample_grid`'s lattice,
and nested shells cut from it for any mesh.  The reference has no such stage: the rule is this library's own
(include/volsurfs_hip.h "Mesh signed distance"), restated in tests/mesh_sdf_restated.py and unpinned.

The distance is `mesh_distance`'s (the closest-point walk of the q16 nodes); its sign is that of r . N, N the
angle-weighted pseudonormal of the closest feature (Baerentzen & Aanaes 2005): negative inside a closed mesh whose faces
wind outward, as `marching_cubes` and `icosphere` wind them.  The sign means inside / outside for closed, consistently
oriented meshes only; for any other mesh it is whatever the rule gives.

Every entry point below takes `sign="pseudonormal"` (the default: the rule above), `"winding"` or `"auto"`, and `beta`.
With `"winding"` a point is inside iff the generalised winding number of the mesh there exceeds 1/2
(`mesh_winding.winding_number(points, mesh, beta)`; "Mesh winding number"), for faces that wind outward:
that also means something for open, self-intersecting and inconsistently wound meshes.  Across a hole the level sets
close with the w = 1/2 membrane; the field jumps from -d to +d there, so all K shells of `offset_shells` cross it within
one cell, in level order: nested, but crowded.  `"auto"` takes the winding number iff `mesh_winding.edge_census` finds a
boundary, a non-manifold or an inconsistently wound edge.  An unknown value raises ValueError.

A mesh is a cuda `TensorMesh` or a pair `(RayTracer, mesh_id)`, as in `mesh_distance`.

* `pseudonormals` — the table [F, 7, 3] of a mesh (csrc/mesh_sdf.hip: vsa_mesh_pseudonormals).
* `signed_distance`, `contains` — per point.
* `mesh_to_sdf_grid` — the field on `sample_grid`'s lattice, clamped to a band, in one call (vsa_mesh_sdf_grid).
* `offset_shells`, `offset_meshes` — the K level sets `level_set_values` names, from a mesh or a mesh file: what
  `simplify_meshes` -> `compute_meshes_atlas` -> `VolSurfs.from_meshes_path` take over, without a trained field.
* `shell_nesting` — is every shell inside the next one?  The signed companion of `mesh_distance.shell_clearance`.
"""
import ctypes
import math
import os

import torch

from . import _lib
from .isosurface import MAX_LEVELS, _lattice, level_set_values, marching_cubes, save_level_sets
from .mesh import TensorMesh, check_mesh, load_mesh
from .mesh_distance import _check_n, _resolve, sample_surface
from .raytrace import RayTracer

REGIONS = ("A", "B", "C", "AB", "AC", "BC", "in")        # the table's entries, by region code


@torch.no_grad()
def pseudonormals(mesh, device=None):
    """[F, 7, 3] f32: per face (original face id) the pseudonormals of its three vertices, its three edges (v0 v1, v0 v2,
    v1 v2) and its own normal, in the order of `REGIONS`: fp64 sums over the vertex rings and the edges' faces in
    ascending face id, stored as fp32.  A zero-area face contributes nothing.  The same mesh gives the same bytes."""
    if device is not None and mesh.vertices.device != torch.device(device):
        mesh = TensorMesh(mesh.vertices, mesh.faces, None, device=device)
    V, F = check_mesh(mesh, "pseudonormals")
    if F.shape[0] < 1:
        raise ValueError("pseudonormals: the mesh has no faces")
    nbytes = _lib.workspace_bytes("vsa_mesh_pseudonormals_workspace_bytes", V.shape[0], F.shape[0])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=V.device)
    table = torch.empty(F.shape[0], len(REGIONS), 3, device=V.device)
    _lib.call("vsa_mesh_pseudonormals", V, V.shape[0], F, F.shape[0], ws, nbytes, table, _lib.stream_ptr())
    return table


@torch.no_grad()
def signed_distance(points, mesh, sign="pseudonormal", beta=2.0):
    """{dist [N] (signed: negative inside), face [N], slot [N], bary [N, 2]} of the closest point of `mesh` to each of
    points [N, 3] f32 (cuda): `mesh_distance.closest_points` with the sign (`RayTracer.signed_distance`).
    sign="winding": inside iff the winding number exceeds 1/2 (the module's text); "auto": by the edge census."""
    tracer, mesh_id = _resolve(mesh, "signed_distance")
    return tracer.signed_distance(points, mesh_id, sign=sign, beta=beta)


@torch.no_grad()
def contains(points, mesh, sign="pseudonormal", beta=2.0):
    """[N] bool: is the point inside the mesh (signed distance < 0; a point on the surface is not).  sign="winding":
    inside iff the winding number exceeds 1/2, whether the mesh is closed or not."""
    return signed_distance(points, mesh, sign=sign, beta=beta)["dist"] < 0


def _axis(n, r, device):
    """sample_grid's axis: the values torch.linspace gives, not origin + i * spacing."""
    return torch.linspace(-r, r, n, dtype=torch.float32).to(device)


def _grid(handle, x, y, z, band, sign="pseudonormal", beta=2.0):
    tracer, mesh_id = handle
    tracer.require_q16("mesh_to_sdf_grid")
    band = math.inf if band is None else float(band)
    if not band > 0.0:
        raise ValueError(f"mesh_to_sdf_grid: band must be > 0 (None: the whole field), got {band}")
    if tracer.sign_rule(sign, [mesh_id]) == "winding":
        return _grid_w(tracer, mesh_id, x, y, z, band, tracer._check_beta(beta))
    table, base = tracer.pseudonormal_tables()
    x, y, z = (_lib.check_f32(a.contiguous(), a.shape[0]) for a in (x, y, z))
    nx, ny, nz = x.shape[0], y.shape[0], z.shape[0]
    nbytes = _lib.workspace_bytes("vsa_mesh_sdf_grid_workspace_bytes", nx, ny, nz) if band < math.inf else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=tracer.device) if nbytes else None
    grid = torch.empty(nx, ny, nz, device=tracer.device)
    counts = (ctypes.c_longlong * 2)()
    qnodes, tris, root, frame, _, depth = tracer.q16_tree_args(mesh_id)
    _lib.call("vsa_mesh_sdf_grid", qnodes, tris, root[0], frame, depth, table, int(base[mesh_id]), x, y, z, nx, ny, nz,
              band, grid, ws, nbytes, ctypes.cast(counts, ctypes.c_void_p), _lib.stream_ptr())
    return grid, {"near_bricks": int(counts[0]), "far_bricks": int(counts[1])}


def _grid_w(tracer, mesh_id, x, y, z, band, beta):
    """`_grid` with the winding sign (vsa_mesh_sdf_grid_w)."""
    table, entries = tracer.winding_moments()
    x, y, z = (_lib.check_f32(a.contiguous(), a.shape[0]) for a in (x, y, z))
    nx, ny, nz = x.shape[0], y.shape[0], z.shape[0]
    nbytes = _lib.workspace_bytes("vsa_mesh_sdf_grid_w_workspace_bytes", nx, ny, nz) if band < math.inf else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=tracer.device) if nbytes else None
    grid = torch.empty(nx, ny, nz, device=tracer.device)
    counts = (ctypes.c_longlong * 2)()
    qnodes, tris, root, frame, _, depth = tracer.q16_tree_args(mesh_id)
    _lib.call("vsa_mesh_sdf_grid_w", qnodes, tris, root[0], frame, depth, table, int(entries[mesh_id]), beta, x, y, z,
              nx, ny, nz, band, grid, ws, nbytes, ctypes.cast(counts, ctypes.c_void_p), _lib.stream_ptr())
    return grid, {"near_bricks": int(counts[0]), "far_bricks": int(counts[1])}


@torch.no_grad()
def sdf_grid(mesh, x, y, z, band=None, sign="pseudonormal", beta=2.0):
    """(grid [nx, ny, nz] f32, {near_bricks, far_bricks}): clamp(signed distance to `mesh` at (x[i], y[j], z[k]), -band,
    band) for three device axis arrays (vsa_mesh_sdf_grid; sign="winding": vsa_mesh_sdf_grid_w, bit for bit the point
    query with that sign).  band None: the whole field."""
    return _grid(_resolve(mesh, "sdf_grid"), x, y, z, band, sign, beta)


@torch.no_grad()
def mesh_to_sdf_grid(mesh, nr_points_per_dim, scene_radius=1.0, band=None, sign="pseudonormal", beta=2.0):
    """(grid [n, n, n] f32, {near_bricks, far_bricks}): the signed distance to `mesh` on `sample_grid`'s lattice of
    radius `scene_radius`, bit for bit `sample_grid(lambda p: signed_distance(p, mesh)["dist"], n, scene_radius)`
    clamped to [-band, band] (None: not clamped).  A wave walks a 4 x 4 x 4 brick of lattice points; with a band, bricks
    farther from the surface than the band plus their own radius are filled with +-band from one query at their centre
    (far_bricks) and only the others are walked (near_bricks).  One blocking read with a band, none without.
    sign="winding": the same contract with `signed_distance(p, mesh, sign="winding", beta=beta)`; bricks are classified
    on the unsigned distance, and a far brick still takes the winding number at each of its points (it crosses 1/2 away
    from the surface, on the membrane that closes a hole), so only the closest-point walk is saved there."""
    handle = _resolve(mesh, "mesh_to_sdf_grid")
    n = int(nr_points_per_dim)
    if n < 2:
        raise ValueError(f"mesh_to_sdf_grid: nr_points_per_dim must be >= 2, got {n}")
    axis = _axis(n, float(scene_radius), handle[0].device)
    return _grid(handle, axis, axis, axis, band, sign, beta)


@torch.no_grad()
def offset_shells(mesh, nr_meshes, delta_surfs=0.0025, extract_level_set=0.0, nr_points_per_dim=512, scene_radius=1.0,
                  band=None, sign="pseudonormal", beta=2.0, repair=False, return_report=False):
    """(meshes, levels), inner to outer: the level sets `level_set_values(nr_meshes, delta_surfs, extract_level_set)`
    of the signed distance to `mesh`, from one banded grid and one K-level `marching_cubes` call.  The band is
    max |level| + 2 |spacing| (|spacing| the lattice cell's diagonal) unless given; a band that does not exceed every
    |level| by a cell's diagonal cannot hold the level's crossings and raises.  sign="winding" (or "auto" on a mesh
    that is not closed): shells from an open mesh; they close across its holes along the w = 1/2 membrane, where all K
    of them lie within one cell of each other.  `repair`: the mesh (a TensorMesh) goes through
    `mesh_repair.repair_mesh` first, so that a soup or a mis-wound mesh takes the sign it would have taken clean;
    `return_report` adds that report (None without `repair`) as a third element."""
    report = None
    if repair:
        from .mesh_repair import repair_mesh
        if isinstance(mesh, tuple):
            raise TypeError("offset_shells: repair=True takes a TensorMesh, not a (RayTracer, mesh_id) pair")
        mesh, report = repair_mesh(mesh)
    levels = sorted(level_set_values(nr_meshes, delta_surfs, extract_level_set))
    if len(levels) > MAX_LEVELS:
        raise _lib.VolsurfsHipError(f"offset_shells: at most {MAX_LEVELS} levels, got {len(levels)}")
    n, r = int(nr_points_per_dim), float(scene_radius)
    origin, spacing = _lattice(n, r)
    diag = math.sqrt(3.0) * spacing[0]
    top = max(abs(lv) for lv in levels)
    band = top + 2.0 * diag if band is None else float(band)
    if not band >= top + diag:
        raise ValueError(f"offset_shells: a band of {band} cannot hold the level {top} on a lattice whose cells are "
                         f"{diag} across (it takes at least {top + diag})")
    grid, _ = mesh_to_sdf_grid(mesh, n, r, band, sign, beta)
    meshes = marching_cubes(grid, levels, origin, spacing)
    return (meshes, levels, report) if return_report else (meshes, levels)


def offset_meshes(mesh_path, out_dir, nr_meshes, delta_surfs=0.0025, extract_level_set=0.0, nr_points_per_dim=512,
                  scene_radius=1.0, sign="pseudonormal", beta=2.0, repair=False, return_report=False):
    """`offset_shells` of the PLY / OBJ at `mesh_path`, written as `<out_dir>/meshes/<level>.ply` (`save_level_sets`):
    the layout `simplify_meshes`, `compute_meshes_atlas` and `VolSurfs.from_meshes_path` continue from.  Returns
    (paths, levels); `repair` and `return_report` as in `offset_shells`."""
    mesh = load_mesh(mesh_path)
    meshes, levels, report = offset_shells(TensorMesh(mesh.vertices, mesh.faces, None, device=mesh.vertices.device),
                                           nr_meshes, delta_surfs, extract_level_set, nr_points_per_dim, scene_radius,
                                           sign=sign, beta=beta, repair=repair, return_report=True)
    paths = save_level_sets(meshes, levels, os.path.join(out_dir, "meshes"))
    return (paths, levels, report) if return_report else (paths, levels)


@torch.no_grad()
def shell_nesting(meshes, n=1_000_000, seed=0, sign="pseudonormal", beta=2.0):
    """Is every shell inside the next one?  For each consecutive pair (k, k + 1): n samples of shell k
    (`sample_surface(shell k, n, seed)`) and their signed distance d to shell k + 1; a list of K - 1 dicts {pair,
    outside = the number of samples with d >= 0 (not inside), clearance = -max d (the smallest depth of a sample below
    shell k + 1; negative when a sample is outside)}.  `meshes`: a list of TensorMeshes (one tracer is built for all of
    them) or a RayTracer.  The signed companion of `mesh_distance.shell_clearance`.  sign="winding": inside means a
    winding number above 1/2, for shells that are not closed."""
    n = _check_n(n, "shell_nesting")
    tracer = RayTracer.over(meshes)
    out = []
    for k in range(tracer.nr_meshes - 1):
        points, _, _ = sample_surface(_resolve((tracer, k), "shell_nesting"), n, seed)
        d = tracer.signed_distance(points, k + 1, sign=sign, beta=beta)["dist"]
        outside, top = torch.stack([(d >= 0).sum().double(), d.max().double()]).cpu().tolist()
        out.append({"pair": (k, k + 1), "outside": int(outside), "clearance": -top})
    return out


__all__ = ["REGIONS", "pseudonormals", "signed_distance", "contains", "sdf_grid", "mesh_to_sdf_grid", "offset_shells",
           "offset_meshes", "shell_nesting"]
