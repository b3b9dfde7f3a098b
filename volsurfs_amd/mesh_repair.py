"""Mesh repair on the device: welding the vertices that are one point and winding every edge-connected component
consistently, normals outward (csrc/mesh_repair.hip; rules in include/volsurfs_hip.h "Mesh repair" and DESIGN §32).  The
reference has no such stage: the rules are this library's own, restated in tests/mesh_repair_restated.py and unpinned.

A mesh from outside the pipeline is often a triangle soup (an STL, an OBJ split at its UV seams) or wound at random.
`mesh_winding.edge_census` finds that; this module mends it, so that `mesh_sdf`'s cheap, exact pseudonormal sign applies
to a mesh whose only fault is its bookkeeping, and the winding number of an open one has the right sign.

* `weld_vertices` — merge equal vertices (tol = 0: equal bits) or vertices linked by a chain of steps within `tol`;
  drop the degenerate and duplicate faces that leaves.
* `orient_faces` — relative orientation by a union-find over the double cover, then outward per component.
* `repair_mesh` — both, with the edge census before and after.
* `repair_meshes` — every `<level>.ply` / `.obj` of a directory repaired into another (`meshes_repaired/`).
"""
import ctypes
import os

import torch

from . import _lib
from .isosurface import _uvless
from .mesh import TensorMesh, check_mesh, level_files, load_mesh, save_ply
from .mesh_clean import _rebuild, _uvs

WELD_STAGES = ("group", "vertices", "duplicates", "faces")
ORIENT_STAGES = ("edges", "hook", "roots", "sums", "flip")
UNSUPPORTED = -2


def _status(name, *args):
    """`_lib.call` that hands the status back instead of raising on VSA_ERR_UNSUPPORTED."""
    fn = getattr(_lib.lib(), name)
    rc = fn(*[_lib._conv(a, True) for a in args])
    if rc not in (0, UNSUPPORTED):
        raise _lib.VolsurfsHipError(f"{name} failed with status {rc}")
    return rc


def _check_weld(mesh, what):
    """`check_mesh` without its refusal of NaN and inf: a NaN vertex is welded with nothing."""
    V, F = mesh.vertices, mesh.faces
    if not (V.is_cuda and F.is_cuda):
        raise ValueError(f"{what}: the mesh must be on cuda, got {V.device} / {F.device}")
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
        raise ValueError(f"{what}: expected vertices [V, 3] and faces [F, 3], got {tuple(V.shape)} / {tuple(F.shape)}")
    V = V.to(torch.float32).contiguous()
    F = F.to(torch.int32).contiguous()
    if F.shape[0]:
        lo, hi = torch.aminmax(F)
        if int(lo) < 0 or int(hi) >= V.shape[0]:
            raise _lib.VolsurfsHipError(f"{what}: face indices out of range [0, {V.shape[0]}): min {int(lo)}, "
                                        f"max {int(hi)}")
    return V, F


def _stage_ptr(ms):
    return ctypes.cast(ms, ctypes.c_void_p) if ms is not None else None


@torch.no_grad()
def weld_vertices(mesh, tol=0.0, drop_degenerate=True, drop_duplicates=True, vertex_colors=None, stage_ms=None):
    """Merge the vertices of a cuda TensorMesh that are one point.  Returns (mesh, vertex_map [V_in] i32, face_map
    [F_in] i32 with -1 for a dropped face, report {vertices_in, vertices_out, degenerate_dropped, duplicates_dropped});
    with `vertex_colors` [V_in, 3] given, the colours of the kept vertices follow the mesh.

    tol = 0: two vertices are one iff their float32 coordinates have equal bits after -0.0 -> +0.0; a NaN vertex merges
    with nothing.  tol > 0: two vertices fall into one cluster iff a chain of vertices links them whose consecutive
    members are within `tol` (a transitive closure: Open3D's `merge_close_vertices`), with float64 distances
    ((dx dx + dy dy) + dz dz <= tol tol).  The device sorts the vertices by their cell floor(p / tol) and searches the 27
    neighbouring cells of each: n vertices in one cell cost n^2 distance tests, so `tol` should be small against the
    vertex spacing; a vertex farther than 2^20 tol from the origin on an axis raises ValueError.

    The lowest vertex of a cluster stands for it and keeps its own bits: nothing is averaged, a vertex that stays does
    not move.  New indices ascend with the old index of the representative.  Faces are remapped; `drop_degenerate`
    removes those that then name a vertex twice, `drop_duplicates` those whose set of vertices equals a lower face's
    (whatever its winding); the rest keep their order, winding and per-corner UVs.  Vertices no face names stay
    (`mesh_clean.remove_unreferenced_vertices` removes them).  One blocking read."""
    tol = float(tol)
    if not (tol >= 0.0 and tol < float("inf")):
        raise ValueError(f"weld_vertices: tol must be a finite number >= 0, got {tol}")
    V, F = _check_weld(mesh, "weld_vertices")
    nv, nf = int(V.shape[0]), int(F.shape[0])
    dev = V.device
    colors = None
    if vertex_colors is not None:
        colors = torch.as_tensor(vertex_colors, device=dev).to(torch.float32)
        if tuple(colors.shape) != (nv, 3):
            raise ValueError(f"vertex_colors must be [{nv}, 3], got {tuple(colors.shape)}")
    if nf == 0 or nv == 0:
        raise ValueError("weld_vertices: the mesh has no faces")
    ws = torch.empty(_lib.workspace_bytes("vsa_mesh_weld_workspace_bytes", nv, nf), dtype=torch.uint8, device=dev)
    out_v = torch.empty(nv, 3, device=dev)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    vmap = torch.empty(nv, dtype=torch.int32, device=dev)
    fmap = torch.empty(nf, dtype=torch.int32, device=dev)
    stats = (ctypes.c_longlong * 4)()
    ms = _lib.stage_array(WELD_STAGES, stage_ms)
    rc = _status("vsa_mesh_weld", V, nv, F, nf, tol, bool(drop_degenerate), bool(drop_duplicates), ws, ws.numel(),
                 out_v, out_f, vmap, fmap, ctypes.cast(stats, ctypes.c_void_p), _stage_ptr(ms), _lib.stream_ptr())
    if rc == UNSUPPORTED:
        raise ValueError(f"weld_vertices: tol = {tol} is too small for this mesh: a vertex lies more than 2^20 tol from "
                         "the origin on an axis (or the mesh is too large for a mesh stage)")
    _lib.stage_update(WELD_STAGES, stage_ms, ms)
    vout, fout, degenerate, duplicates = (int(x) for x in stats)
    v, f = out_v[:vout].clone(), out_f[:fout].clone()
    out = _rebuild(mesh, v, f, fmap)
    report = {"vertices_in": nv, "vertices_out": vout, "degenerate_dropped": degenerate,
              "duplicates_dropped": duplicates}
    if colors is None:
        return out, vmap, fmap, report
    # the representative of new vertex k is the lowest old vertex mapped to k
    first = torch.full((vout,), nv, dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, vmap.long(), torch.arange(nv, device=dev), "amin")
    return out, colors.index_select(0, first), vmap, fmap, report


@torch.no_grad()
def orient_faces(mesh, outward=True, stage_ms=None):
    """Wind every edge-connected component of a cuda TensorMesh consistently, its normals outward.  Returns (mesh,
    flipped [F] bool, component [F] i32 = the lowest face of the face's component, report {components, flipped,
    unorientable_components, undecided_components, undecided_faces}).

    Two faces are tied by an undirected edge that exactly two faces of positive area name (`edge_census`' live faces
    and manifold edges; non-manifold edges and faces without area tie nothing).  A union-find over the double cover
    (face kept / face flipped) gives every face its flip relative to the lowest face of its component, independent of
    the order of the work; a component in which a face is tied to its own mirror image (a Moebius band) is not
    orientable, stays as it is and is counted.

    Outward, per orientable component, from float64 sums of a fixed order: with N_f = 1/2 (v1 - v0) x (v2 - v0) after
    the relative flip, A_f = |N_f|, c_f the face centroid and cbar the area-weighted centroid of the component,
    S = sum N_f . (c_f - cbar) is three times the signed volume of a closed component and positive for an open sheet
    whose normals point away from its centroid; U = sum A_f (|c_f|_1 + |cbar|_1) scales its rounding error.  A
    component is decided iff |S| > 2^-20 U; a decided one with S < 0 (`outward=False`: S > 0) is flipped whole.  An
    undecided one (a single face, a flat sheet) keeps its relative orientation.

    A flipped face has its corners 1 and 2 swapped, and so have its UVs: flipping twice restores the bits.  Components
    are judged one by one: the inner wall of a solid with a cavity is wound outward too (its normals then point into
    the solid), and nothing looks at which component encloses which.  One blocking read."""
    V, F = check_mesh(mesh, "orient_faces")
    nv, nf = int(V.shape[0]), int(F.shape[0])
    dev = V.device
    if nf == 0 or nv == 0:
        raise ValueError("orient_faces: the mesh has no faces")
    uv = _uvs(mesh)
    uv_in = uv.to(torch.float32).reshape(nf, 3, 2).contiguous() if uv is not None else None
    uv_out = torch.empty_like(uv_in) if uv_in is not None else None
    ws = torch.empty(_lib.workspace_bytes("vsa_mesh_orient_workspace_bytes", nv, nf), dtype=torch.uint8, device=dev)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    flipped = torch.empty(nf, dtype=torch.uint8, device=dev)
    component = torch.empty(nf, dtype=torch.int32, device=dev)
    stats = (ctypes.c_longlong * 5)()
    ms = _lib.stage_array(ORIENT_STAGES, stage_ms)
    _lib.call("vsa_mesh_orient", V, nv, F, nf, bool(outward), uv_in, ws, ws.numel(), out_f, uv_out, flipped, component,
              ctypes.cast(stats, ctypes.c_void_p), _stage_ptr(ms), _lib.stream_ptr())
    _lib.stage_update(ORIENT_STAGES, stage_ms, ms)
    if uv_out is None:
        out = _uvless(V.clone(), out_f)
    else:
        out = TensorMesh(V.clone(), out_f, uv_out, device=dev)
        out.has_uvs = True
    names = ("components", "flipped", "unorientable_components", "undecided_components", "undecided_faces")
    return out, flipped.bool(), component, {k: int(x) for k, x in zip(names, stats)}


@torch.no_grad()
def repair_mesh(mesh, tol=0.0, weld=True, orient=True, outward=True):
    """`weld_vertices(mesh, tol)` then `orient_faces(mesh, outward)` (either can be switched off).  Returns (mesh,
    report): the two reports joined, plus `census_before` and `census_after` from `mesh_winding.edge_census`."""
    from .mesh_winding import edge_census
    report = {"census_before": edge_census(mesh)}
    if weld:
        mesh, _, _, r = weld_vertices(mesh, tol)
        report.update(r)
    if orient:
        mesh, _, _, r = orient_faces(mesh, outward)
        report.update(r)
    report["census_after"] = edge_census(mesh)
    return mesh, report


def repair_meshes(meshes_dir, out_dir, tol=0.0, weld=True, orient=True, outward=True, device="cuda"):
    """Every `<level>.ply` / `<level>.obj` of `meshes_dir` through `repair_mesh`, written as `<level>.ply` into `out_dir`
    (a `meshes_repaired/` next to `meshes/`, as `mesh_clean.clean_meshes` writes `meshes_cleaned/`), with its texcoords
    when the file had them.  Returns (paths, reports), inner to outer."""
    names = level_files(meshes_dir, obj=True)
    os.makedirs(out_dir, exist_ok=True)
    paths, reports = [], []
    for n in names:
        m, report = repair_mesh(load_mesh(os.path.join(meshes_dir, n), device=device), tol, weld, orient, outward)
        if m.faces.shape[0] == 0:
            raise ValueError(f"{n}: no faces left to save")
        path = os.path.join(out_dir, n[:-4] + ".ply")
        save_ply(path, TensorMesh(m.vertices, m.faces, _uvs(m), device=m.vertices.device))
        paths.append(path)
        reports.append(report)
    return paths, reports


__all__ = ["weld_vertices", "orient_faces", "repair_mesh", "repair_meshes", "WELD_STAGES", "ORIENT_STAGES"]
