"""Floater removal on the device: `post_process_mesh` of the reference (volsurfs_py/utils/mesh_extraction.py:18-46, the
commented-out copy at utils/mesh_from_depth.py:449-464, the baker's `meshes_cleaned/` directory, baker.py:254-270) with
Open3D's connected-triangle clustering and removals in HIP (csrc/mesh_clean.hip, rules in include/volsurfs_hip.h "Mesh
cleaning" and DESIGN §25).  Open3D is absent: the rule is restated (tests/mesh_clean_restated.py) and unpinned.

* `cluster_connected_triangles` — triangle_clusters [F] i32, cluster_n_triangles [C] i32, cluster_area [C] f64.
* `remove_triangles_by_mask`, `remove_unreferenced_vertices`, `remove_degenerate_triangles` — Open3D's meanings.
* `post_process_mesh` — the clusters with fewer faces than the `cluster_to_keep`-th largest (at least
  `min_cluster_faces`) removed, then the two other removals; per-corner UVs and vertex colours carried along.
* `clean_meshes` — every `<level>.ply` of a directory cleaned into another (the reference's `meshes_cleaned/`).
"""
import ctypes
import os

import torch

from . import _lib
from .isosurface import _uvless
from .mesh import TensorMesh, check_mesh, level_files, load_ply, save_ply

STAGES = ("edges", "sort", "hook", "roots", "number", "areas", "threshold", "mask", "compact")
MODE_ALL, MODE_MASK, MODE_CLUSTERS = 0, 1, 2


def workspace_bytes(nr_verts, nr_faces):
    """Device workspace of one clustering or one filter of a mesh with `nr_verts` vertices and `nr_faces` faces."""
    return _lib.workspace_bytes("vsa_mesh_clusters_workspace_bytes", int(nr_verts), int(nr_faces))


@torch.no_grad()
def cluster_connected_triangles(mesh, stage_ms=None):
    """Open3D's `cluster_connected_triangles` of a cuda TensorMesh: two faces are adjacent when they share an
    undirected edge (the same pair of vertex indices); a cluster is a connected component, numbered in ascending order
    of its smallest face.  Returns (triangle_clusters [F] i32, cluster_n_triangles [C] i32, cluster_area [C] f64) on
    the device.  `stage_ms` (a dict) receives the device ms per stage."""
    V, F = check_mesh(mesh, "cluster_connected_triangles")
    nv, nf = int(V.shape[0]), int(F.shape[0])
    dev = V.device
    if nf == 0:
        return (torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.float64, device=dev))
    ws = torch.empty(workspace_bytes(nv, nf), dtype=torch.uint8, device=dev)
    clusters = torch.empty(nf, dtype=torch.int32, device=dev)
    counts = torch.empty(nf, dtype=torch.int32, device=dev)
    areas = torch.empty(nf, dtype=torch.float64, device=dev)
    C = ctypes.c_longlong(0)
    ms = _lib.stage_array(STAGES, stage_ms)
    _lib.call("vsa_mesh_clusters", V, nv, F, nf, ws, ws.numel(), clusters, counts, areas,
              ctypes.cast(ctypes.pointer(C), ctypes.c_void_p),
              ctypes.cast(ms, ctypes.c_void_p) if ms is not None else None, _lib.stream_ptr())
    _lib.stage_update(STAGES, stage_ms, ms)
    return clusters, counts[:C.value].clone(), areas[:C.value].clone()


@torch.no_grad()
def _filter(V, F, mode, keep_mask=None, cluster_to_keep=1, min_cluster_faces=0, drop_unreferenced=False,
            drop_degenerate=False, stage_ms=None):
    """The C-ABI call: (vertices, faces, vertex_map [V], face_map [F], stats dict)."""
    nv, nf = int(V.shape[0]), int(F.shape[0])
    dev = V.device
    ws = torch.empty(workspace_bytes(nv, nf), dtype=torch.uint8, device=dev)
    out_v = torch.empty(nv, 3, device=dev)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    vmap = torch.empty(nv, dtype=torch.int32, device=dev)
    fmap = torch.empty(nf, dtype=torch.int32, device=dev)
    stats = (ctypes.c_longlong * 6)()
    ms = _lib.stage_array(STAGES, stage_ms)
    _lib.call("vsa_mesh_filter", V, nv, F, nf, int(mode), keep_mask, int(cluster_to_keep), int(min_cluster_faces),
              bool(drop_unreferenced), bool(drop_degenerate), ws, ws.numel(), out_v, out_f, vmap, fmap,
              ctypes.cast(stats, ctypes.c_void_p), ctypes.cast(ms, ctypes.c_void_p) if ms is not None else None,
              _lib.stream_ptr())
    _lib.stage_update(STAGES, stage_ms, ms)
    vout, fout, C, thr, kept, passed = (int(x) for x in stats)
    st = {"clusters": C, "threshold": thr, "clusters_kept": kept, "faces_in": nf, "faces_out": fout,
          "vertices_in": nv, "vertices_out": vout, "faces_passed": passed}
    return out_v[:vout].clone(), out_f[:fout].clone(), vmap, fmap, st


@torch.no_grad()
def compact_rows(rows, index_map, nr_out):
    """out[index_map[i]] = rows[i] for index_map[i] >= 0: a per-vertex or per-corner attribute ([N, ...], 32-bit
    elements) through a map of the filter, on the device.  Returns [nr_out, ...]."""
    if rows.element_size() != 4:
        raise _lib.VolsurfsHipError(f"compact_rows: 32-bit elements expected, got {rows.dtype}")
    rows = rows.contiguous()
    n = int(rows.shape[0])
    if int(index_map.shape[0]) != n:
        raise ValueError(f"compact_rows: {n} rows for a map of {int(index_map.shape[0])}")
    words = 1
    for s in rows.shape[1:]:
        words *= int(s)
    out = torch.empty((int(nr_out),) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    if n and words and int(nr_out):                    # (an empty output has no address to hand over)
        _lib.call("vsa_mesh_compact_rows", rows, n, words, index_map, out, _lib.stream_ptr())
    return out


def _uvs(mesh):
    """The mesh's per-corner UVs when it carries real ones (`has_uvs` not False), else None."""
    uv = mesh.get_faces_uvs()
    return uv if uv is not None and getattr(mesh, "has_uvs", True) else None


def _rebuild(mesh, v, f, fmap):
    """A TensorMesh of (v, f) with the source mesh's UVs carried through the face map."""
    uv = _uvs(mesh)
    if uv is None:
        return _uvless(v, f)
    out = TensorMesh(v, f, compact_rows(uv.to(torch.float32).reshape(-1, 6), fmap, f.shape[0]).reshape(-1, 3, 2),
                     device=v.device)
    out.has_uvs = True
    return out


def _unchanged(mesh, V, F):
    return _rebuild(mesh, V.clone(), F.clone(), torch.arange(F.shape[0], dtype=torch.int32, device=F.device))


def remove_triangles_by_mask(mesh, mask):
    """Open3D's `remove_triangles_by_mask`: the faces with mask[f] True are removed, the others keep their order;
    the vertices stay as they are.  `mask` [F] bool."""
    V, F = check_mesh(mesh, "remove_triangles_by_mask")
    mask = torch.as_tensor(mask, device=F.device).reshape(-1)
    if mask.shape[0] != F.shape[0]:
        raise ValueError(f"remove_triangles_by_mask: a mask of {mask.shape[0]} for {F.shape[0]} faces")
    if F.shape[0] == 0 or V.shape[0] == 0:
        return _unchanged(mesh, V, F)
    keep = (~mask.to(torch.bool)).to(torch.uint8).contiguous()
    v, f, _, fmap, _ = _filter(V, F, MODE_MASK, keep_mask=keep)
    return _rebuild(mesh, v, f, fmap)


def remove_unreferenced_vertices(mesh):
    """Open3D's `remove_unreferenced_vertices`: the vertices a face names, in their order and with their bits; the
    faces renumbered."""
    V, F = check_mesh(mesh, "remove_unreferenced_vertices")
    if F.shape[0] == 0 or V.shape[0] == 0:
        return _rebuild(mesh, V[:0].clone(), F.clone(), torch.zeros(0, dtype=torch.int32, device=F.device))
    v, f, _, fmap, _ = _filter(V, F, MODE_ALL, drop_unreferenced=True)
    return _rebuild(mesh, v, f, fmap)


def remove_degenerate_triangles(mesh):
    """Open3D's `remove_degenerate_triangles`: the faces that name a vertex twice are removed, the others keep their
    order; the vertices stay as they are."""
    V, F = check_mesh(mesh, "remove_degenerate_triangles")
    if F.shape[0] == 0 or V.shape[0] == 0:
        return _unchanged(mesh, V, F)
    v, f, _, fmap, _ = _filter(V, F, MODE_ALL, drop_degenerate=True)
    return _rebuild(mesh, v, f, fmap)


def post_process_mesh(mesh, cluster_to_keep=1000, min_cluster_faces=50, vertex_colors=None, return_stats=False,
                      stage_ms=None):
    """The reference's `post_process_mesh(mesh, cluster_to_keep=1000)` (mesh_extraction.py:18-46) on a cuda TensorMesh:
    n = max(the cluster_to_keep-th largest cluster's face count, min_cluster_faces); every face whose cluster has fewer
    than n faces is removed (a strict <: clusters tied at n all stay); then `remove_unreferenced_vertices` and
    `remove_degenerate_triangles`, in that order, so a vertex named only by a degenerate face stays.

    One departure, on purpose: with fewer than `cluster_to_keep` clusters the reference's
    `np.sort(cluster_n_triangles.copy())[-cluster_to_keep]` raises IndexError (with its default of 1000, on almost
    every mesh); here k = min(cluster_to_keep, C), so the floor of `min_cluster_faces` decides.  cluster_to_keep < 1
    raises ValueError.  An empty mesh comes back empty.

    Returns a TensorMesh; the mesh's `faces_uvs` (when it has them) follow the faces.  With `vertex_colors` [V, 3]
    given, (mesh, colours of the kept vertices).  With `return_stats`, a last element {clusters, threshold,
    clusters_kept, faces_in, faces_out, vertices_in, vertices_out, faces_passed}."""
    if int(cluster_to_keep) < 1:
        raise ValueError(f"cluster_to_keep must be at least 1, got {cluster_to_keep}")
    if int(min_cluster_faces) < 0:
        raise ValueError(f"min_cluster_faces must not be negative, got {min_cluster_faces}")
    V, F = check_mesh(mesh, "post_process_mesh")
    colors = None
    if vertex_colors is not None:
        colors = torch.as_tensor(vertex_colors, device=V.device).to(torch.float32)
        if tuple(colors.shape) != (V.shape[0], 3):
            raise ValueError(f"vertex_colors must be [{V.shape[0]}, 3], got {tuple(colors.shape)}")
    if F.shape[0] == 0:
        fmap = torch.zeros(0, dtype=torch.int32, device=V.device)
        out = _rebuild(mesh, V[:0].clone(), F.clone(), fmap)
        st = {"clusters": 0, "threshold": 0, "clusters_kept": 0, "faces_in": 0, "faces_out": 0,
              "vertices_in": int(V.shape[0]), "vertices_out": 0, "faces_passed": 0}
        colors = None if colors is None else colors[:0].clone()
    else:
        v, f, vmap, fmap, st = _filter(V, F, MODE_CLUSTERS, cluster_to_keep=cluster_to_keep,
                                       min_cluster_faces=min_cluster_faces, drop_unreferenced=True,
                                       drop_degenerate=True, stage_ms=stage_ms)
        out = _rebuild(mesh, v, f, fmap)
        if colors is not None:
            colors = compact_rows(colors, vmap, v.shape[0])
    res = (out,) + ((colors,) if vertex_colors is not None else ()) + ((st,) if return_stats else ())
    return res[0] if len(res) == 1 else res


def clean_meshes(meshes_dir, out_dir, cluster_to_keep=1000, min_cluster_faces=50, device="cuda"):
    """The baker's `meshes_cleaned/` stage (baker.py:254-270, between `meshes/` and `meshes_simplified/`): every
    `<level>.ply` of `meshes_dir` through `post_process_mesh`, written under the same name into `out_dir`, with its
    texcoords when the file had them.  Returns the paths, inner to outer; `simplify.simplify_meshes` and
    `mesh.load_meshes_indexed_from_path` take `out_dir` as they take `meshes/`."""
    names = level_files(meshes_dir)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for n in names:
        m = post_process_mesh(load_ply(os.path.join(meshes_dir, n), device=device), cluster_to_keep, min_cluster_faces)
        if m.faces.shape[0] == 0:
            raise ValueError(f"{n}: no faces left to save")
        path = os.path.join(out_dir, n)
        save_ply(path, TensorMesh(m.vertices, m.faces, _uvs(m), device=m.vertices.device))
        paths.append(path)
    return paths


__all__ = ["cluster_connected_triangles", "remove_triangles_by_mask", "remove_unreferenced_vertices",
           "remove_degenerate_triangles", "post_process_mesh", "clean_meshes", "compact_rows", "workspace_bytes",
           "STAGES"]
