"""Shell simplification on the device: the baker's `--simplify_meshes` step (volsurfs_py/baker.py:682-724,
utils/mesh_extraction.py:492-537, pymeshlab's quadric edge-collapse decimation in the reference) as parallel
Garland-Heckbert edge collapse in HIP (csrc/simplify.hip, rules in include/volsurfs_hip.h and DESIGN §15).

* `simplify_mesh` — one uv-less TensorMesh down to int(F * ratio) faces (`simplify_o3d_mesh`'s counterpart, same
  default ratio); output order and bits depend on the input mesh and the ratio only.
* `simplify_meshes` — every `<level>.ply` of a directory (what `isosurface.save_level_sets` writes) simplified into
  `out_dir` under the same names (the reference's `meshes_simplified/`).
"""
import ctypes
import os

import torch

from . import _lib
from .isosurface import _uvless
from .mesh import TensorMesh, check_mesh, level_files, load_ply, save_ply

STAGES = ("init", "edges", "cost", "select", "collapse", "compact")


def workspace_bytes(nr_verts, nr_faces):
    """Device workspace of one simplification of a mesh with `nr_verts` vertices and `nr_faces` faces."""
    return _lib.workspace_bytes("vsa_simplify_workspace_bytes", int(nr_verts), int(nr_faces))


def target_faces(nr_faces, ratio):
    """pymeshlab's targetfacenum rule: int(F * ratio)."""
    return int(int(nr_faces) * float(ratio))


def _check(mesh, ratio):
    ratio = float(ratio)
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"target_nr_faces_ratio must lie in (0, 1], got {ratio}")
    V, F = check_mesh(mesh, "simplify_mesh", refuse_degenerate=True)
    return V, F, ratio


@torch.no_grad()
def _simplify(V, F, target, stage_ms=None):
    """The C-ABI call: (vertices, faces, stats dict); `stage_ms` (a dict) receives the device ms per stage."""
    nv, nf = int(V.shape[0]), int(F.shape[0])
    ws = torch.empty(workspace_bytes(nv, nf), dtype=torch.uint8, device=V.device)
    out_v = torch.empty(nv, 3, device=V.device)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=V.device)
    stats = (ctypes.c_longlong * 5)()
    ms = _lib.stage_array(STAGES, stage_ms)
    _lib.call("vsa_simplify", V, nv, F, nf, int(target), ws, ws.numel(), out_v, out_f,
              ctypes.cast(stats, ctypes.c_void_p), ctypes.cast(ms, ctypes.c_void_p) if ms is not None else None,
              _lib.stream_ptr())
    _lib.stage_update(STAGES, stage_ms, ms)
    rounds, collapses, stalled, vout, fout = (int(x) for x in stats)
    st = {"rounds": rounds, "collapses": collapses, "stalled": bool(stalled), "faces_in": nf, "faces_out": fout,
          "target": int(target)}
    return out_v[:vout].clone(), out_f[:fout].clone(), st


def simplify_mesh(mesh, target_nr_faces_ratio=0.1, return_stats=False):
    """Quadric edge-collapse decimation of a cuda TensorMesh to int(F * target_nr_faces_ratio) faces
    (simplify_o3d_mesh, utils/mesh_extraction.py:492-537).  Closed 2-manifolds stay closed 2-manifolds with their
    Euler characteristic; open boundaries keep their loops.  Returns a TensorMesh without UVs (as marching_cubes
    does), and with `return_stats` also {rounds, collapses, stalled, faces_in, faces_out, target}: faces_out <= target
    unless stalled (no collapse left that keeps the mesh valid)."""
    V, F, ratio = _check(mesh, target_nr_faces_ratio)
    target = target_faces(F.shape[0], ratio)
    if F.shape[0] == 0:
        out = _uvless(torch.zeros(0, 3, device=V.device), torch.zeros(0, 3, dtype=torch.int32, device=V.device))
        st = {"rounds": 0, "collapses": 0, "stalled": False, "faces_in": 0, "faces_out": 0, "target": 0}
    else:
        v, f, st = _simplify(V, F, target)
        out = _uvless(v, f)
    return (out, st) if return_stats else out


def simplify_meshes(meshes_dir, out_dir, target_nr_faces_ratio=0.025, device="cuda"):
    """The baker's `--simplify_meshes` (baker.py:682-724): every `<level>.ply` of `meshes_dir` simplified on its own
    to `target_nr_faces_ratio` of its faces, written under the same name into `out_dir` (the reference's
    `meshes_simplified/`) without texcoords.  Returns the paths, inner to outer; `mesh.load_meshes_indexed_from_path`
    reads them back in that order."""
    names = level_files(meshes_dir)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for n in names:
        m = simplify_mesh(load_ply(os.path.join(meshes_dir, n), device=device), target_nr_faces_ratio)
        if m.faces.shape[0] == 0:
            raise ValueError(f"{n}: no faces left to save")
        path = os.path.join(out_dir, n)
        save_ply(path, TensorMesh(m.vertices, m.faces, None, device=m.vertices.device))
        paths.append(path)
    return paths


__all__ = ["simplify_mesh", "simplify_meshes", "workspace_bytes", "target_faces", "STAGES"]
