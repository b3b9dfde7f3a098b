"""Shell simplification on the device: the baker's `--simplify_meshes` step (volsurfs_py/baker.py:682-724,
utils/mesh_extraction.py:492-537, pymeshlab's quadric edge-collapse decimation in the reference) as parallel
Garland-Heckbert edge collapse in HIP (csrc/simplify.hip, rules in include/volsurfs_hip.h and DESIGN §15).

* `simplify_mesh` — one uv-less TensorMesh down to int(F * ratio) faces (`simplify_o3d_mesh`'s counterpart, same
  default ratio); output order and bits depend on the input mesh and the ratio only.
* `simplify_meshes` — every `<level>.ply` of a directory (what `isosurface.save_level_sets` writes) simplified into
  `out_dir` under the same names (the reference's `meshes_simplified/`).

Shells simplified one by one stop being shells: each surface moves by its own error and consecutive ones cross.  The
guarded path (no counterpart in the reference; the `guard` rule of include/volsurfs_hip.h, DESIGN §36, restated in
tests/simplify_guarded_restated.py) refuses every collapse that would create a face crossing a guard mesh:

* `simplify_mesh(.., guards=[...])` — one mesh against up to four guard meshes.
* `simplify_shells` — a stack, every shell guarded by its two neighbours: no consecutive pair of outputs has a
  crossing pair of faces that its inputs did not have.
* `simplify_meshes_nested` — that on a directory.  The pipeline order is `clean_meshes` -> `cull_meshes` ->
  `simplify_meshes_nested` -> (`untangle_meshes` for what remains) -> `compute_meshes_atlas`.
"""
import collections
import ctypes
import os

import torch

from . import _lib
from .isosurface import _uvless
from .mesh import TensorMesh, check_mesh, level_files, load_ply, save_ply
from .mesh_intersect import check_shells
from .raytrace import RayTracer
from .shell_stack import (StackReports, check_stack, guard_block, resolve_guards, self_crossing_count,
                          stack_order)

STAGES = ("init", "edges", "cost", "select", "collapse", "compact")
GUARDED_STAGES = ("init", "edges", "cost", "guard", "select", "collapse", "compact")

ShellSimplifyReport = collections.namedtuple(
    "ShellSimplifyReport", "shell guards faces_in faces_out target rounds collapses stalled guard_rejected "
                           "self_crossings")
ShellSimplifyReport.__doc__ = """One shell of `simplify_shells`: shell = its index, guards = the meshes it was guarded by,
lower shell first, as ("in", k) = input shell k or ("out", k) = the already simplified shell k; faces_in, faces_out,
target, rounds, collapses, stalled as `simplify_mesh`'s stats; guard_rejected = the (round, edge) verdicts the guard
turned down; self_crossings = the crossing pairs i < j of the output's own faces."""


class ShellSimplifyReports(StackReports):
    """The K `ShellSimplifyReport`s of `simplify_shells`, inner to outer, with the stack's own figures: crossings_in /
    crossings_out = the crossing face pairs of every consecutive pair (k, k + 1) of the inputs / of the outputs
    (`mesh_intersect.shell_crossings`, count passes), nested = `mesh_intersect.shells_nested` of the outputs."""


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


@torch.no_grad()
def _simplify_guarded(V, F, target, block, stage_ms=None):
    """vsa_simplify_guarded against the guards of `block` (`shell_stack.guard_block`): (vertices, faces, stats dict)."""
    nv, nf = int(V.shape[0]), int(F.shape[0])
    guard_args, _ = block                                         # (its second entry keeps the trees alive)
    ws = torch.empty(_lib.workspace_bytes("vsa_simplify_guarded_workspace_bytes", nv, nf), dtype=torch.uint8,
                     device=V.device)
    out_v = torch.empty(nv, 3, device=V.device)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=V.device)
    stats = (ctypes.c_longlong * 6)()
    ms = _lib.stage_array(GUARDED_STAGES, stage_ms)
    _lib.call("vsa_simplify_guarded", V, nv, F, nf, int(target), *guard_args, ws, ws.numel(), out_v, out_f,
              ctypes.cast(stats, ctypes.c_void_p), ctypes.cast(ms, ctypes.c_void_p) if ms is not None else None,
              _lib.stream_ptr())
    _lib.stage_update(GUARDED_STAGES, stage_ms, ms)
    rounds, collapses, stalled, vout, fout, rejected = (int(x) for x in stats)
    st = {"rounds": rounds, "collapses": collapses, "stalled": bool(stalled), "faces_in": nf, "faces_out": fout,
          "target": int(target), "guard_rejected": rejected}
    return out_v[:vout].clone(), out_f[:fout].clone(), st


def simplify_mesh(mesh, target_nr_faces_ratio=0.1, return_stats=False, guards=None):
    """Quadric edge-collapse decimation of a cuda TensorMesh to int(F * target_nr_faces_ratio) faces
    (simplify_o3d_mesh, utils/mesh_extraction.py:492-537).  Closed 2-manifolds stay closed 2-manifolds with their
    Euler characteristic; open boundaries keep their loops.  Returns a TensorMesh without UVs (as marching_cubes
    does), and with `return_stats` also {rounds, collapses, stalled, faces_in, faces_out, target}: faces_out <= target
    unless stalled (no collapse left that keeps the mesh valid).

    guards: None or [] (the path above, untouched) or 1..4 meshes, each a cuda TensorMesh (it gets a
    RayTracer(builder="device") of its own) or a pair (RayTracer, mesh_id) of a tracer with q16 nodes: no collapse is
    made that would create a face crossing a face of a guard (vsa_simplify_guarded; the stats gain `guard_rejected`).
    Crossings the input already has with a guard stay until a collapse removes their faces; a guard that rejects
    nothing leaves the unguarded bits."""
    V, F, ratio = _check(mesh, target_nr_faces_ratio)
    resolved = resolve_guards(guards, "simplify_mesh") if guards is not None and len(guards) else None
    target = target_faces(F.shape[0], ratio)
    if F.shape[0] == 0:
        out = _uvless(torch.zeros(0, 3, device=V.device), torch.zeros(0, 3, dtype=torch.int32, device=V.device))
        st = {"rounds": 0, "collapses": 0, "stalled": False, "faces_in": 0, "faces_out": 0, "target": 0}
        if resolved:
            st["guard_rejected"] = 0
    else:
        v, f, st = (_simplify_guarded(V, F, target, guard_block(resolved, "simplify_mesh")) if resolved else
                    _simplify(V, F, target))
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


@torch.no_grad()
def simplify_shells(meshes, target_nr_faces_ratio=0.025, anchor=None, builder="device", sign="pseudonormal"):
    """(meshes, reports): the K >= 2 shells `meshes` (inner to outer, cuda TensorMeshes) each simplified to
    int(F_k * target_nr_faces_ratio) faces under the guard of its neighbours.  The anchor (default K // 2) goes first,
    guarded by the input shells anchor - 1 and anchor + 1; then outward, shell k guarded by the already simplified
    shell k - 1 and the input shell k + 1 (if there is one); then inward, mirrored.  The guards' trees are built with
    `builder`; the result does not depend on it.

    For every consecutive pair the crossing face pairs of the outputs are a subset of the pairs of surviving input
    faces: crossings_out <= crossings_in, and a stack that comes in without crossings goes out without.  Crossing
    inputs are reported, not refused.  NOT promised: that a target is reached (`stalled`, `faces_out`), that a shell
    does not cross itself (`self_crossings`), anything about shells that are not consecutive.

    `reports` is a `ShellSimplifyReports`: one `ShellSimplifyReport` per shell, and crossings_in, crossings_out and
    nested (by `sign`) of the stack.  Argument errors raise before any HIP call."""
    meshes, K, anchor = check_stack(meshes, anchor, builder, "simplify_shells")
    if sign not in RayTracer.SIGNS:
        raise ValueError(f"sign must be one of {RayTracer.SIGNS}, got {sign!r}")
    ratio = float(target_nr_faces_ratio)
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"target_nr_faces_ratio must lie in (0, 1], got {ratio}")
    for k, m in enumerate(meshes):
        if m.vertices.shape[0] < 1 or m.faces.shape[0] < 1:
            raise ValueError(f"simplify_shells: shell {k} is empty")
    inputs = RayTracer(meshes, builder=builder)
    done, out, stats = [None] * K, [None] * K, [None] * K

    def run(k, names):
        guards = [(inputs, g) if which == "in" else (done[g], 0) for which, g in names]
        out[k], stats[k] = simplify_mesh(meshes[k], ratio, return_stats=True, guards=guards)
        if out[k].faces.shape[0] < 1:
            raise ValueError(f"simplify_shells: shell {k} has no faces left")
        done[k] = RayTracer([out[k]], builder=builder)
        stats[k]["guards"] = tuple(names)

    for k, names in stack_order(K, anchor):
        run(k, names)
    selfs = torch.cat([self_crossing_count(done[k], 0) for k in range(K)]).cpu().tolist()
    reports = ShellSimplifyReports(
        ShellSimplifyReport(k, st["guards"], st["faces_in"], st["faces_out"], st["target"], st["rounds"],
                            st["collapses"], st["stalled"], st["guard_rejected"], int(selfs[k]))
        for k, st in enumerate(stats))
    return out, reports.fill(inputs, out, sign)


def simplify_meshes_nested(meshes_dir, out_dir, target_nr_faces_ratio=0.025, device="cuda"):
    """`simplify_meshes` for shells that must stay shells: every `<level>.ply` of `meshes_dir` (sorted by level, inner
    to outer) through `simplify_shells`, written under the same names into `out_dir` without texcoords.  Returns
    (paths, reports, `mesh_intersect.check_shells(out_dir)`).  It sits between `cull_meshes` and
    `compute_meshes_atlas`; `untangle_meshes` is for the crossings the input already had."""
    names = level_files(meshes_dir)
    meshes = [load_ply(os.path.join(meshes_dir, n), device=device) for n in names]
    out, reports = simplify_shells(meshes, target_nr_faces_ratio)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for n, m in zip(names, out):
        path = os.path.join(out_dir, n)
        save_ply(path, TensorMesh(m.vertices, m.faces, None, device=m.vertices.device))
        paths.append(path)
    return paths, reports, check_shells(out_dir)


__all__ = ["simplify_mesh", "simplify_meshes", "simplify_shells", "simplify_meshes_nested", "ShellSimplifyReport",
           "ShellSimplifyReports", "stack_order", "workspace_bytes", "target_faces", "STAGES", "GUARDED_STAGES"]
