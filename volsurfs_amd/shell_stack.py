"""What the stages that work on a stack of nested shells share (`simplify.simplify_shells`, `shell_untangle`,
`mesh_smooth`; `mesh_intersect.check_shells` for the self count): the order in which a stack is taken, the guard meshes
of one shell and their block of C-ABI arguments (csrc/cross_walk.h: CrossGuards), the reports, and a `meshes*/`
directory read and written in its own formats.  It is built on `mesh_intersect`'s passes and holds no rule of its own:
the rules are the stages' (include/volsurfs_hip.h).
"""
import ctypes
import os

import torch

from .mesh import TensorMesh, load_obj, load_ply, save_obj, save_ply
from .mesh_distance import _resolve
from .mesh_intersect import cross_passes, leaf_order, shell_crossings, shells_nested, tree_of
from .raytrace import RayTracer

MAX_GUARDS = 4


def stack_order(K, anchor):
    """[(shell, guards)] in the order a stack of K shells is taken: the anchor against its two input neighbours, then
    outward, then inward; guards as ("in", k) = input shell k or ("out", k) = the already finished shell k, lower shell
    first."""
    order = [(anchor, [("in", k) for k in (anchor - 1, anchor + 1) if 0 <= k < K])]
    for k in range(anchor + 1, K):
        order.append((k, [("out", k - 1)] + ([("in", k + 1)] if k + 1 < K else [])))
    for k in range(anchor - 1, -1, -1):
        order.append((k, ([("in", k - 1)] if k - 1 >= 0 else []) + [("out", k + 1)]))
    return order


def check_stack(meshes, anchor, builder, what):
    """(meshes, K, anchor) of a stage's stack: K >= 2 cuda TensorMeshes (as a list) or a RayTracer over them (as it
    is), the anchor K // 2 by default; `builder` None where the stage builds no tree of its own.  Raises ValueError
    before any HIP call."""
    is_tracer = isinstance(meshes, RayTracer)
    if not is_tracer:
        meshes = list(meshes)
    K = meshes.nr_meshes if is_tracer else len(meshes)
    if K < 2:
        raise ValueError(f"{what}: at least 2 shells, got {K}")
    anchor = K // 2 if anchor is None else int(anchor)
    if not 0 <= anchor < K:
        raise ValueError(f"{what}: anchor {anchor} outside 0..{K - 1}")
    if builder is not None and builder not in RayTracer.BUILDERS:
        raise ValueError(f"builder must be one of {RayTracer.BUILDERS}, got {builder!r}")
    for k, m in enumerate(() if is_tracer else meshes):
        if not (m.vertices.is_cuda and m.faces.is_cuda):
            raise ValueError(f"{what}: shell {k} must be on cuda, got {m.vertices.device}")
    return meshes, K, anchor


def resolve_guards(guards, what):
    """[(tracer, mesh_id)] of `guards`: a cuda TensorMesh gets a RayTracer(builder="device") of its own.  Raises
    before any HIP call for a wrong count, a wrong type, a mesh off the device or without faces."""
    guards = list(guards)
    if not 1 <= len(guards) <= MAX_GUARDS:
        raise ValueError(f"{what}: 1..{MAX_GUARDS} guards, got {len(guards)}")
    for g in guards:
        if isinstance(g, TensorMesh):
            if not (g.vertices.is_cuda and g.faces.is_cuda):
                raise ValueError(f"{what}: a guard must be on cuda, got {g.vertices.device}")
            if g.vertices.shape[0] < 1 or g.faces.shape[0] < 1:
                raise ValueError(f"{what}: a guard has no faces")
        elif not (isinstance(g, (tuple, list)) and len(g) == 2 and isinstance(g[0], RayTracer)):
            raise TypeError(f"{what}: a guard is a TensorMesh or (RayTracer, mesh_id), got {type(g).__name__}")
    return [_resolve(g, what) for g in guards]


def guard_block(resolved, what):
    """(args, keepalive): the ten guard arguments of vsa_simplify_guarded and vsa_mesh_smooth_guard (nr_guards, then the
    nine arrays) for the resolved guards [(tracer, mesh_id)], and the trees whose arrays they point into: keep
    `keepalive` until the last launch."""
    G = len(resolved)
    trees = [tree_of(g, what) for g in resolved]                  # (tracer, mesh_id, vertices, faces)
    ptrs = lambda ts: (ctypes.c_void_p * G)(*[t.data_ptr() for t in ts])
    frames = (ctypes.c_float * (6 * G))()
    for i, (tracer, mesh_id, _, _) in enumerate(trees):
        frame = ctypes.cast(tracer.q16_tree_args(mesh_id)[3], ctypes.POINTER(ctypes.c_float))
        frames[6 * i:6 * i + 6] = frame[0:6]
    args = (G, ptrs([t[0].qnodes for t in trees]), ptrs([t[0].tris for t in trees]),
            (ctypes.c_int32 * G)(*[t[0].roots[t[1]] for t in trees]), frames,
            (ctypes.c_int32 * G)(*[t[0].max_depth for t in trees]),
            ptrs([t[2] for t in trees]), (ctypes.c_longlong * G)(*[t[2].shape[0] for t in trees]),
            ptrs([t[3] for t in trees]), (ctypes.c_longlong * G)(*[t[3].shape[0] for t in trees]))
    return args, trees


def self_crossing_count(tracer, mesh_id):
    """[1] i64 on the device: the crossing pairs i < j of tracer's shell `mesh_id` (the self count pass; no read)."""
    tree = tree_of((tracer, mesh_id), "self_crossing_count")
    return cross_passes(tree, (tree[2], tree[3], leaf_order(tracer, mesh_id)), True, False, False)[4]


def with_vertices(mesh, vertices):
    """A new TensorMesh with these vertices and the mesh's faces, UVs and (where it carries them) `has_uvs` and
    `vertex_colors`."""
    new = TensorMesh(vertices, mesh.faces, mesh.faces_uvs, device=vertices.device)
    for name in ("has_uvs", "vertex_colors"):
        if hasattr(mesh, name):
            setattr(new, name, getattr(mesh, name))
    return new


def displacement(v, v0):
    """(changed [V] bool, disp [V] f64) of the vertices v against v0: whose bits differ, and how far those moved (fp64
    of the fp32 coordinates, 0 for the others).  No read."""
    changed = (v.view(torch.int32) != v0.view(torch.int32)).any(1)
    d = v.double() - v0.double()
    disp = torch.where(changed, ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sqrt(),
                       torch.zeros((), dtype=torch.float64, device=v.device))
    return changed, disp


class StackReports(list):
    """The K per-shell reports of a stage, inner to outer, with the stack's own figures: crossings_in / crossings_out =
    the crossing face pairs of every consecutive pair (k, k + 1) of the inputs / of the outputs
    (`mesh_intersect.shell_crossings`, count passes), nested = `mesh_intersect.shells_nested` of the outputs."""
    crossings_in = crossings_out = nested = None

    def fill(self, inputs, outputs, sign="pseudonormal"):
        """Sets the stack's figures from the inputs and the outputs (lists of meshes or RayTracers); returns self."""
        self.crossings_in = [c["pairs"] for c in shell_crossings(inputs)]
        self.crossings_out = [c["pairs"] for c in shell_crossings(outputs)]
        self.nested = shells_nested(outputs, sign=sign)
        return self


def _ply_is_binary(path):
    with open(path, "rb") as f:
        f.readline()
        return not f.readline().split()[1:2] == [b"ascii"]


def load_shell_dir(meshes_dir):
    """(names, meshes, vertex colours or None) of a `meshes*/` directory (`<level>.ply` / `.obj`), sorted by level as
    `VolSurfs.from_meshes_path` sorts them."""
    names = [n for n in os.listdir(meshes_dir) if n.endswith(".obj") or n.endswith(".ply")]
    names.sort(key=lambda x: float(x[:-4]))
    if not names:
        raise FileNotFoundError(f"no meshes found in {meshes_dir}")
    meshes, colors = [], []
    for n in names:
        path = os.path.join(meshes_dir, n)
        if n.endswith(".ply"):
            m, c = load_ply(path, return_colors=True)
        else:
            m, c = load_obj(path), None
        meshes.append(m)
        colors.append(c)
    return names, meshes, colors


def save_shell_dir(meshes_dir, out_dir, names, out, colors):
    """The meshes `out` into `out_dir` under the names and in the formats of `meshes_dir`: an OBJ keeps its per-corner
    UVs, a PLY its wedge UVs, its vertex colours and its ascii / binary form."""
    os.makedirs(out_dir, exist_ok=True)
    for n, m, c in zip(names, out, colors):
        src, dst = os.path.join(meshes_dir, n), os.path.join(out_dir, n)
        if n.endswith(".obj"):
            save_obj(dst, m)
        else:
            uvs = m.faces_uvs if getattr(m, "has_uvs", True) else None
            save_ply(dst, TensorMesh(m.vertices, m.faces, uvs, device=m.vertices.device), binary=_ply_is_binary(src),
                     vertex_colors=c)


__all__ = ["MAX_GUARDS", "stack_order", "check_stack", "resolve_guards", "guard_block", "self_crossing_count",
           "with_vertices", "displacement", "StackReports", "load_shell_dir", "save_shell_dir"]
