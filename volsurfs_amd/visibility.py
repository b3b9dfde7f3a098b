"""Faces no training view can see, removed on the device: the baker's `--remove_invisible_faces` ("Set to remove faces
not visible from any training view", volsurfs_py/baker.py:140-144), which the reference leaves a commented-out stub.
There is no reference behaviour to follow: the rule is this library's own (include/volsurfs_hip.h "Face visibility",
DESIGN §26), restated and unpinned, and is tested against the library's ray generation, its traversal and the
brute-force oracle.

* `face_view_counts` — per shell, how many samples of how many views had each face as the shell's closest hit: one
  fused launch (csrc/face_visibility.hip) that makes the rays in registers, walks the q16 nodes and counts, with no
  ray or hit record in memory.
* `visible_face_mask` — `counts >= min_hits`, grown by vertex rings.
* `remove_invisible_faces` — the shells without the other faces, through the mask filter of `mesh_clean` (faces keep
  their order, unreferenced vertices go, per-corner UVs and vertex colours follow).
* `cull_meshes` — the stage: every `.ply` / `.obj` of a directory into another (`meshes_visible/`), between
  `mesh_clean.clean_meshes` and `simplify.simplify_meshes`.
"""
import ctypes
import os

import torch

from . import _lib
from . import mesh_clean
from .mesh import TensorMesh, check_mesh, load_mesh, save_obj, save_ply
from .raytrace import RayTracer

TILES = ("8x8", "row")


def set_tile(tile):
    """Process-wide tile shape of the counting launch: "8x8" (default; a wave owns 8 x 8 neighbouring samples) or "row"
    (64 consecutive samples of a row).  The counts do not depend on it; tools/visibility_bench.py measures both."""
    if tile not in TILES:
        raise ValueError(f"unknown tile {tile!r} (expected one of {TILES})")
    _lib.call("vsa_face_view_counts_tile", TILES.index(tile))


def _stack_cameras(cameras, device):
    cameras = list(cameras)
    if not cameras:
        raise ValueError("face_view_counts needs at least one camera")
    H, W = cameras[0].height, cameras[0].width
    if any((c.height, c.width) != (H, W) for c in cameras):
        raise ValueError("all cameras of one call must have the same resolution")
    c2w = torch.stack([c.c2w.to(device) for c in cameras]).to(torch.float32).contiguous()
    kinv = torch.stack([c.intrinsics_inv.to(device) for c in cameras]).to(torch.float32).contiguous()
    return c2w, kinv, H, W


@torch.no_grad()
def tracer_face_view_counts(tracer, cameras, supersample=1, t_min=0.0, nr_faces=None):
    """`RayTracer.face_view_counts`: the counts of the tracer's shells, a list of K int64 [F_k] tensors.  `nr_faces`:
    the shells' face counts (default: the tracer's triangle counts)."""
    tracer.require_q16("face_view_counts")
    s = int(supersample)
    if not 1 <= s <= 8:
        raise ValueError(f"supersample must be in 1..8, got {supersample}")
    dev = tracer.device
    c2w, kinv, H, W = _stack_cameras(cameras, dev)
    V = int(c2w.shape[0])
    if V * H * W * s * s >= 1 << 32:
        raise _lib.VolsurfsHipError(f"{V} views of {H} x {W} at supersample {s}: 2^32 samples or more, a count could wrap; "
                                    "split the cameras and add the counts")
    nr_faces = [int(n) for n in (tracer.mesh_nr_tris if nr_faces is None else nr_faces)]
    if len(nr_faces) != tracer.nr_meshes:
        raise ValueError(f"{len(nr_faces)} face counts for a tracer of {tracer.nr_meshes} shells")
    base, total = [], 0
    for n in nr_faces:
        base.append(total)
        total += n
    counts = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)         # (u32 on the device)
    face_base = (ctypes.c_longlong * tracer.nr_meshes)(*base)
    _lib.call("vsa_face_view_counts", *tracer.q16_tree_args(), c2w, kinv, V, H, W, s, float(t_min), face_base, counts,
              _lib.stream_ptr())
    wide = counts.to(torch.int64) & 0xFFFFFFFF
    return [wide[b:b + n].clone() for b, n in zip(base, nr_faces)]


def face_view_counts(meshes, cameras, supersample=1, t_min=0.0, tracer=None):
    """How often each face is seen.  `meshes`: K cuda TensorMeshes; `cameras`: `camera.Camera` objects of one size.
    Sub-pixel sample (i, j) of pixel (col, row) goes through (col + (i + 0.5) / s, row + (j + 0.5) / s); each shell is
    traced on its own (the others do not occlude: they are semi-transparent layers).  Returns a list of K int64 [F_k]
    tensors on the device: the number of samples, over all views, whose closest hit (t > t_min; ties to the smallest face)
    on shell k was face f.  `tracer`: a RayTracer of these meshes with q16 nodes (default: one is built on the device)."""
    meshes = list(meshes)
    tracer = RayTracer.over(meshes if tracer is None else tracer, len(meshes))
    return tracer_face_view_counts(tracer, cameras, supersample, t_min, [int(m.faces.shape[0]) for m in meshes])


@torch.no_grad()
def visible_face_mask(mesh, counts, min_hits=1, rings=1):
    """bool [F]: `counts >= min_hits`, grown by `rings` (0..16) vertex rings (a ring adds every face that shares a
    vertex with a face of the mask).  The default ring is there because training draws jittered pixels: those rays
    land between the pixel centres counted here, on neighbours of the faces seen."""
    rings = int(rings)
    if not 0 <= rings <= 16:
        raise ValueError(f"rings must be in 0..16, got {rings}")
    V, F = check_mesh(mesh, "visible_face_mask")
    counts = torch.as_tensor(counts, device=F.device).reshape(-1)
    if counts.shape[0] != F.shape[0]:
        raise ValueError(f"visible_face_mask: {counts.shape[0]} counts for {F.shape[0]} faces")
    keep = (counts >= int(min_hits)).to(torch.uint8).contiguous()
    if rings and F.shape[0] and V.shape[0]:
        scratch = torch.empty(V.shape[0], dtype=torch.uint8, device=F.device)
        _lib.call("vsa_face_ring_dilate", F, int(F.shape[0]), int(V.shape[0]), keep, rings, scratch, _lib.stream_ptr())
    return keep.bool()


@torch.no_grad()
def remove_invisible_faces(meshes, cameras, min_hits=1, rings=1, supersample=1, vertex_colors=None, return_stats=False):
    """The shells without the faces no camera sees: `face_view_counts`, `visible_face_mask(min_hits, rings)`, then the
    mask filter of `mesh_clean` with the unreferenced vertices dropped.  Faces keep input order, the kept vertices their
    order and bits; per-corner UVs follow the faces, `vertex_colors` (a list of K [V_k, 3] tensors) the vertices.
    A shell with no visible face raises ValueError naming its index: a camera set that sees nothing is a mistake of the
    caller, not an empty asset.

    Returns the list of culled TensorMeshes; with `vertex_colors`, (meshes, colours); with `return_stats`, a last
    element: per shell {faces_in, faces_out, vertices_in, vertices_out, faces_seen (before the rings), hits}."""
    meshes, cameras = list(meshes), list(cameras)
    if vertex_colors is not None and len(vertex_colors) != len(meshes):
        raise ValueError(f"{len(vertex_colors)} colour tensors for {len(meshes)} meshes")
    counts = face_view_counts(meshes, cameras, supersample=supersample)
    out, colors_out, stats = [], [], []
    for k, (m, c) in enumerate(zip(meshes, counts)):
        V, F = check_mesh(m, "remove_invisible_faces")
        colors = None
        if vertex_colors is not None:
            colors = torch.as_tensor(vertex_colors[k], device=V.device).to(torch.float32)
            if tuple(colors.shape) != (V.shape[0], 3):
                raise ValueError(f"vertex_colors[{k}] must be [{V.shape[0]}, 3], got {tuple(colors.shape)}")
        keep = visible_face_mask(m, c, min_hits, rings)
        seen, hits = int((c >= int(min_hits)).sum()), int(c.sum())
        if not bool(keep.any()):
            raise ValueError(f"shell {k}: none of its {F.shape[0]} faces is visible from the {len(cameras)} cameras")
        v, f, vmap, fmap, st = mesh_clean._filter(V, F, mesh_clean.MODE_MASK, keep_mask=keep.to(torch.uint8).contiguous(),
                                                  drop_unreferenced=True)
        out.append(mesh_clean._rebuild(m, v, f, fmap))
        if colors is not None:
            colors_out.append(mesh_clean.compact_rows(colors, vmap, v.shape[0]))
        stats.append({"faces_in": st["faces_in"], "faces_out": st["faces_out"], "vertices_in": st["vertices_in"],
                      "vertices_out": st["vertices_out"], "faces_seen": seen, "hits": hits})
    res = (out,) + ((colors_out,) if vertex_colors is not None else ()) + ((stats,) if return_stats else ())
    return res[0] if len(res) == 1 else res


def cull_meshes(meshes_dir, cameras, out_dir, min_hits=1, rings=1, supersample=1, device="cuda"):
    """The stage (by convention `meshes_visible/`; the reference's name `meshes_cleaned/` is the floater stage here):
    every `*.ply` / `*.obj` of `meshes_dir` through `remove_invisible_faces`, all of them in one tracer and one counting
    launch, written under the same name into `out_dir` with its texcoords when the file had them.  Returns the paths in
    name order; `simplify.simplify_meshes` and `mesh.load_meshes_indexed_from_path` take `out_dir` as they take
    `meshes_cleaned/`."""
    names = sorted(n for n in os.listdir(meshes_dir) if n.endswith(".ply") or n.endswith(".obj"))
    if not names:
        raise FileNotFoundError(f"no .ply / .obj meshes in {meshes_dir}")
    meshes = [load_mesh(os.path.join(meshes_dir, n), device=device) for n in names]
    culled = remove_invisible_faces(meshes, cameras, min_hits=min_hits, rings=rings, supersample=supersample)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for n, m in zip(names, culled):
        path = os.path.join(out_dir, n)
        if n.endswith(".ply"):
            save_ply(path, TensorMesh(m.vertices, m.faces, mesh_clean._uvs(m), device=m.vertices.device))
        else:
            save_obj(path, m)
        paths.append(path)
    return paths


__all__ = ["face_view_counts", "visible_face_mask", "remove_invisible_faces", "cull_meshes", "set_tile", "TILES"]
