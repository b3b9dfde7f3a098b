"""UV atlases of extracted shells on the device: the baker's `--compute_meshes_xatlas` step (volsurfs_py/baker.py:727-776,
utils/texture_extraction.py::compute_o3d_mesh_atlas, xatlas with padding 3 in the reference) as box-projection charts
packed into one square atlas in HIP (csrc/atlas.hip, rules in include/volsurfs_hip.h and DESIGN §16), or with
`charts="merged"` as box charts merged into plane-projected groups first.

* `compute_atlas` — one uv-less, consistently wound TensorMesh (what `marching_cubes` / `simplify_mesh` return) with
  per-corner UVs; vertices and faces unchanged; output bits depend on the mesh, the resolution and the padding only.
* `rasterize_atlas` — which face covers each texel of an atlas, and how many do.
* `compute_meshes_atlas` — every `<level>.ply` of a directory (what `simplify.simplify_meshes` writes) into
  `<level>.obj` with UVs plus `atlas/<level>.png` (the reference's `meshes_simplified_uvs/`), the neural-texture
  branch's input.
"""
import ctypes
import os

import torch

from . import _lib
from .mesh import TensorMesh, check_mesh, level_files, load_ply, save_obj

STAGES = ("label", "charts", "pack", "emit", "raster")
MERGED_STAGES = STAGES + ("merge",)
CHARTS = ("box", "merged")
ERR_ATLAS_FULL = -3


def workspace_bytes(nr_verts, nr_faces, resolution):
    """Device workspace of one atlas of a mesh with `nr_verts` vertices and `nr_faces` faces at `resolution`^2."""
    return _lib.workspace_bytes("vsa_atlas_workspace_bytes", int(nr_verts), int(nr_faces), int(resolution))


def min_resolution(charts, padding):
    """Smallest resolution at which `charts` rectangles of (2 padding)^2 texels (every chart at zero size) fit on
    next-fit shelves."""
    side = 2 * int(padding)
    r = max(side, 1)
    while True:
        per = r // side if side else charts
        if per > 0 and -(-charts // per) * side <= r:
            return r
        r += 1


def full_message(charts, resolution, padding, smallest):
    return (f"compute_atlas: {charts} charts do not fit a {resolution} x {resolution} atlas with padding {padding} "
            f"even at zero size; the smallest resolution that holds them is {smallest}")


def merged_workspace_bytes(nr_verts, nr_faces, resolution):
    """Device workspace of one `charts="merged"` atlas."""
    return _lib.workspace_bytes("vsa_atlas_merged_workspace_bytes", int(nr_verts), int(nr_faces), int(resolution))


def _check_charts(charts, min_cos, merge_rounds):
    """The chart mode's arguments, checked before any device call."""
    if charts not in CHARTS:
        raise ValueError(f"compute_atlas: charts must be one of {CHARTS}, got {charts!r}")
    if charts == "box":                                # (neither is read there)
        return min_cos, merge_rounds
    min_cos, merge_rounds = float(min_cos), int(merge_rounds)
    if not 0.0 < min_cos <= 1.0:                       # (a NaN fails it)
        raise ValueError(f"compute_atlas: min_cos must lie in (0, 1], got {min_cos}")
    if merge_rounds < 0:
        raise ValueError(f"compute_atlas: merge_rounds must be >= 0, got {merge_rounds}")
    return min_cos, merge_rounds


def _check(mesh, resolution, padding):
    resolution, padding = int(resolution), int(padding)
    if not 8 <= resolution <= 16384:
        raise ValueError(f"compute_atlas: resolution must lie in [8, 16384], got {resolution}")
    if padding < 0 or 2 * padding >= resolution:
        raise ValueError(f"compute_atlas: padding must satisfy 0 <= 2 * padding < resolution, got {padding}")
    V, F = check_mesh(mesh, "compute_atlas", refuse_degenerate=True)
    return V, F, resolution, padding


@torch.no_grad()
def _atlas(V, F, R, p, stage_ms=None):
    """The C-ABI call: (faces_uvs [F, 3, 2], chart [F], stats dict)."""
    nv, nf = int(V.shape[0]), int(F.shape[0])
    ws = torch.empty(workspace_bytes(nv, nf, R), dtype=torch.uint8, device=V.device)
    uv = torch.empty(nf, 3, 2, device=V.device)
    chart = torch.empty(nf, dtype=torch.int32, device=V.device)
    stats = (ctypes.c_longlong * 4)()
    scale = ctypes.c_float(0.0)
    ms = _lib.stage_array(STAGES, stage_ms)
    rc = _lib.lib().vsa_atlas(V.data_ptr(), nv, F.data_ptr(), nf, R, p, ws.data_ptr(), ws.numel(), uv.data_ptr(),
                              chart.data_ptr(), ctypes.addressof(stats), ctypes.addressof(scale),
                              ctypes.addressof(ms) if ms is not None else None, _lib.stream_ptr().value)
    if rc == ERR_ATLAS_FULL:
        raise _lib.VolsurfsHipError(full_message(int(stats[0]), R, p, int(stats[3])))
    if rc != 0:
        raise _lib.VolsurfsHipError(f"vsa_atlas failed with status {rc}")
    _lib.stage_update(STAGES, stage_ms, ms)
    charts, splits, covered = int(stats[0]), int(stats[1]), int(stats[2])
    st = {"charts": charts, "split_rounds": splits, "scale": float(scale.value), "covered": covered,
          "utilization": covered / float(R * R), "resolution": R, "padding": p}
    return uv, chart, st


@torch.no_grad()
def _atlas_merged(V, F, R, p, min_cos, merge_rounds, stage_ms=None):
    """vsa_atlas_merged: `_atlas`'s triple, the stats with the four merge counts."""
    nv, nf = int(V.shape[0]), int(F.shape[0])
    ws = torch.empty(merged_workspace_bytes(nv, nf, R), dtype=torch.uint8, device=V.device)
    uv = torch.empty(nf, 3, 2, device=V.device)
    chart = torch.empty(nf, dtype=torch.int32, device=V.device)
    stats = (ctypes.c_longlong * 8)()
    scale = ctypes.c_float(0.0)
    ms = _lib.stage_array(MERGED_STAGES, stage_ms)
    rc = _lib.lib().vsa_atlas_merged(V.data_ptr(), nv, F.data_ptr(), nf, R, p, min_cos, merge_rounds, ws.data_ptr(),
                                     ws.numel(), uv.data_ptr(), chart.data_ptr(), ctypes.addressof(stats),
                                     ctypes.addressof(scale), ctypes.addressof(ms) if ms is not None else None,
                                     _lib.stream_ptr().value)
    if rc == ERR_ATLAS_FULL:
        raise _lib.VolsurfsHipError(full_message(int(stats[0]), R, p, int(stats[3])))
    if rc != 0:
        raise _lib.VolsurfsHipError(f"vsa_atlas_merged failed with status {rc}")
    _lib.stage_update(MERGED_STAGES, stage_ms, ms)
    covered = int(stats[2])
    st = {"charts": int(stats[0]), "split_rounds": int(stats[1]), "scale": float(scale.value), "covered": covered,
          "utilization": covered / float(R * R), "resolution": R, "padding": p, "box_charts": int(stats[4]),
          "groups": int(stats[5]), "merge_rounds": int(stats[6]), "valid_pairs_left": int(stats[7])}
    return uv, chart, st


def compute_atlas(mesh, resolution=1024, padding=4, return_stats=False, return_charts=False, stage_ms=None,
                  charts="box", min_cos=0.5, merge_rounds=64):
    """Per-corner UVs for a uv-less, consistently wound cuda TensorMesh by box projection: faces grouped
    by normal direction into connected charts, each projected along its direction (at least half of every face's area
    survives, no face flips), charts that overlap themselves split, and all packed by shelves into one
    `resolution`^2 atlas at the largest texel density the bisection finds.  Returns a TensorMesh with the same
    vertices and faces and `has_uvs = True`; with `return_stats` also {charts, split_rounds, scale (texels per unit),
    covered, utilization (covered texels / resolution^2), resolution, padding}; with `return_charts` also the chart
    number per face.

    Padding: chart contents sit `padding` texels inside their rectangles, so two charts are at least 2 * padding
    texels apart at `resolution`.  The default 4 at 1024 keeps them 2 texels apart at 256, the coarsest default
    `textures_res` of the neural textures, so a bilinear lookup (which reads a 2 x 2 texel footprint) at every level
    of the texture pyramid never mixes two charts.  The reference's xatlas call uses 3.

    `charts="merged"` first merges connected box charts into groups whose faces all lie within
    acos(`min_cos`) of the group's summed normal and projects each group along that normal, in at most `merge_rounds`
    rounds of mutual best-neighbour merges (0: the box atlas): every face keeps at least `min_cos` of its area and none
    flips.  The default 0.5 is the box rule's own bound, so it adds no stretch the atlas does not already allow; lower
    values trade up to 1 / `min_cos` of texel stretch along the tilt for fewer charts.  The stats then also hold
    {box_charts, groups, merge_rounds (rounds run), valid_pairs_left}, and `stage_ms` a sixth entry, `merge`.  A mesh
    on which nothing merges gets the bytes of `charts="box"`, which runs exactly the code it ran before the mode
    existed.  Any other `charts`, and with "merged" a `min_cos` outside (0, 1] or a negative `merge_rounds`, is a
    ValueError.

    Raises VolsurfsHipError (naming the chart count and the smallest resolution that would hold them) when the charts
    do not fit even at zero size."""
    min_cos, merge_rounds = _check_charts(charts, min_cos, merge_rounds)
    V, F, R, p = _check(mesh, resolution, padding)
    if F.shape[0] == 0:
        uv = torch.zeros(0, 3, 2, device=V.device)
        chart = torch.zeros(0, dtype=torch.int32, device=V.device)
        st = {"charts": 0, "split_rounds": 0, "scale": 0.0, "covered": 0, "utilization": 0.0, "resolution": R,
              "padding": p}
        if charts == "merged":
            st.update(box_charts=0, groups=0, merge_rounds=0, valid_pairs_left=0)
    elif charts == "merged":
        uv, chart, st = _atlas_merged(V, F, R, p, min_cos, merge_rounds, stage_ms)
    else:
        uv, chart, st = _atlas(V, F, R, p, stage_ms)
    out = TensorMesh(V, F, uv, device=V.device)
    out.has_uvs = True
    res = (out,)
    if return_stats:
        res += (st,)
    if return_charts:
        res += (chart,)
    return res[0] if len(res) == 1 else res


@torch.no_grad()
def rasterize_atlas(mesh, resolution):
    """(face_id [R, R] i32, count [R, R] i32) of a cuda mesh's faces_uvs: row j holds texel centres v = (j + 0.5) / R,
    column i u = (i + 0.5) / R; face_id is the lowest face covering the texel (-1: none), count the number of faces
    covering it (header rule: 1/256-texel snapping, top-left fill, faces of zero or negative UV area cover nothing)."""
    R = int(resolution)
    if not 8 <= R <= 16384:
        raise ValueError(f"rasterize_atlas: resolution must lie in [8, 16384], got {R}")
    uv = mesh.get_faces_uvs() if isinstance(mesh, TensorMesh) else mesh
    if uv is None or not uv.is_cuda or uv.dim() != 3 or tuple(uv.shape[1:]) != (3, 2):
        raise ValueError("rasterize_atlas: expected cuda faces_uvs [F, 3, 2]")
    uv = uv.to(torch.float32).contiguous()
    face_id = torch.full((R, R), -1, dtype=torch.int32, device=uv.device)
    count = torch.zeros((R, R), dtype=torch.int32, device=uv.device)
    nf = int(uv.shape[0])
    if nf == 0:
        return face_id, count
    if not bool(torch.isfinite(uv).all()):
        raise _lib.VolsurfsHipError("rasterize_atlas: the UVs hold NaN or inf")
    n = _lib.workspace_bytes("vsa_atlas_rasterize_workspace_bytes", nf)
    ws = torch.empty(n, dtype=torch.uint8, device=uv.device)
    _lib.call("vsa_atlas_rasterize", uv, nf, R, ws, ws.numel(), face_id, count, _lib.stream_ptr())
    return face_id, count


def chart_image(charts, face_id):
    """[R, R, 3] uint8: one colour per chart (a fixed hash of the chart number), black where no face covers the
    texel; row 0 is the top of the atlas (v = 1), as image files and OBJ texture coordinates expect."""
    c = charts.to(torch.int64)[face_id.clamp(min=0).to(torch.int64)]
    h = (c + 1) * 2654435761
    rgb = torch.stack([(h >> 8) & 255, (h >> 16) & 255, (h >> 24) & 255], -1)
    rgb = (rgb % 192 + 64).to(torch.uint8)
    rgb[face_id < 0] = 0
    return torch.flip(rgb, [0])


def compute_meshes_atlas(meshes_dir, out_dir, resolution=1024, padding=4, device="cuda", charts="box", min_cos=0.5):
    """The baker's `--compute_meshes_xatlas` (baker.py:727-776): every `<level>.ply` of `meshes_dir` (the reference's
    `meshes_simplified/`) atlased on its own and written to `out_dir` (its `meshes_simplified_uvs/`) as `<level>.obj`
    with per-corner UVs, plus `atlas/<level>.png`, one colour per chart.  Returns the .obj paths, inner to outer;
    `VolSurfs.from_meshes_path(out_dir, ..., using_neural_textures=True)` trains on them.  `charts` and `min_cos` are
    `compute_atlas`'s."""
    _check_charts(charts, min_cos, 0)
    from .evaluation import _save_png
    from .mesh import load_mesh
    names = level_files(meshes_dir, obj=True)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for n in names:
        src = os.path.join(meshes_dir, n)
        m = load_ply(src, device=device) if n.endswith(".ply") else load_mesh(src, device=device)
        if m.faces.shape[0] == 0:
            raise ValueError(f"{n}: no faces to atlas")
        out, chart_of = compute_atlas(m, resolution, padding, return_charts=True, charts=charts, min_cos=min_cos)
        stem = n[:-4]
        path = os.path.join(out_dir, stem + ".obj")
        save_obj(path, out)
        face_id, _ = rasterize_atlas(out, resolution)
        _save_png(chart_image(chart_of, face_id), os.path.join(out_dir, "atlas", stem + ".png"))
        paths.append(path)
    return paths


__all__ = ["compute_atlas", "rasterize_atlas", "compute_meshes_atlas", "chart_image", "workspace_bytes",
           "merged_workspace_bytes", "STAGES", "MERGED_STAGES", "CHARTS"]
