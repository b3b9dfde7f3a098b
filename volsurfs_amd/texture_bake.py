"""Baking a field appearance model (hash grid or permutohedral lattice + MLP: models.ColorSH / models.RGB, the
`using_neural_textures=False` branch of methods.VolSurfs) into a texture over a shell's UV atlas: the reference's
`utils/texture_extraction.py` (`extract_texture_from_color_model`, `extract_textures`, `dilate_texture`) with the
per-face Python loop replaced by device passes (csrc/texture_bake.hip; the rule is in include/volsurfs_hip.h; DESIGN
§22): one sample pass over (face, texel) pairs, the model on a few large batches of rows, one resolve per batch.

* `bake_samples` — the ordered rows a bake evaluates (points, normals, per-texel spans) and the owner map.
* `bake_field_texture` — rows -> `appearance_fn(points, normals)` in chunks -> `[R, R, C]` means.
* `extract_texture_from_color_model`, `extract_textures` — the reference's two functions on top of it.
* `dilate_texture` — the reference's dilation, on the device.
* `to_renderer_layout`, `extract_field_textures` — the float textures `renderers.MeshRenderer` reads, with the shells'
  OBJs and a `scene.json`.
"""
import json
import os

import numpy as np
import torch

from . import _lib

MAX_RES, MAX_SAMPLES = 8192, 64            # include/volsurfs_hip.h
# Rows per model call.  2^20 rows of a ColorSH (48-wide encoding, 128-wide fused MLP, 36 outputs) hold about 0.5 GB
# of activations; the rows themselves (24 bytes each) are at most 1.2 GB at R = 2048, S = 12.
DEFAULT_CHUNK_ROWS = 1 << 20
_CTL_HEAD = 4


class BakeSamples:
    """points [M, 3], normals [M, 3] (rows ordered by texel index ix * R + iy, then by sample); row_start [R^2 + 1]
    int32 (texel t's rows are row_start[t] : row_start[t + 1]); owner [R, R] int32 (the face whose samples a texel
    holds, -1 = uncovered); chunks: [(texel_begin, texel_end, row_begin, row_end)] of at most `chunk_rows` rows."""

    def __init__(self, points, normals, row_start, owner, chunks, resolution, nr_samples):
        self.points, self.normals, self.row_start, self.owner, self.chunks = points, normals, row_start, owner, chunks
        self.resolution, self.nr_samples, self.nr_rows = resolution, nr_samples, int(points.shape[0])


def _check(mesh, texture_res, nr_samples_per_texel, chunk_rows):
    R, S, chunk_rows = int(texture_res), int(nr_samples_per_texel), int(chunk_rows)
    if not 1 <= R <= MAX_RES:
        raise ValueError(f"texture bake: texture_res must lie in [1, {MAX_RES}], got {R}")
    if not 1 <= S <= MAX_SAMPLES:
        raise ValueError(f"texture bake: nr_samples_per_texel must lie in [1, {MAX_SAMPLES}], got {S}")
    if R * R * S > 0x7FFFFFFF:
        raise ValueError(f"texture bake: texture_res^2 * nr_samples_per_texel must stay below 2^31, got {R}^2 * {S}")
    if chunk_rows < S:
        raise ValueError(f"texture bake: chunk_rows ({chunk_rows}) must hold one texel's {S} samples")
    uv = mesh.get_faces_uvs() if hasattr(mesh, "get_faces_uvs") else None
    if uv is None or getattr(mesh, "has_uvs", True) is False:
        raise _lib.VolsurfsHipError("texture bake: the mesh has no UVs (atlas.compute_atlas gives it some)")
    V, F = mesh.vertices, mesh.faces
    if not (V.is_cuda and F.is_cuda and uv.is_cuda):
        raise ValueError(f"texture bake: the mesh must be on cuda, got {V.device} / {F.device} / {uv.device}")
    nf = int(F.shape[0])
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3 or tuple(uv.shape) != (nf, 3, 2):
        raise ValueError(f"texture bake: expected vertices [V, 3], faces [F, 3] and per-corner uvs [F, 3, 2], got "
                         f"{tuple(V.shape)} / {tuple(F.shape)} / {tuple(uv.shape)}")
    if nf == 0:
        raise ValueError("texture bake: the mesh has no faces")
    lo, hi = torch.aminmax(F)           # the emit kernel reads verts[faces[...]] unguarded (one read, whatever F)
    if int(lo) < 0 or int(hi) >= V.shape[0]:
        raise _lib.VolsurfsHipError(f"texture bake: face indices out of range [0, {V.shape[0]}): min {int(lo)}, "
                                    f"max {int(hi)}")
    return (V.to(torch.float32).contiguous(), F.to(torch.int32).contiguous(), uv.to(torch.float32).contiguous(),
            R, S, chunk_rows)


@torch.no_grad()
def bake_samples(mesh, texture_res, nr_samples_per_texel=12, seed=0, chunk_rows=DEFAULT_CHUNK_ROWS):
    """The sample pass of a bake (include/volsurfs_hip.h, "texture bake") -> BakeSamples.  Two host reads whatever the
    mesh: the range of the face indices before the launches, and after them the row count, the chunk table and the UV
    check together.  Raises VolsurfsHipError when a UV is NaN, inf or outside [0, 1] or a face index is out of range,
    ValueError when `chunk_rows` is so small that the bake would take more than 2^20 chunks."""
    V, F, uv, R, S, chunk_rows = _check(mesh, texture_res, nr_samples_per_texel, chunk_rows)
    dev, nf, T = V.device, int(F.shape[0]), R * R
    L = _lib.lib()
    ws = torch.empty(int(L.vsa_tb_workspace_bytes(nf, R)), dtype=torch.uint8, device=dev)
    max_chunks = int(L.vsa_tb_max_chunks(R, S, chunk_rows))
    if max_chunks < 0:
        raise ValueError(f"texture bake: chunk_rows ({chunk_rows}) would split {R}^2 x {S} samples into more than "
                         "2^20 chunks")
    ctl = torch.empty(_CTL_HEAD + 2 * (max_chunks + 1), dtype=torch.int32, device=dev)
    owner = torch.empty(R, R, dtype=torch.int32, device=dev)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    stream = _lib.stream_ptr()
    _lib.call("vsa_tb_samples", uv, nf, R, S, seed, chunk_rows, ws, ws.numel(), owner, ctl, ctl.numel(), stream)
    host = ctl.cpu().tolist()
    if host[2] & 1:
        raise _lib.VolsurfsHipError("texture bake: the mesh's UVs hold NaN, inf or values outside [0, 1]")
    M, n = host[0], host[1]
    if n < 0:
        raise _lib.VolsurfsHipError("texture bake: the chunk table overflowed")
    points = torch.empty(M, 3, device=dev)
    normals = torch.empty(M, 3, device=dev)
    row_start = torch.empty(T + 1, dtype=torch.int32, device=dev)
    _lib.call("vsa_tb_emit", V, F, uv, nf, R, S, seed, ws, ws.numel(), owner, row_start, points, normals, stream)
    tab = host[_CTL_HEAD:_CTL_HEAD + 2 * (n + 1)]          # (first texel, first row) per chunk, then (R^2, M)
    chunks = [(tab[2 * c], tab[2 * c + 2], tab[2 * c + 1], tab[2 * c + 3]) for c in range(n)]
    return BakeSamples(points, normals, row_start, owner, chunks, R, S)


def _aligned(t):
    """A row slice starts at a multiple of 12 bytes; the encoders and the MLP move rows in 16-byte pieces."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


@torch.no_grad()
def bake_field_texture(appearance_fn, mesh, texture_res, nr_samples_per_texel=12, seed=0, return_owner=False,
                       chunk_rows=DEFAULT_CHUNK_ROWS, stage_ms=None):
    """`appearance_fn(points [m, 3], normals [m, 3]) -> [m, C]` baked over the UV atlas of a cuda TensorMesh with
    per-corner UVs -> float32 [R, R, C] in the reference's layout (first index along u, second along v; `to_renderer_
    layout` gives what `renderers.TensorTexture` reads).  A texel holds the mean of the model over the inside samples
    of the highest-numbered face that covers it (sample 0 the texel centre, the others jittered by a counter-based
    generator keyed by `seed`), 0 where no face covers it; the same arguments give the same bytes.  The model sees the
    rows in chunks of at most `chunk_rows` that never split a texel.  return_owner: also the owner map [R, R] int32.
    stage_ms: a dict that receives the device ms of {"samples", "model", "resolve"} (events; synchronises)."""
    ev = (lambda: torch.cuda.Event(enable_timing=True)) if stage_ms is not None else None
    marks = []

    def mark(name):
        if ev is not None:
            e = ev()
            e.record()
            marks.append((name, e))

    mark("start")
    smp = bake_samples(mesh, texture_res, nr_samples_per_texel, seed, chunk_rows)
    mark("samples")
    R, texture, C = smp.resolution, None, None
    stream = _lib.stream_ptr()
    for t0, t1, r0, r1 in smp.chunks:
        if r1 == r0:
            continue
        vals = appearance_fn(_aligned(smp.points[r0:r1]), _aligned(smp.normals[r0:r1]))
        if not torch.is_tensor(vals) or vals.dim() != 2 or vals.shape[0] != r1 - r0:
            got = tuple(vals.shape) if torch.is_tensor(vals) else type(vals)
            raise _lib.VolsurfsHipError(f"texture bake: appearance_fn returned {got} for {r1 - r0} points; expected "
                                        f"[{r1 - r0}, C]")
        vals = _lib.check_f32(vals.detach().contiguous())
        if texture is None:
            C = int(vals.shape[1])
            texture = torch.zeros(R, R, C, device=vals.device)
        elif vals.shape[1] != C:
            raise _lib.VolsurfsHipError(f"texture bake: appearance_fn returned {vals.shape[1]} channels after {C}")
        mark("model")
        _lib.call("vsa_tb_resolve", vals, C, smp.row_start, t0, t1, R, texture, stream)
        mark("resolve")
    if texture is None:           # nothing covered: ask the model for its width on one dummy row
        dev = smp.owner.device
        C = int(appearance_fn(torch.zeros(1, 3, device=dev), torch.ones(1, 3, device=dev)).shape[1])
        texture = torch.zeros(R, R, C, device=dev)
    if stage_ms is not None:
        torch.cuda.synchronize()
        stage_ms.update({"samples": 0.0, "model": 0.0, "resolve": 0.0, "rows": smp.nr_rows,
                         "chunks": len(smp.chunks)})
        for (_, a), (name, b) in zip(marks[:-1], marks[1:]):
            stage_ms[name] += a.elapsed_time(b)
    return (texture, smp.owner) if return_owner else texture


def _model_fn(model, export_rgb, iter_nr):
    if export_rgb:
        return lambda p, n: model(p, samples_dirs=-n, normals=n, iter_nr=iter_nr)
    if getattr(model, "view_dep", False):
        raise _lib.VolsurfsHipError("texture bake: export_rgb=False asks the model for view-independent coefficients; "
                                    f"{type(model).__name__} with view_dep=True has none (ColorSH, or export_rgb=True)")
    return lambda p, n: model(p, samples_dirs=None, normals=n, iter_nr=iter_nr)


@torch.no_grad()
def extract_texture_from_color_model(appearance_model, vertices, faces, uvs, texture_res=512, nr_samples_per_texel=12,
                                     export_rgb=False, iter_nr=None, seed=0, chunk_rows=DEFAULT_CHUNK_ROWS):
    """utils/texture_extraction.py:56-205 -> float32 [R, R, C] device tensor.  `uvs` are per-CORNER [F, 3, 2] (this
    project's TensorMesh; the reference indexes per-vertex uvs by `faces`, which is the same thing for a mesh
    un-welded to 3 F vertices).  export_rgb=False: `model(points, samples_dirs=None, normals=normals, iter_nr=iter_nr)`,
    C = model.out_channels (a ColorSH's coefficients); export_rgb=True: `samples_dirs=-normals`, C = 3.  `seed` keys
    the jitter of samples 1 .. S-1 (the reference draws it from torch's global generator)."""
    from .mesh import TensorMesh
    mesh = TensorMesh(vertices, faces, uvs, device=vertices.device)
    tex = bake_field_texture(_model_fn(appearance_model, export_rgb, iter_nr), mesh, texture_res, nr_samples_per_texel,
                             seed=seed, chunk_rows=chunk_rows)
    want = 3 if export_rgb else int(appearance_model.out_channels)
    if tex.shape[2] != want:
        raise _lib.VolsurfsHipError(f"texture bake: the model returned {tex.shape[2]} channels, expected {want}")
    return tex


def _legacy_models(method, mesh_idx):
    """(rgb model, alpha model or None) of shell `mesh_idx` of a legacy methods.VolSurfs (shared models: keys "rgb" /
    "alpha"; a solid inner mesh has no alpha model)."""
    if getattr(method, "using_neural_textures", False) or not len(getattr(method, "models", {})):
        raise _lib.VolsurfsHipError("field texture extraction bakes the legacy appearance models "
                                    "(using_neural_textures=False); a neural-texture VolSurfs holds its textures "
                                    "already: texture_export.extract_textures writes them")
    if not 0 <= mesh_idx < method.nr_meshes:
        raise ValueError(f"mesh_idx {mesh_idx} outside [0, {method.nr_meshes})")
    rgb = method.models[f"rgb_{mesh_idx}" if method.colors_indep else "rgb"]
    key = f"alpha_{mesh_idx}" if method.alphas_indep else "alpha"
    solid = bool(getattr(method, "solid_inner", False)) and mesh_idx == 0
    return rgb, (method.models[key] if key in method.models and not solid else None)


@torch.no_grad()
def extract_textures(mesh_idx, method, texture_res=512, nr_samples_per_texel=12, iter_nr=None, seed=0):
    """utils/texture_extraction.py:209-260 for a legacy methods.VolSurfs -> (texture, None): the rgb model's texture
    and, when the shell has an alpha model, the alpha model's, concatenated on the channel axis, [R, R, C] in the
    reference's layout."""
    rgb, alpha = _legacy_models(method, int(mesh_idx))
    mesh = method.tensor_meshes[mesh_idx]
    args = (mesh.vertices, mesh.faces, mesh.get_faces_uvs())
    kw = dict(texture_res=texture_res, nr_samples_per_texel=nr_samples_per_texel, iter_nr=iter_nr, seed=seed)
    tex_alpha = extract_texture_from_color_model(alpha, *args, **kw) if alpha is not None else None
    tex = extract_texture_from_color_model(rgb, *args, **kw)
    if tex_alpha is not None:
        tex = torch.cat([tex, tex_alpha], dim=2)
    return tex, None


@torch.no_grad()
def dilate_texture(img, nr_iterations):
    """utils/texture_extraction.py:325-407 on a cuda tensor [H, W, C] -> a new tensor, bit for bit the reference's
    result (include/volsurfs_hip.h, vsa_tb_dilate): empty pixels (all channels 0) next to full ones (no channel 0)
    copy a neighbour, ring by ring, `nr_iterations` times or until an iteration fills nothing."""
    if not torch.is_tensor(img) or img.dim() != 3 or not img.is_cuda:
        raise ValueError("dilate_texture: expected a cuda tensor [H, W, C]")
    nr_iterations = int(nr_iterations)
    if not 0 <= nr_iterations <= 4096:
        raise ValueError(f"dilate_texture: nr_iterations must lie in [0, 4096], got {nr_iterations}")
    out = _lib.check_f32(img.detach().to(torch.float32).contiguous().clone())
    H, W, C = (int(v) for v in out.shape)
    if H == 0 or W == 0 or C == 0 or nr_iterations == 0:
        return out
    stamp = torch.empty(H * W, dtype=torch.int32, device=out.device)
    filled = torch.empty(nr_iterations + 1, dtype=torch.int32, device=out.device)
    _lib.call("vsa_tb_dilate", out, H, W, C, nr_iterations, stamp, filled, _lib.stream_ptr())
    return out


def to_renderer_layout(texture):
    """The reference's [R, R, C] layout (texture[ix, iy], ix along u, iy along v) -> the layout renderers.TensorTexture
    fetches with NeuralTexture.forward's addressing, texture[floor(u R), R - 1 - floor(v R)]: the second axis
    flipped."""
    return torch.flip(texture, [1]).contiguous()


@torch.no_grad()
def extract_field_textures(method, out_dir, texture_res, nr_samples_per_texel=12, dilate=False, nr_dilation_iters=5,
                           cameras=None, resolution=None, bg_color=None, iter_nr=None, seed=0, write_meshes=True):
    """The baker's texture step for a legacy methods.VolSurfs (appearance models that are 3-D fields): per shell m
    <out_dir>/textures/mesh_{m}.npy (float32 [R, R, C], `to_renderer_layout`, after the optional dilation),
    <out_dir>/meshes/{m}.obj and <out_dir>/scene.json, whose "meshes" entries (`mesh_path`, `textures[0].texture_path`,
    `ignore_alpha`) `renderers.MeshRenderer(scene_path=...)` reads; cameras, resolution and background as
    texture_export.scene_info writes them.  A shell without an alpha model (a solid inner mesh) gets what the
    reference gives it: the rgb coefficients alone, [R, R, 3 * nr_coeffs], marked `"ignore_alpha": true` as
    texture_export marks such shells.  MeshRenderer wants four channels of coefficients, so that file is not
    renderable as it is: a reader appends an opaque alpha block (tests/test_texture_bake.py does).  Returns the scene dict.  Raises
    VolsurfsHipError for a neural-texture VolSurfs (texture_export.extract_textures is its exporter)."""
    from .mesh import save_obj
    from .texture_export import scene_info
    _legacy_models(method, 0)
    os.makedirs(os.path.join(out_dir, "textures"), exist_ok=True)
    info = []
    for m in range(method.nr_meshes):
        tex, _ = extract_textures(m, method, texture_res, nr_samples_per_texel, iter_nr=iter_nr, seed=seed)
        if dilate:
            tex = dilate_texture(tex, nr_dilation_iters)
        rel = os.path.join("textures", f"mesh_{m}.npy")
        np.save(os.path.join(out_dir, rel), to_renderer_layout(tex).cpu().numpy())
        info.append({"mesh_path": os.path.join("meshes", f"{m}.obj"),
                     "textures": [{"texture_path": rel, "texture_resolution": [int(tex.shape[0]), int(tex.shape[1])],
                                   "nr_channels": int(tex.shape[2])}],
                     "ignore_alpha": _legacy_models(method, m)[1] is None})
    if write_meshes:
        os.makedirs(os.path.join(out_dir, "meshes"), exist_ok=True)
        for m, mesh in enumerate(method.tensor_meshes):
            save_obj(os.path.join(out_dir, "meshes", f"{m}.obj"), mesh)
    cams = cameras or {}
    if resolution is None:
        first = next((c for split in ("train", "test") for c in cams.get(split, [])), None)
        resolution = (first.width, first.height) if first is not None else (800, 800)
    scene = scene_info(info, resolution, method.bg_color if bg_color is None else bg_color, cams)
    scene["volsurfs_amd"]["field_textures"] = True
    with open(os.path.join(out_dir, "scene.json"), "w") as f:
        json.dump(scene, f, indent=2)
    return scene
