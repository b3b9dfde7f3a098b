"""Export of baked shell textures as PNGs + `scene.json`, and the loader that renders them again: the baker's
`--extract_textures` step (volsurfs_py/baker.py:778-1009) and its inverse.

* `export_planes` — the RGBA8 images of a baked NeuralTextureBank, in PNG orientation, from one
  `vsa_nt_export_planes` launch (csrc/texture_io.hip).
* `opengl_camera` / `scene_info` — the cameras and the dict of the reference's `scene.json`.
* `extract_textures` — bake if needed, then write `textures/mesh_{m}_texture_{d}_feature_{i}.png`,
  `meshes/{m}.obj` and `scene.json`.
* `load_scene` — read such a directory back into a `BakedScene` that renders through the same trace ->
  `tex_uv_only` -> `shade` -> `composite_dense` path as `VolSurfs.render_baked`.
"""
import ctypes
import json
import math
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .methods import VolSurfs
from .neural_textures import MAX_DEG, NeuralTextureBank

FORMAT_VERSION = 1
NEAR, FAR = 0.1, 100.0
_FLIP_YZ = np.diag([1.0, -1.0, -1.0, 1.0])
_PNG_THREADS = 16


def texture_name(mesh_idx, degree, feature):
    """baker.py:68: the file name of coefficient `feature` of SH degree `degree` of shell `mesh_idx`."""
    return f"mesh_{mesh_idx}_texture_{degree}_feature_{feature}.png"


def plane_layout(resolutions, K, D):
    """([(shell, degree, byte offset, coefficients, R)], total bytes) of the planes of K shells and D degrees with these
    per-degree resolutions, in the planes' order (include/volsurfs_hip.h; csrc/nt_common.h nt_plane_layout)."""
    out, off = [], 0
    for s in range(K):
        for d in range(D):
            R, n = int(resolutions[d]), 2 * d + 1
            out.append((s, d, off, n, R))
            off += n * R * R * 4
    return out, off


def plane_views(flat, layout):
    """{(shell, degree): [2d+1, R, R, 4] view} of a flat buffer (torch or numpy) with `plane_layout`'s layout."""
    return {(s, d): flat[off:off + n * R * R * 4].reshape(n, R, R, 4) for s, d, off, n, R in layout}


def _planes_bytes(bank):
    n = _lib.lib().vsa_nt_planes_bytes(ctypes.byref(bank.plan))
    if n < 0:
        raise _lib.VolsurfsHipError(f"vsa_nt_planes_bytes failed with status {n}")
    return int(n)


def _check_exportable(bank):
    if bank.row_format != 0:
        raise _lib.VolsurfsHipError("texture export writes 8-bit textures: using_sh_quantization=1 only")
    if bank.alpha_degrees != bank.rgb_degrees:
        raise _lib.VolsurfsHipError(
            "texture export needs as many alpha SH degrees as rgb ones (transp_view_dep=1): the reference pairs them "
            "with zip(rgb, alpha) and would drop the rgb degrees above the alpha ones")


def baked_bank_of(scene, what):
    """The baked, exportable bank of `scene` (a BakedScene, or a VolSurfs after bake()); `what` names the caller."""
    bank = getattr(scene, "baked", None)
    if bank is None or not getattr(bank, "baked", False):
        raise _lib.VolsurfsHipError(f"{what} needs a baked scene: a BakedScene, or a VolSurfs after bake()")
    _check_exportable(bank)
    return bank


def _export_flat(bank):
    """(uint8 device buffer of every image, layout) from one vsa_nt_export_planes launch."""
    if not getattr(bank, "baked", False):
        raise _lib.VolsurfsHipError("export_planes needs a baked bank (VolSurfs.bake() / NeuralTextureBank.bake_all())")
    _check_exportable(bank)
    total = _planes_bytes(bank)
    planes = torch.empty(total, dtype=torch.uint8, device=bank.texels.device)
    _lib.call("vsa_nt_export_planes", ctypes.byref(bank.plan), bank.slot_of, bank.seg_start, bank.texels, planes,
              total, _lib.stream_ptr())
    return planes, plane_layout(bank.tex_res, bank.K, bank.D)[0]


@torch.no_grad()
def export_planes(bank):
    """{(shell, degree): uint8 [2d+1, R, R, 4]} device views into one buffer: coefficient i of (shell, degree) as the
    RGBA image of `textures/mesh_{shell}_texture_{degree}_feature_{i}.png` (pixel (r, c) = texel (c, R-1-r) of
    `bank.baked_textures()`; A = 255 on a shell without an alpha model).  `bank` must be baked."""
    planes, layout = _export_flat(bank)
    return plane_views(planes, layout)


def opengl_camera(camera, near=NEAR, far=FAR):
    """(projectionMatrix, matrixWorld) of a `camera.Camera` as float64 4x4 arrays, the pair the reference writes per
    camera (mvdatasets' get_opengl_projection_matrix / get_opengl_matrix_world; that package is absent, so the rule is
    this project's):
      matrixWorld = c2w . diag(1, -1, -1, 1)   (the camera here is x right, y down, z forward; OpenGL's eye space is
                                                 y up, z backward)
      projectionMatrix = [[2 fx / W, 0, 1 - 2 cx / W, 0],
                          [0, 2 fy / H, 2 cy / H - 1, 0],
                          [0, 0, -(f + n) / (f - n), -2 f n / (f - n)],
                          [0, 0, -1, 0]]
    so that a world point projects (through projectionMatrix . inv(matrixWorld) and the divide by w) to pixel
    x = (ndc_x + 1) / 2 W, y = (1 - ndc_y) / 2 H, and depths near / far to ndc z = -1 / +1."""
    K = camera.intrinsics.detach().cpu().double().numpy()
    W, H = float(camera.width), float(camera.height)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    n, f = float(near), float(far)
    proj = np.array([[2 * fx / W, 0.0, 1 - 2 * cx / W, 0.0],
                     [0.0, 2 * fy / H, 2 * cy / H - 1, 0.0],
                     [0.0, 0.0, -(f + n) / (f - n), -2 * f * n / (f - n)],
                     [0.0, 0.0, -1.0, 0.0]])
    c2w = np.eye(4)
    c2w[:3, :4] = camera.c2w.detach().cpu().double().numpy()
    return proj, c2w @ _FLIP_YZ


def camera_from_opengl(projection, matrix_world, width, height, device="cuda"):
    """The inverse of `opengl_camera`: a `camera.Camera` of `width` x `height` pixels."""
    from .camera import Camera
    P, M = np.asarray(projection, np.float64), np.asarray(matrix_world, np.float64)
    W, H = float(width), float(height)
    K = [[P[0, 0] * W / 2, 0.0, (1 - P[0, 2]) * W / 2], [0.0, P[1, 1] * H / 2, (P[1, 2] + 1) * H / 2], [0.0, 0.0, 1.0]]
    c2w = M @ _FLIP_YZ
    return Camera(K, c2w[:3, :4], int(height), int(width), device=device)


def _bg_entry(bg_color):
    if bg_color is None:
        return "black"
    if isinstance(bg_color, str):
        return bg_color
    c = [float(v) for v in torch.as_tensor(bg_color, dtype=torch.float32).flatten().tolist()]
    if len(c) != 3:
        raise ValueError(f"bg_color must hold 3 values, got {len(c)}")
    if c == [1.0, 1.0, 1.0]:
        return "white"
    if c == [0.0, 0.0, 0.0]:
        return "black"
    return c


def scene_info(meshes_info, resolution, bg_color, cameras, lerp=True, with_alpha_decay=True):
    """The dict of the reference's scene.json (baker.py:956-1005):
      "resolution": [[W, H]], "bg_color": "white" / "black" / [r, g, b] ("black" for None, as the reference writes when
      no colour is set), "meshes": meshes_info (a list of {"mesh_path", "textures", "ignore_alpha"}), "cameras":
      {"test": {idx: {...}}, "train": {idx: {...}}} with each camera's OpenGL "projectionMatrix" (near 0.1, far 100)
      and "matrixWorld" as nested row lists, keyed by the camera's index in its list;
    plus "volsurfs_amd": {"format", "lerp", "with_alpha_decay"}, the render settings the loader needs (readers of the
    reference's format ignore the key).  resolution: (W, H); cameras: {"train": [Camera], "test": [Camera]} or None."""
    W, H = (int(v) for v in resolution)
    out = {"resolution": [[W, H]], "bg_color": _bg_entry(bg_color), "meshes": list(meshes_info),
           "cameras": {"test": {}, "train": {}}}
    for split in ("test", "train"):
        for idx, cam in enumerate((cameras or {}).get(split, [])):
            proj, world = opengl_camera(cam)
            out["cameras"][split][idx] = {"projectionMatrix": proj.tolist(), "matrixWorld": world.tolist()}
    out["volsurfs_amd"] = {"format": FORMAT_VERSION, "lerp": bool(lerp), "with_alpha_decay": bool(with_alpha_decay)}
    return out


def meshes_info_of(nr_meshes, textures_res, sh_range, degrees, ignore_alpha):
    """The "meshes" list of scene.json: per shell its OBJ and, in (degree, feature) order, every texture with
    texture_scale [-sh_range[d], sh_range[d]] and texture_resolution [R, R]."""
    out = []
    for m in range(nr_meshes):
        tex = []
        for d in range(degrees):
            R = int(textures_res[d])
            for i in range(2 * d + 1):
                tex.append({"texture_path": os.path.join("textures", texture_name(m, d, i)),
                            "texture_scale": [-float(sh_range[d]), float(sh_range[d])],
                            "texture_resolution": [R, R]})
        out.append({"mesh_path": os.path.join("meshes", f"{m}.obj"), "textures": tex,
                    "ignore_alpha": bool(ignore_alpha[m])})
    return out


def _save_png(path, img, compress_level):
    from PIL import Image
    Image.fromarray(img).save(path, compress_level=int(compress_level))


@torch.no_grad()
def extract_textures(method, out_dir, cameras=None, resolution=None, bg_color=None, compress_level=6,
                     write_meshes=True, timings=None):
    """The baker's `--extract_textures` for a `methods.VolSurfs` on the neural-texture branch: bake if `method.baked`
    is None, then write <out_dir>/textures/mesh_{m}_texture_{d}_feature_{i}.png (RGBA8), <out_dir>/meshes/{m}.obj (the
    shells with their per-corner UVs, mesh.save_obj) and <out_dir>/scene.json; returns the scene dict.
    cameras: {"train": [Camera], "test": [Camera]}; resolution: (W, H), default the first camera's, else (800, 800);
    bg_color: the dataset's colour or name, default the method's constant background (a learned one is not exported:
    "black").  compress_level: zlib level of the PNGs (encoded on the host, up to 16 threads).
    timings: a dict that receives {bake_ms, export_ms, d2h_ms, png_s, meshes_s} (wall clock).
    Raises VolsurfsHipError for the legacy appearance branch, a bank that is not 8-bit and transp_view_dep=0 with
    sh_degree > 0."""
    if not getattr(method, "using_neural_textures", False) or method.bank is None:
        raise _lib.VolsurfsHipError("legacy texture extraction method deprecated: texture export needs "
                                    "using_neural_textures=1 (the reference exits here, baker.py:896-900)")
    _check_exportable(method.bank)
    t = {} if timings is None else timings
    t0 = _now()
    if method.baked is None:
        method.bake()
    t["bake_ms"] = (_now() - t0) * 1e3
    return _write_baked(method, method.baked, out_dir, cameras or {}, resolution,
                        method.bg_color if bg_color is None else bg_color, compress_level, write_meshes, t)


def _now():
    torch.cuda.synchronize()
    return time.perf_counter()


def _write_baked(scene, bank, out_dir, cams, resolution, bg_color, compress_level, write_meshes, t):
    """The writer of `extract_textures` and `write_scene`: the PNGs of `bank`, the OBJs of `scene.tensor_meshes` and
    scene.json; returns the scene dict.  resolution None: the first camera's, else (800, 800).  t: a dict that
    receives {export_ms, d2h_ms, png_s, meshes_s} (wall clock)."""
    from .mesh import save_obj
    t1 = _now()
    planes, layout = _export_flat(bank)
    t2 = _now()
    flat = planes.cpu().numpy()
    t3 = _now()
    tex_dir = os.path.join(out_dir, "textures")
    os.makedirs(tex_dir, exist_ok=True)
    jobs = []
    for (s, d), img in plane_views(flat, layout).items():
        jobs.extend((os.path.join(tex_dir, texture_name(s, d, i)), img[i]) for i in range(len(img)))
    with ThreadPoolExecutor(max_workers=min(_PNG_THREADS, len(jobs))) as ex:
        list(ex.map(lambda j: _save_png(j[0], j[1], compress_level), jobs))
    t4 = time.perf_counter()
    if write_meshes:
        os.makedirs(os.path.join(out_dir, "meshes"), exist_ok=True)
        for m, mesh in enumerate(scene.tensor_meshes):
            save_obj(os.path.join(out_dir, "meshes", f"{m}.obj"), mesh)
    t5 = time.perf_counter()
    ignore = [bank.tex_channels(bank.tex_index(s, 1, 0)) == 0 for s in range(bank.K)]   # no alpha model
    sh_range = [-float(bank.plan.sh_lo[d]) for d in range(MAX_DEG)]
    info = meshes_info_of(bank.K, bank.tex_res, sh_range, bank.D, ignore)
    if resolution is None:
        first = next((c for split in ("train", "test") for c in cams.get(split, [])), None)
        resolution = (first.width, first.height) if first is not None else (800, 800)
    out = scene_info(info, resolution, bg_color, cams, lerp=not bank.anchor,
                     with_alpha_decay=bool(bank.plan.with_alpha_decay))
    with open(os.path.join(out_dir, "scene.json"), "w") as f:
        json.dump(out, f, indent=2)
    t.update({"export_ms": (t2 - t1) * 1e3, "d2h_ms": (t3 - t2) * 1e3, "png_s": t4 - t3, "meshes_s": t5 - t4})
    return out


# ---------------------------------------------------------------------------------------------------------------------
# loading

_BG_NAMES = {"white": (1.0, 1.0, 1.0), "black": (0.0, 0.0, 0.0)}


def _bg_color_of(entry):
    if isinstance(entry, str):
        if entry not in _BG_NAMES:
            raise _lib.VolsurfsHipError(f"scene.json: unknown bg_color {entry!r} (expected white, black or [r, g, b])")
        return _BG_NAMES[entry]
    c = [float(v) for v in entry]
    if len(c) != 3:
        raise _lib.VolsurfsHipError(f"scene.json: bg_color must hold 3 values, got {entry!r}")
    return tuple(c)


def _scene_layout(meta):
    """(degrees D, per-degree resolutions, per-degree sh_range, ignore_alpha per mesh) of scene.json's "meshes", checked:
    every mesh lists D^2 textures in (degree, feature) order with the same square per-degree resolutions and scales."""
    meshes = meta.get("meshes") or []
    if not meshes:
        raise _lib.VolsurfsHipError("scene.json: no meshes")
    ref = None
    for m, mesh in enumerate(meshes):
        tex = mesh.get("textures") or []
        D = math.isqrt(len(tex))
        if D * D != len(tex) or not 1 <= D <= MAX_DEG:
            raise _lib.VolsurfsHipError(f"scene.json: mesh {m} lists {len(tex)} textures; expected D^2 for D in 1..4 "
                                        "(degrees 0..D-1 with 2d+1 features each)")
        res, rng, j = [], [], 0
        for d in range(D):
            for i in range(2 * d + 1):
                t = tex[j]
                j += 1
                R = [int(v) for v in t["texture_resolution"]]
                lo, hi = (float(v) for v in t["texture_scale"])
                if len(R) != 2 or R[0] != R[1] or R[0] < 1:
                    raise _lib.VolsurfsHipError(f"scene.json: mesh {m} texture {t['texture_path']}: resolution {R} is "
                                                "not square")
                if lo != -hi:
                    raise _lib.VolsurfsHipError(f"scene.json: mesh {m} texture {t['texture_path']}: texture_scale "
                                                f"[{lo}, {hi}] is not symmetric")
                if i == 0:
                    res.append(R[0])
                    rng.append(hi)
                elif (R[0], hi) != (res[d], rng[d]):
                    raise _lib.VolsurfsHipError(f"scene.json: mesh {m} degree {d}: features differ in resolution or "
                                                "scale")
        if ref is None:
            ref = (D, res, rng)
        elif (D, res, rng) != ref:
            raise _lib.VolsurfsHipError(f"scene.json: mesh {m} has degrees / resolutions / scales {(D, res, rng)}, "
                                        f"mesh 0 {ref}: every shell must match")
    ignore = [bool(mesh.get("ignore_alpha", False)) for mesh in meshes]
    return ref[0], ref[1], ref[2], ignore


def _alpha_flags(ignore):
    """(inner_solid, shared_alpha) of NeuralTextureBank that give the shells these ignore_alpha flags
    (nt_shell_has_alpha: none, the inner shell only, or every shell)."""
    K = len(ignore)
    if not any(ignore):
        return False, False
    if ignore[0] and not any(ignore[1:]):
        return True, False
    if all(ignore):
        return True, True
    raise _lib.VolsurfsHipError(f"scene.json: ignore_alpha {ignore} is not representable: only the inner shell "
                                f"or all {K} shells can lack an alpha model")


def _read_png(path, R):
    from PIL import Image
    with Image.open(path) as im:
        if im.size != (R, R):
            raise _lib.VolsurfsHipError(f"{path}: {im.size[0]} x {im.size[1]} pixels, scene.json says {R} x {R}")
        if im.mode != "RGBA":
            raise _lib.VolsurfsHipError(f"{path}: mode {im.mode}; the textures are RGBA (four channels)")
        return np.asarray(im)


class BakedScene:
    """A scene read back by `load_scene`: the shells, their BVHs, a bank that holds the 8-bit textures only (no hash
    tables, no MLP weights, no feature planes or gradient buffers), the background colour and the cameras.
    render_rays / render_baked return the dict of VolSurfs.render_baked, through the same code."""

    def __init__(self, meshes, bank, bg_color, cameras, resolution, bvh_builder="host"):
        from .raytrace import RayTracer
        self.tensor_meshes, self.nr_meshes = meshes, len(meshes)
        self.raytracer = RayTracer(meshes, builder=bvh_builder)
        self.face_uvs = self.raytracer.slot_face_uvs(meshes)
        self.baked = bank
        self.mips = None            # a texture_mip.MipChain of `baked` (build_mips)
        self.bg_color = torch.tensor([bg_color], dtype=torch.float32, device=bank.texels.device)
        self.cameras = cameras
        self.resolution = resolution

    # VolSurfs' own methods, so that a loaded scene and a baked method render through one path
    _trace_now = VolSurfs._trace_now
    render_baked = VolSurfs.render_baked
    _shade_baked = VolSurfs._shade_baked
    _composite_baked = VolSurfs._composite_baked
    _camera_hit_chunks = VolSurfs._camera_hit_chunks
    render_baked_camera = VolSurfs.render_baked_camera
    build_mips = VolSurfs.build_mips
    refit_to = VolSurfs.refit_to

    def render_rays(self, rays_o, rays_d, chunk=1 << 20):
        return self.render_baked(rays_o, rays_d, chunk=chunk)


def _empty_baked_bank(K, D, res, rng, inner_solid, shared_alpha, decay, lerp, device):
    """A bank of K shells and D degrees that holds 8-bit texel rows only, every texel of every domain with the slot
    `bake_all` would give it, the rows not yet written.  res / rng: the D per-degree resolutions and sh ranges."""
    textures_res = list(res) + [res[-1]] * (MAX_DEG - D)
    sh_range = list(rng) + [rng[-1]] * (MAX_DEG - D)
    bank = NeuralTextureBank(K, NeuralTextureBank.full_capacity_rays(res), sh_degree=D - 1, alpha_sh_degree=D - 1,
                             sh_range=sh_range, textures_res=textures_res, inner_solid=inner_solid,
                             with_alpha_decay=decay, device=device, training=False, anchor=not lerp, lerp=lerp,
                             shared_alpha=shared_alpha, parameters=False)
    bank.compact_all(want_texel_of_slot=False)
    # only slot_of / seg_start / texels are read from here on
    bank.marks = bank.slot_xy = bank.texel_of_slot = bank.block_scratch = None
    return bank


def _import_planes(bank, planes):
    """The flat device buffer of every image (export_planes' order) into the bank's texel rows, the apron clamped to
    the edge (vsa_nt_import_planes); the bank is baked afterwards."""
    total = _planes_bytes(bank)
    if planes.dtype != torch.uint8 or planes.numel() != total:
        raise _lib.VolsurfsHipError(f"expected {total} plane bytes (uint8), got {planes.numel()} of {planes.dtype}")
    _lib.call("vsa_nt_import_planes", ctypes.byref(bank.plan), planes, total, bank.slot_of, bank.seg_start,
              bank.texels, _lib.stream_ptr())
    bank.baked = True
    bank.texels_version += 1


@torch.no_grad()
def write_scene(scene, out_dir, cameras=None, resolution=None, compress_level=6, write_meshes=True):
    """Write a `BakedScene` (or a baked VolSurfs) the way `extract_textures` writes a method: the same
    textures/mesh_{m}_texture_{d}_feature_{i}.png, meshes/{m}.obj and scene.json, so that `load_scene` and
    `VolsurfsRenderer.from_scene` read it.  cameras / resolution default to the scene's own; returns the scene dict."""
    bank = baked_bank_of(scene, "write_scene")
    cams = cameras if cameras is not None else (getattr(scene, "cameras", None) or {})
    if resolution is None:
        resolution = getattr(scene, "resolution", None)
    return _write_baked(scene, bank, out_dir, cams, resolution, scene.bg_color, compress_level, write_meshes, {})


@torch.no_grad()
def load_scene(scene_path, device="cuda", bvh_builder="host", timings=None, mips=None):
    """Read a directory written by `extract_textures` (scene.json, meshes/*.obj, textures/*.png) into a BakedScene.
    mips: None, or the levels of the mip chain to build after loading (`BakedScene.build_mips(levels=mips)`; the chain
    is derived, nothing of it is on disk).
    sh_range comes from texture_scale, the degrees and resolutions from the texture list, the alpha models from
    ignore_alpha and lerp / with_alpha_decay from the "volsurfs_amd" key (absent: lerp, with alpha decay — the shipped
    configs).  The textures are uploaded with vsa_nt_import_planes into the slots `bake_all` would give them; the
    one-texel apron is clamped to the edge (include/volsurfs_hip.h).  Raises VolsurfsHipError for a scene whose shells
    differ in degrees, resolutions or scales, whose PNGs differ from texture_resolution or are not RGBA.
    timings: a dict that receives {meshes_s, png_s, h2d_ms, import_ms} (wall clock)."""
    from .mesh import load_obj
    t = {} if timings is None else timings
    with open(os.path.join(scene_path, "scene.json")) as f:
        meta = json.load(f)
    D, res, rng, ignore = _scene_layout(meta)
    inner_solid, shared_alpha = _alpha_flags(ignore)
    opts = meta.get("volsurfs_amd") or {}
    lerp, decay = bool(opts.get("lerp", True)), bool(opts.get("with_alpha_decay", True))
    t0 = time.perf_counter()
    meshes = [load_obj(os.path.join(scene_path, m["mesh_path"]), device=device) for m in meta["meshes"]]
    t1 = time.perf_counter()
    K = len(meshes)
    bank = _empty_baked_bank(K, D, res, rng, inner_solid, shared_alpha, decay, lerp, device)
    layout, total = plane_layout(res, K, D)
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    flat = host.numpy()
    jobs = []
    for s, d, off, n, R in layout:
        tex = meta["meshes"][s]["textures"][d * d:(d + 1) * (d + 1)]
        for i in range(n):
            jobs.append((os.path.join(scene_path, tex[i]["texture_path"]), R, off + i * R * R * 4))

    def decode(job):
        path, R, off = job
        flat[off:off + R * R * 4] = _read_png(path, R).reshape(-1)
    with ThreadPoolExecutor(max_workers=min(_PNG_THREADS, len(jobs))) as ex:
        list(ex.map(decode, jobs))
    t2 = time.perf_counter()
    planes = host.to(device)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    _import_planes(bank, planes)
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    W, H = (int(v) for v in meta.get("resolution", [[800, 800]])[0])
    cameras = {}
    for split, cams in (meta.get("cameras") or {}).items():
        cameras[split] = [camera_from_opengl(c["projectionMatrix"], c["matrixWorld"], W, H, device=device)
                          for _, c in sorted(cams.items(), key=lambda kv: int(kv[0]))]
    scene = BakedScene(meshes, bank, _bg_color_of(meta.get("bg_color", "black")), cameras, (W, H), bvh_builder)
    t.update({"meshes_s": t1 - t0, "png_s": t2 - t1, "h2d_ms": (t3 - t2) * 1e3, "import_ms": (t4 - t3) * 1e3})
    if mips is not None:
        scene.build_mips(levels=mips)
    return scene
