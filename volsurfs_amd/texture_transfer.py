"""Baked textures carried from one stack of shells onto another with other faces and other UVs, on the device
(csrc/texture_transfer.hip; the rule in include/volsurfs_hip.h "Texture transfer").  The reference has no such
stage: the rule is this library's own, restated in tests/texture_transfer_restated.py and unpinned.

A baked scene is valid only for the meshes and atlases it was trained on; every stage that changes faces or UVs afterwards
(`simplify_shells`, `post_process_mesh`, `remove_invisible_faces`, `repair_mesh`, another `compute_atlas`) used to throw
the trained appearance away.  Here each texel of the new atlas finds the face that owns it, the point of that face in
space, the closest point of the SAME shell of the source (`RayTracer.closest`'s bits) and the coefficients the baked shade
would fetch there, and stores the nearest byte.

* `texel_owners` — which face owns each texel of an atlas, with barycentrics and squared texel distance.
* `transfer_planes` — the planes of `export_planes` for the destination meshes, and the reports.
* `transfer_scene` — the same as a `BakedScene` that renders.
* `make_lod` / `lod_chain` — `simplify_shells` + `compute_atlas` + `transfer_scene`: lighter copies of a baked scene.

NOT promised: appearance is resampled, not retrained; coefficients are filtered BEFORE the SH sum and the sigmoid; the two
charts that meet at a seam may disagree; destination surface far from the source takes the nearest source value, and only
the report (`max_distance`, `rms_distance`, `far`) says so.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from .mesh import TensorMesh

STAT_WORDS = 8
MAX_REACH = 64.0


def _check_options(samples, reach, max_distance):
    if isinstance(samples, bool) or int(samples) != samples or not 1 <= int(samples) <= 4:
        raise _lib.VolsurfsHipError(f"texture transfer: samples must be an integer in 1..4, got {samples!r}")
    reach, max_distance = float(reach), float(max_distance)
    if not 0.0 <= reach <= MAX_REACH:
        raise _lib.VolsurfsHipError(f"texture transfer: reach must lie in [0, {MAX_REACH:g}] texels, got {reach}")
    if math.isnan(max_distance):
        raise _lib.VolsurfsHipError("texture transfer: max_distance is NaN")
    return int(samples), reach, max_distance


def _check_resolution(R, what):
    if isinstance(R, bool) or int(R) != R or not 1 <= int(R) <= 16384:
        raise _lib.VolsurfsHipError(f"{what}: resolution must be an integer in 1..16384, got {R!r}")
    return int(R)


def _dst_tables(meshes, what):
    """(uvs [F, 3, 2], records [F, 12], face_base (host, K + 1)) of the destination shells, one after the other: the
    per-corner UVs and the records (v0, e1 = v1 - v0, e2 = v2 - v0) of vsa_surface_sample's expression."""
    uvs, recs, base = [], [], [0]
    for k, m in enumerate(meshes):
        if not isinstance(m, TensorMesh):
            raise _lib.VolsurfsHipError(f"{what}: shell {k} is a {type(m).__name__}, expected a TensorMesh")
        uv = m.get_faces_uvs()
        if uv is None:
            raise _lib.VolsurfsHipError(f"{what}: shell {k} has no per-corner UVs (compute_atlas gives them)")
        V, F = m.vertices, m.faces
        if not (V.is_cuda and F.is_cuda and uv.is_cuda):
            raise _lib.VolsurfsHipError(f"{what}: shell {k} must be on cuda")
        nf = int(F.shape[0])
        if nf < 1 or F.dim() != 2 or F.shape[1] != 3 or V.dim() != 2 or V.shape[1] != 3 or tuple(uv.shape) != (nf, 3, 2):
            raise _lib.VolsurfsHipError(f"{what}: shell {k}: expected vertices [V, 3], faces [F >= 1, 3] and UVs "
                                        f"[F, 3, 2], got {tuple(V.shape)} / {tuple(F.shape)} / {tuple(uv.shape)}")
        uvs.append(uv.to(torch.float32))
        base.append(base[-1] + nf)
    for k, m in enumerate(meshes):                      # (after the argument checks: the first device work)
        V, F = m.vertices.to(torch.float32), m.faces.long()
        lo, hi = torch.aminmax(F)
        if int(lo) < 0 or int(hi) >= V.shape[0]:
            raise _lib.VolsurfsHipError(f"{what}: shell {k}: face indices out of range [0, {V.shape[0]})")
        v0, v1, v2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
        rec = torch.zeros(F.shape[0], 12, device=V.device)
        rec[:, 0:3], rec[:, 4:7], rec[:, 8:11] = v0, v1 - v0, v2 - v0
        recs.append(rec)
    return torch.cat(uvs).contiguous(), torch.cat(recs).contiguous(), (ctypes.c_longlong * len(base))(*base)


def _workspace(K, R, device):
    n = _lib.workspace_bytes("vsa_textransfer_workspace_bytes", K, R)
    return torch.empty(n, dtype=torch.uint8, device=device), n


@torch.no_grad()
def texel_owners(mesh, resolution, reach=1.5):
    """(face [R, R] i32, bary [R, R, 2] f32, d2 [R, R] f32) of a cuda TensorMesh with per-corner UVs, in
    `rasterize_atlas`' orientation (row j holds texel centres v = (j + 0.5) / R, column i u = (i + 0.5) / R): the face
    that owns each texel (-1: unowned), the weights of its second and third corner at the point of its uv triangle
    nearest to the texel centre, and the squared distance to it in texels (0: the centre is covered; +inf: unowned).
    Wherever `rasterize_atlas` says a face covers the texel, the owner is its `face_id` (the lowest such face) with
    d2 = 0; elsewhere the minimum over (d2 bits, face id) of the faces within `reach` texels."""
    R = _check_resolution(resolution, "texel_owners")
    _, reach, _ = _check_options(1, reach, 0.0)
    uvs, recs, base = _dst_tables([mesh], "texel_owners")
    dev = uvs.device
    ws, n = _workspace(1, R, dev)
    _lib.call("vsa_textransfer_owners", uvs, recs, base, 1, R, reach, ws, n, _lib.stream_ptr())
    face = torch.empty(R, R, dtype=torch.int32, device=dev)
    bary = torch.empty(R, R, 2, device=dev)
    d2 = torch.empty(R, R, device=dev)
    _lib.call("vsa_textransfer_owner_fields", ws, n, uvs, base, 1, 0, R, face, bary, d2, _lib.stream_ptr())
    return face, bary, d2


def _source(src, builder):
    """(tracer with q16 nodes, per-slot uv table) of anything that renders baked."""
    from .raytrace import RayTracer
    tracer, face_uvs = src.raytracer, src.face_uvs
    if tracer.node_format != "q16":
        tracer = RayTracer(src.tensor_meshes, builder=builder)
        face_uvs = tracer.slot_face_uvs(src.tensor_meshes)
    tracer.require_q16("texture transfer")
    return tracer, face_uvs


def _report(words, samples, texels):
    owned, covered, n, dmax, far, s2 = (int(w) for w in words[:6])
    d = float(np.array([dmax], np.uint64).astype(np.uint32).view(np.float32)[0])
    sum_d2 = float(np.array([s2], np.int64).view(np.float64)[0])
    return {"texels": texels, "owned": owned, "covered": covered, "samples": n, "max_distance": d,
            "rms_distance": math.sqrt(sum_d2 / n) if n else 0.0, "sum_d2": sum_d2, "far": far}


@torch.no_grad()
def transfer_planes(src, dst_meshes, textures_res=None, samples=1, reach=1.5, max_distance=math.inf,
                    builder="device"):
    """(planes, reports): the baked textures of `src` (a `BakedScene`, or a `VolSurfs` after `bake()`) carried onto
    `dst_meshes`, K cuda TensorMeshes with per-corner UVs, shell k from the source's shell k.
    planes: {(shell, degree): uint8 [2d+1, R', R', 4]} device views in `export_planes`' layout, R' = textures_res[d]
    (default: the source's).  reports: {(shell, degree): {texels, owned, covered, samples, max_distance, rms_distance,
    sum_d2, far}} -- the 3-D distances from the samples' points to their closest source points, `far` the samples
    beyond `max_distance`; read with one blocking read.  samples = s: an s x s grid per texel, averaged before the
    byte is chosen.  reach: how far (in texels) from its uv triangle a face still owns a texel; 1.5 covers every texel
    a bilinear lookup on the mesh can read.  builder: of the tree built when the source's tracer has no q16 nodes.
    The same inputs give the same bytes.  Raises VolsurfsHipError for a shell-count mismatch, meshes without UVs,
    resolutions out of range and a source that is not exportable, before any launch."""
    from .neural_textures import MAX_DEG
    from .texture_export import _export_flat, baked_bank_of, plane_layout, plane_views
    samples, reach, max_distance = _check_options(samples, reach, max_distance)
    bank = baked_bank_of(src, "texture transfer")
    dst_meshes = list(dst_meshes)
    K, D = bank.K, bank.D
    if len(dst_meshes) != K:
        raise _lib.VolsurfsHipError(f"texture transfer: {len(dst_meshes)} destination meshes for a source of {K} shells")
    res = list(bank.tex_res if textures_res is None else textures_res)
    if len(res) < D:
        raise _lib.VolsurfsHipError(f"texture transfer: textures_res needs {D} entries, got {len(res)}")
    res = [_check_resolution(r, "texture transfer") for r in res[:D]]
    for k, m in enumerate(dst_meshes):
        if not isinstance(m, TensorMesh) or m.get_faces_uvs() is None:
            raise _lib.VolsurfsHipError(f"texture transfer: destination shell {k} has no per-corner UVs")
    tracer, face_uvs = _source(src, builder)
    uvs, recs, base = _dst_tables(dst_meshes, "texture transfer")
    dev = uvs.device
    src_planes, _ = _export_flat(bank)
    dst_res = (ctypes.c_int32 * MAX_DEG)(*(res + [res[-1]] * (MAX_DEG - D)))
    layout, total = plane_layout(res, K, D)
    dst_planes = torch.empty(total, dtype=torch.uint8, device=dev)
    stats = torch.empty(D, K, STAT_WORDS, dtype=torch.int64, device=dev)
    for d in range(D):
        ws, n = _workspace(K, res[d], dev)
        _lib.call("vsa_textransfer_owners", uvs, recs, base, K, res[d], reach, ws, n, _lib.stream_ptr())
        _lib.call("vsa_textransfer_planes", ctypes.byref(bank.plan), d, src_planes, src_planes.numel(),
                  *tracer.q16_tree_args(), face_uvs, uvs, recs, base, dst_res, samples, max_distance, ws, n,
                  dst_planes, total, stats[d], _lib.stream_ptr())
    words = stats.cpu().numpy()                     # the one blocking read
    reports = {(s, d): _report(words[d, s], samples, res[d] * res[d]) for s in range(K) for d in range(D)}
    return plane_views(dst_planes, layout), reports


@torch.no_grad()
def scene_from_planes(meshes, planes, sh_range, inner_solid=False, shared_alpha=False, lerp=True,
                      with_alpha_decay=True, bg_color=(1.0, 1.0, 1.0), cameras=None, resolution=(800, 800),
                      builder="device"):
    """A `BakedScene` of `meshes` (K cuda TensorMeshes with UVs) whose bank holds `planes` ({(shell, degree): uint8
    [2d+1, R_d, R_d, 4]} in `export_planes`' layout): built and filled the way `load_scene` builds one from PNGs (the
    same constructor arguments, vsa_nt_import_planes: the apron clamped to the edge).  sh_range: per degree; the
    other arguments are scene.json's."""
    from .texture_export import BakedScene, _empty_baked_bank, _import_planes
    meshes = list(meshes)
    K = len(meshes)
    D = len({d for _, d in planes})
    if set(planes) != {(s, d) for s in range(K) for d in range(D)}:
        raise _lib.VolsurfsHipError(f"scene_from_planes: planes of {sorted(planes)} for {K} meshes")
    res = [int(planes[(0, d)].shape[1]) for d in range(D)]
    for (s, d), p in planes.items():
        if p.dtype != torch.uint8 or tuple(p.shape) != (2 * d + 1, res[d], res[d], 4):
            raise _lib.VolsurfsHipError(f"scene_from_planes: plane {(s, d)} is {p.dtype} {tuple(p.shape)}, expected "
                                        f"uint8 {(2 * d + 1, res[d], res[d], 4)}")
    flat = torch.cat([planes[(s, d)].reshape(-1) for s in range(K) for d in range(D)])
    bank = _empty_baked_bank(K, D, res, [float(r) for r in sh_range][:D], bool(inner_solid), bool(shared_alpha),
                             bool(with_alpha_decay), bool(lerp), flat.device)
    _import_planes(bank, flat)
    return BakedScene(meshes, bank, tuple(float(v) for v in bg_color), cameras or {}, tuple(resolution), builder)


@torch.no_grad()
def scene_like(src, meshes, planes, builder="device"):
    """`scene_from_planes(meshes, planes)` with everything else taken from the baked scene `src`: sh ranges,
    inner_solid, shared_alpha, lerp, alpha decay, background colour (white when it has none), cameras and resolution."""
    bank, bg = src.baked, src.bg_color
    return scene_from_planes(
        meshes, planes, [-float(bank.plan.sh_lo[d]) for d in range(bank.D)], bool(bank.plan.inner_solid),
        bool(bank.shared_alpha), not bank.anchor, bool(bank.plan.with_alpha_decay),
        (1.0, 1.0, 1.0) if bg is None else bg.flatten().tolist(), getattr(src, "cameras", None),
        getattr(src, "resolution", None) or (800, 800), builder)


@torch.no_grad()
def transfer_scene(src, dst_meshes, textures_res=None, samples=1, reach=1.5, max_distance=math.inf,
                   builder="device", return_reports=False):
    """`transfer_planes` as a `BakedScene` of `dst_meshes` (its tracer built with `builder`): renders through
    `render_baked*` like a loaded scene.  Background colour, cameras, resolution, lerp and with_alpha_decay are the
    source's.  With `return_reports` also the reports."""
    planes, reports = transfer_planes(src, dst_meshes, textures_res, samples, reach, max_distance, builder)
    scene = scene_like(src, dst_meshes, planes, builder)
    return (scene, reports) if return_reports else scene


@torch.no_grad()
def make_lod(src, ratio, textures_res=None, padding=4, samples=1, anchor_shell=None, builder="device", reach=1.5,
             max_distance=math.inf, refit=None, charts="box", min_cos=0.5):
    """(scene, report): a lighter copy of a baked scene.  `simplify_shells` of the source's meshes to `ratio` of their
    faces (guarded: a nested stack stays nested; a single shell goes through `simplify_mesh`), `compute_atlas` of every
    result at the finest destination resolution with `padding`, then `transfer_scene`.
    report: {"simplify": the ShellSimplifyReports (None for one shell), "atlas": [stats per shell], "transfer":
    {(shell, degree): ...}, "faces": [faces per shell]}.
    refit: None, or a dict of `texture_fit.refit_lod`'s arguments: the transferred textures are then fitted to renders
    of the source (the returned scene is the fitted one) and the report gains "refit", the `FitReport`.
    charts, min_cos: `compute_atlas`'s chart mode ("merged": fewer, plane-projected charts; the atlas stats then carry
    `groups`)."""
    from .atlas import compute_atlas
    from .simplify import simplify_mesh, simplify_shells
    from .texture_export import baked_bank_of
    bank = baked_bank_of(src, "make_lod")
    _check_options(samples, reach, max_distance)
    res = list(bank.tex_res if textures_res is None else textures_res)[:bank.D]
    bare = [TensorMesh(m.vertices, m.faces, None, device=m.vertices.device) for m in src.tensor_meshes]
    if len(bare) >= 2:
        simple, simplify_reports = simplify_shells(bare, ratio, anchor=anchor_shell, builder=builder)
    else:
        simple, simplify_reports = [simplify_mesh(bare[0], ratio)], None
    atlased, atlas_stats = [], []
    for m in simple:
        out, st = compute_atlas(m, max(res), padding, return_stats=True, charts=charts, min_cos=min_cos)
        atlased.append(out)
        atlas_stats.append(st)
    scene, reports = transfer_scene(src, atlased, res, samples, reach, max_distance, builder, return_reports=True)
    report = {"simplify": simplify_reports, "atlas": atlas_stats, "transfer": reports,
              "faces": [int(m.faces.shape[0]) for m in atlased]}
    if refit is not None:
        from .texture_fit import refit_lod
        scene, report["refit"] = refit_lod(src, scene, **dict({"builder": builder}, **refit))
    return scene, report


@torch.no_grad()
def lod_chain(src, ratios, out_dir, textures_res=None, padding=4, samples=1, anchor_shell=None, builder="device",
              cameras=None, compress_level=6, refit=None, charts="box", min_cos=0.5):
    """Writes <out_dir>/lod_0/ as the source itself and <out_dir>/lod_i/ for ratios[i - 1] (`write_scene`'s layout,
    read by `load_scene` and `VolsurfsRenderer.from_scene`).  Every level is made from the SOURCE, not from the level
    before it, so that resampling errors do not compound.  refit, charts, min_cos: as `make_lod`'s, for every level.
    Returns the list of `make_lod`'s reports (None for lod_0)."""
    from .texture_export import write_scene
    write_scene(src, os.path.join(out_dir, "lod_0"), cameras=cameras, compress_level=compress_level)
    reports = [None]
    for i, ratio in enumerate(ratios, 1):
        scene, report = make_lod(src, ratio, textures_res, padding, samples, anchor_shell, builder, refit=refit,
                                 charts=charts, min_cos=min_cos)
        write_scene(scene, os.path.join(out_dir, f"lod_{i}"), cameras=cameras, compress_level=compress_level)
        reports.append(report)
    return reports


__all__ = ["texel_owners", "transfer_planes", "transfer_scene", "scene_from_planes", "scene_like", "make_lod",
           "lod_chain"]
