"""Mip chains of baked textures and the footprint-filtered baked shade, on the device (csrc/texture_mip.hip; the rule in
include/volsurfs_hip.h "Texture mips").  The reference has no such stage: the rule is this library's own,
restated in tests/texture_mip_restated.py and unpinned.

A baked scene seen from far away puts many texels under one pixel, and the bilinear fetch of the full-resolution texture
aliases; the only remedy used to be `supersample`, at s^2 times the traces, shades and composites.  Here every SH degree
of a hit reads the level whose texels match the pixel's footprint on the surface, blended with the next one.

* `mip_planes` — levels 1..L of a plane buffer (`export_planes`' layout) and of a coverage mask, one launch per level.
* `build_mips` — the `MipChain` of a baked scene; `VolSurfs.build_mips` / `BakedScene.build_mips` keep it at `.mips`.
* `mip_shader` — the per-chunk shade that `render_baked_camera(filter="mip")` runs.
* `hit_lod` — the level + fraction of every hit of a camera, for inspection.

NOT promised: coefficients are filtered BEFORE the SH sum and the sigmoid (as the texture transfer does); the filter is
isotropic (a grazing hit is blurred along both axes, the cosine clamped at 1/8); charts closer than 2^l texels share
texels of level l, with `coverage="owners"` only through texels that no face can read.  Nothing is written to disk: the
chain is derivable, scene.json and the PNGs keep their format.  Forward only.
"""
import ctypes
import weakref

import torch

from . import _lib

MAX_LEVELS = 8               # VSA_TEXMIP_MAX_LEVELS
DEFAULT_MAX_LEVELS = 4       # build_mips(levels=None): the largest L <= 4 that divides every resolution
OWNER_REACH = 1.5            # texels: every texel a bilinear lookup on the mesh can read has an owner ("Texture transfer")


def _check_levels(levels, resolutions):
    if isinstance(levels, bool) or int(levels) != levels or not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError(f"texture mips: levels must be an integer in 1..{MAX_LEVELS}, got {levels!r}")
    L = int(levels)
    bad = [int(r) for r in resolutions if int(r) < 1 or int(r) % (1 << L)]
    if bad:
        raise ValueError(f"texture mips: resolutions {bad} are not divisible by 2^{L}")
    return L


def default_levels(resolutions):
    """The largest L <= 4 with every resolution divisible by 2^L; ValueError when there is none (an odd resolution)."""
    for L in range(DEFAULT_MAX_LEVELS, 0, -1):
        if all(int(r) >= 1 and int(r) % (1 << L) == 0 for r in resolutions):
            return L
    raise ValueError(f"texture mips: resolutions {[int(r) for r in resolutions]} allow no level (one of them is odd)")


def _plan(K, D, resolutions):
    """The plan fields the chain's entry points read, for planes that belong to no bank."""
    from .neural_textures import MAX_DEG, Plan
    p = Plan()
    p.nr_shells, p.rgb_degrees, p.alpha_degrees, p.row_format = int(K), int(D), int(D), 0
    for d in range(MAX_DEG):
        p.tex_res[d] = int(resolutions[min(d, D - 1)])
    return p


def _level_views(buf, sizes):
    """Views of one buffer, one per size, each starting on a 16-byte boundary."""
    out, off = [], 0
    for n in sizes:
        out.append(buf[off:off + n])
        off += (n + 15) // 16 * 16
    return out


def _padded(sizes):
    return sum((n + 15) // 16 * 16 for n in sizes)


@torch.no_grad()
def mip_planes(planes, resolutions, K, D, levels, cover=None):
    """(level_planes, level_covers): lists indexed by level 0..L.  planes: the flat uint8 device buffer of
    `export_planes`' layout at `resolutions` (level 0, returned as entry 0); entry l is a buffer of the same layout at
    resolutions >> l.  cover: None (every texel covered; level_covers is then None), or a flat uint8 device buffer of
    [R_d, R_d] masks ordered (shell, degree), nonzero = covered; level l's mask is the OR of its children.
    Levels 1..L live in ONE allocation each (planes, masks), level after level on 16-byte boundaries.  The same inputs
    give the same bytes."""
    K, D = int(K), int(D)
    res = [int(r) for r in resolutions][:D]
    L = _check_levels(levels, res)
    total = sum((2 * d + 1) * 4 * res[d] * res[d] for d in range(D)) * K
    ctotal = sum(r * r for r in res) * K
    if planes.dtype != torch.uint8 or planes.numel() != total or not planes.is_cuda or not planes.is_contiguous():
        raise ValueError(f"mip_planes: expected {total} contiguous uint8 plane bytes on the GPU, got {planes.numel()} of "
                         f"{planes.dtype} on {planes.device}")
    if cover is not None and (cover.dtype != torch.uint8 or cover.numel() != ctotal or not cover.is_cuda
                              or not cover.is_contiguous()):
        raise ValueError(f"mip_planes: expected {ctotal} contiguous uint8 mask bytes on the GPU")
    dev = planes.device
    sizes = [total >> (2 * l) for l in range(1, L + 1)]
    level_planes = [planes] + _level_views(torch.empty(_padded(sizes), dtype=torch.uint8, device=dev), sizes)
    level_covers = None
    if cover is not None:
        csizes = [ctotal >> (2 * l) for l in range(1, L + 1)]
        level_covers = [cover] + _level_views(torch.empty(_padded(csizes), dtype=torch.uint8, device=dev), csizes)
    plan = _plan(K, D, res)
    for l in range(1, L + 1):
        _lib.call("vsa_texmip_reduce", ctypes.byref(plan), l, level_planes[l - 1], level_planes[l - 1].numel(),
                  None if level_covers is None else level_covers[l - 1], level_planes[l], level_planes[l].numel(),
                  None if level_covers is None else level_covers[l], _lib.stream_ptr())
    return level_planes, level_covers


class _BankVersion:
    """What a chain was built from: the bank and the tracer themselves (weak references, compared by identity: an id()
    can be reused once its object is gone), the bank's texel storage, and the counter of whatever rewrites a baked
    bank's bytes (`NeuralTextureBank.texels_version`: bake_all, the plane import, a texel-fit step)."""

    def __init__(self, scene):
        bank = scene.baked
        self.bank, self.tracer = weakref.ref(bank), weakref.ref(scene.raytracer)
        self.texels = weakref.ref(bank.texels)
        self.counters = (int(bank.texels_version), bank.texels._version)

    def holds(self, scene):
        bank = scene.baked
        return (bank is not None and self.bank() is bank and self.tracer() is scene.raytracer
                and self.texels() is bank.texels and self.counters == (int(bank.texels_version), bank.texels._version))


class MipChain:
    """The mip chain of one baked scene (`build_mips`).
    levels: L.  resolutions: level 0's per-degree resolutions.  planes: [L + 1] flat uint8 buffers, planes[l] in
    `export_planes`' layout at resolutions >> l (planes[0]: the export the chain was built from; the shade reads level 0
    from the scene's own bank).  covers: the per-level masks, or None.  slot_density: f32 per slot of the scene's
    tracer, uv area per world area.  covered: [L + 1] lists of covered texels per (shell, degree) in that order.
    version: the `_BankVersion` of the scene at build time; `stale(scene)` tells whether it still holds."""

    def __init__(self, levels, resolutions, planes, covers, slot_density, covered, version):
        self.levels, self.resolutions, self.planes, self.covers = levels, list(resolutions), planes, covers
        self.slot_density, self.covered, self.version = slot_density, covered, version
        self.level_ptrs = (ctypes.c_void_p * levels)(*(p.data_ptr() for p in planes[1:]))

    def stale(self, scene):
        return not self.version.holds(scene)

    def level_views(self, level, K, D):
        """{(shell, degree): uint8 [2d+1, R, R, 4]} views of one level's planes."""
        from .texture_export import plane_layout, plane_views
        res = [r >> level for r in self.resolutions]
        return plane_views(self.planes[level], plane_layout(res, K, D)[0])


def _owner_cover(scene, res, K, D):
    """The flat mask of `mip_planes`: texel covered iff `texel_owners` gives it an owner at reach 1.5."""
    from .texture_transfer import texel_owners
    parts = []
    for s in range(K):
        for d in range(D):
            face, _, _ = texel_owners(scene.tensor_meshes[s], res[d], reach=OWNER_REACH)
            parts.append((face >= 0).to(torch.uint8).reshape(-1))
    return torch.cat(parts).contiguous()


@torch.no_grad()
def build_mips(scene, levels=None, coverage="owners"):
    """The `MipChain` of a baked scene (a `BakedScene`, or a `VolSurfs` after `bake()`); not stored (the scenes'
    `build_mips` methods store it at `.mips`).  levels: L in 1..8 with every resolution divisible by 2^L; None takes
    the largest L <= 4.  coverage="owners": a coarse texel averages only texels that some face can read (an owner within
    1.5 texels, `texture_transfer.texel_owners`); None: every texel counts, and the zero bytes outside the charts bleed
    into their edges.  One blocking read (the covered counts)."""
    from .texture_export import _export_flat, baked_bank_of
    if coverage not in ("owners", None):
        raise ValueError(f'build_mips: coverage must be "owners" or None, got {coverage!r}')
    bank = baked_bank_of(scene, "build_mips")
    K, D, res = bank.K, bank.D, [int(r) for r in bank.tex_res[:bank.D]]
    L = default_levels(res) if levels is None else _check_levels(levels, res)
    planes, _ = _export_flat(bank)
    cover = _owner_cover(scene, res, K, D) if coverage == "owners" else None
    level_planes, level_covers = mip_planes(planes, res, K, D, L, cover)
    tris = scene.raytracer.tris
    nr_slots = int(tris.shape[0])
    density = torch.empty(nr_slots, device=tris.device)
    _lib.call("vsa_texmip_density", tris, scene.face_uvs, nr_slots, density, _lib.stream_ptr())
    covered = []
    for l in range(L + 1):
        sizes = [(res[d] >> l) ** 2 for _ in range(K) for d in range(D)]
        if level_covers is None:
            covered.append(sizes)
        else:
            covered.append(torch.stack([c.ne(0).sum() for c in level_covers[l].split(sizes)]))
    if level_covers is not None:
        covered = torch.stack(covered).cpu().tolist()                  # the one blocking read
    return MipChain(L, res, level_planes, level_covers, density, covered, _BankVersion(scene))


def require_chain(scene):
    """The scene's chain, or a ValueError that names `build_mips`."""
    chain = getattr(scene, "mips", None)
    if chain is None:
        raise ValueError('filter="mip" needs a mip chain: call build_mips() on the scene first (or load it with mips=L)')
    if chain.stale(scene):
        raise ValueError('filter="mip": the mip chain is stale (the baked textures changed since build_mips()): call '
                         "build_mips() again")
    return chain


def spread2_of(camera, supersample=1, lod_bias=0.0):
    """The solid angle of one sample of a pinhole camera, 1 / (fx fy s^2), times 4^lod_bias: formed in double, handed
    to the shade as a float."""
    K = camera.intrinsics.detach().cpu().double()
    s = int(supersample)
    return float(4.0 ** float(lod_bias) / (float(K[0, 0]) * float(K[1, 1]) * s * s))


def shade_mip(scene, chain, hit_t, hit_slot, hit_uv, rays_d, spread2, want_lod=False, want_coeffs=False):
    """vsa_nt_shade_mip_fwd for these hits: (surfs_rgb [N, K, 3], surfs_alpha [N, K], normals [N, K, 3], coeffs
    [K, N, 64] | None, lod [K, N, D] | None)."""
    bank = scene.baked
    K, N = hit_slot.shape
    dev = hit_slot.device
    tex_uv = bank.tex_uv_only(hit_slot, hit_uv, scene.face_uvs)
    rgb, alpha, normals = torch.empty(N, K, 3, device=dev), torch.empty(N, K, device=dev), torch.empty(N, K, 3, device=dev)
    coeffs = torch.empty(K, N, 64, device=dev) if want_coeffs else None
    lod = torch.empty(K, N, bank.D, device=dev) if want_lod else None
    _lib.call("vsa_nt_shade_mip_fwd", ctypes.byref(bank.plan), hit_slot, tex_uv, rays_d.contiguous(),
              scene.raytracer.tris, bank.slot_of, bank.seg_start, bank.texels, N, hit_t.contiguous(), chain.slot_density,
              float(spread2), chain.levels, chain.level_ptrs, rgb, alpha, normals, coeffs, lod, _lib.stream_ptr())
    return rgb, alpha, normals, coeffs, lod


def mip_shader(scene, camera, supersample=1, lod_bias=0.0, want_lod=False):
    """The shade of `render_baked_camera(filter="mip")` for one camera: a function of a chunk of hits (hit_t, hit_slot,
    hit_uv, rays_d), as `VolSurfs._camera_hit_chunks` yields them, that returns the chunk's `ray_traced` dict (or, with
    want_lod, its lod [K, N, D]).  ValueError (naming `build_mips`) without a chain or with a stale one."""
    chain = require_chain(scene)
    spread2 = spread2_of(camera, supersample, lod_bias)

    def shade(hit_t, hit_slot, hit_uv, rays_d):
        rgb_k, alpha_k, normals, _, lod = shade_mip(scene, chain, hit_t, hit_slot, hit_uv, rays_d, spread2,
                                                    want_lod=want_lod)
        return lod if want_lod else scene._composite_baked(rgb_k, alpha_k, normals)
    return shade


@torch.no_grad()
def hit_lod(scene, camera, supersample=1, lod_bias=0.0, hits="trace"):
    """lod [K, H * W * s^2, D] f32: level + fraction per shell, sample and SH degree (NaN where the sample misses the
    shell), as the mip shade of `render_baked_camera(camera, supersample, filter="mip")` picks them."""
    from .rasterize import check_hits_mode
    s = int(supersample)
    shade = mip_shader(scene, camera, s, lod_bias, want_lod=True)
    lods = [shade(*h) for h in scene._camera_hit_chunks(camera, s, check_hits_mode(hits))]
    return lods[0] if len(lods) == 1 else torch.cat(lods, 1)


__all__ = ["MAX_LEVELS", "MipChain", "mip_planes", "build_mips", "default_levels", "require_chain", "spread2_of",
           "shade_mip", "mip_shader", "hit_lod"]
