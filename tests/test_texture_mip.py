"""Texture mips (`volsurfs_amd.texture_mip`, csrc/texture_mip.hip): the mip chain of a baked scene and the baked shade that
picks each degree's level from the pixel's footprint (include/volsurfs_hip.h "Texture mips"), against the
numpy restatement tests/texture_mip_restated.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import texture_mip_restated as TM
from texture_scene_cases import RENDER_KEYS, SH_RANGE
from texture_scene_cases import camera as _camera
from texture_scene_cases import constant_planes as _constant_planes
from texture_scene_cases import random_planes as _random_planes
from texture_scene_cases import scene as _scene
from texture_scene_cases import stack as _stack

RES = (64, 32, 16)                  # per-degree grids differ: the degrees of one hit land on different levels
LEVELS = 2
# Eyes on the z axis looking at the origin, focal 60 px at 64 x 64: the footprint of the outer shell's (r = 0.7) nearest
# point is about 0.2 t^2 texels of the 64^2 degree, a quarter and a sixteenth of that for the 32^2 and 16^2 degrees, so
# these distances put hits on every level 0..2 of some degree, in between, and above the top.
EYES = ((0.0, 0.0, -2.5), (0.0, 0.0, -5.0), (0.0, 0.0, -9.0), (0.0, 0.0, -20.0))
NEAR_EYE, NEAR_FOCAL = (0.0, 0.3, -1.5), 400.0
FAR_EYE = (0.0, 0.0, -6.0)


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU

def test_restated_constant_planes_stay_constant():
    rng = np.random.default_rng(0)
    img = np.empty((3, 16, 16, 4), np.uint8)
    img[:] = np.array([7, 130, 255, 0], np.uint8)
    cover = rng.random((16, 16)) < 0.4
    for c in (None, cover):
        cur, cv = img, c
        for _ in range(4):
            cur, cv = TM.reduce_image(cur, cv)
            assert (cur == img[:, :1, :1]).all()
    assert cur.shape == (3, 1, 1, 4)


def test_restated_block_rounding_by_covered_children():
    block = np.array([[[10, 0, 255, 1], [11, 0, 255, 2]], [[13, 1, 254, 4], [200, 3, 0, 8]]], np.uint8)   # [2, 2, 4]
    a, b, c, d = (block[r, k].astype(int) for r in (0, 1) for k in (0, 1))

    def mean(vals):                       # the mean with halves rounded up, in exact integers
        n = len(vals)
        return (2 * sum(vals) + n) // (2 * n)
    cases = {(): [a, b, c, d], ((0, 0),): [a], ((0, 1), (1, 1)): [b, d], ((0, 0), (0, 1), (1, 0)): [a, b, c],
             ((0, 0), (0, 1), (1, 0), (1, 1)): [a, b, c, d]}
    for covered, vals in cases.items():
        cover = np.zeros((2, 2), bool)
        for rc in covered:
            cover[rc] = True
        out, any_ = TM.reduce_image(block[None], cover)
        assert out.shape == (1, 1, 1, 4) and bool(any_[0, 0]) == bool(covered)
        assert out[0, 0, 0].tolist() == mean(vals).tolist(), covered
    # halves round up: (1 + 2) / 2 -> 2, (0 + 1 + 1) / 3 -> 1 (0.67), (0 + 0 + 1) / 3 -> 0 (0.33), 255 stays 255
    two = np.array([[[1, 0, 0, 255], [2, 1, 0, 255]], [[9, 1, 1, 255], [9, 9, 9, 9]]], np.uint8)
    out, _ = TM.reduce_image(two[None], np.array([[1, 1], [1, 0]], bool))
    assert out[0, 0, 0].tolist() == [4, 1, 0, 255]
    out, _ = TM.reduce_image(two[None], np.array([[1, 1], [0, 0]], bool))
    assert out[0, 0, 0].tolist() == [2, 1, 0, 255]


def test_restated_mask_is_the_or_of_its_children():
    rng = np.random.default_rng(1)
    cover = rng.random((32, 32)) < 0.15
    planes = {(0, 0): rng.integers(0, 256, (1, 32, 32, 4), dtype=np.uint8)}
    chain = TM.mip_chain(planes, 5, {(0, 0): cover})
    for l in range(1, 6):
        R = 32 >> l
        below = np.asarray(chain[l - 1][1][(0, 0)]).reshape(R, 2, R, 2)
        assert (chain[l][1][(0, 0)] == below.any((1, 3))).all()
        assert chain[l][0][(0, 0)].shape == (1, R, R, 4)
    assert chain[5][1][(0, 0)].all()


def test_restated_level_rule():
    A = np.array([0.0, 0.5, np.nan, 1.0, 2.5, 3.9999998, 4.0, 15.0, 16.0, 63.0, 64.0, 1e30, np.inf], np.float32)
    l, f = TM.level_of(A, 3)
    assert l.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 3]
    assert f[:4].tolist() == [0, 0, 0, 0] and f[6] == 0 and f[8] == 0 and (f[10:] == 0).all()
    assert f[4] == np.float32(1.5) * np.float32(0.333333343) and 0.99 < f[5] < 1 and 0.9 < f[7] < 1 and 0.9 < f[9] < 1


def test_cabi_argument_errors_return_before_any_hip_call():
    from volsurfs_amd import _lib
    from volsurfs_amd.neural_textures import Plan
    L = _lib.lib()
    ERR_ARG, ERR_UNSUPPORTED = -1, -2
    buf = (ctypes.c_char * 4096)()
    a16 = (ctypes.addressof(buf) + 15) & ~15                    # 16-byte aligned host addresses: never dereferenced
    b16 = a16 + 1024
    plan = Plan()
    plan.nr_shells, plan.rgb_degrees, plan.alpha_degrees = 2, 2, 2
    plan.tex_res[0], plan.tex_res[1] = 16, 8
    total = 2 * (4 * 16 * 16 + 3 * 4 * 8 * 8)
    assert L.vsa_texmip_planes_bytes(ctypes.byref(plan), 0) == total
    assert L.vsa_texmip_planes_bytes(ctypes.byref(plan), 3) == total >> 6
    assert L.vsa_texmip_planes_bytes(ctypes.byref(plan), 4) == ERR_ARG          # 8 is not divisible by 16
    assert L.vsa_texmip_planes_bytes(None, 1) == ERR_ARG

    def reduce(plan=ctypes.byref(plan), level=1, src=a16, src_bytes=total, scov=None, dst=b16, dst_bytes=total >> 2,
               dcov=None):
        return L.vsa_texmip_reduce(plan, level, src, src_bytes, scov, dst, dst_bytes, dcov, None)
    assert reduce(plan=None) == ERR_ARG
    assert reduce(src=None) == ERR_ARG and reduce(dst=None) == ERR_ARG and reduce(dst=a16) == ERR_ARG
    assert reduce(src=a16 + 4) == ERR_ARG and reduce(dst=b16 + 8) == ERR_ARG                 # misaligned
    assert reduce(scov=a16 + 1) == ERR_ARG and reduce(dcov=b16 + 2) == ERR_ARG
    assert reduce(level=0) == ERR_ARG and reduce(level=9) == ERR_ARG and reduce(level=-1) == ERR_ARG
    assert reduce(level=4, src_bytes=total >> 6, dst_bytes=total >> 8) == ERR_ARG            # 8 % 2^4
    assert reduce(src_bytes=total - 4) == ERR_ARG and reduce(dst_bytes=total) == ERR_ARG     # wrong planes_bytes
    assert reduce(level=2, src_bytes=total, dst_bytes=total >> 4) == ERR_ARG                  # level 2 reads level 1
    plan.tex_res[1] = 12
    assert reduce(src_bytes=2 * (4 * 256 + 12 * 144), dst_bytes=2 * (4 * 64 + 12 * 36), level=3) == ERR_ARG   # 12 % 8
    plan.tex_res[1] = 0
    assert reduce() == ERR_ARG
    plan.tex_res[1] = 8
    plan.nr_shells = 17
    assert reduce() == ERR_ARG
    plan.nr_shells, plan.alpha_degrees = 2, 1
    assert reduce() == ERR_UNSUPPORTED
    plan.alpha_degrees, plan.row_format = 2, 1
    assert reduce() == ERR_UNSUPPORTED
    plan.row_format = 0

    dens = L.vsa_texmip_density
    assert dens(None, a16, 4, a16, None) == ERR_ARG and dens(a16, None, 4, a16, None) == ERR_ARG
    assert dens(a16, a16, 4, None, None) == ERR_ARG and dens(a16, a16, 0, a16, None) == ERR_ARG
    assert dens(a16 + 4, a16, 4, a16, None) == ERR_ARG and dens(a16, a16, 4, a16 + 8, None) == ERR_ARG

    levels = (ctypes.c_void_p * 8)(*([b16] * 8))

    def shade(plan=ctypes.byref(plan), hit_slot=a16, texels=a16, n=64, hit_t=a16, density=a16, spread2=1e-4, L_=3,
              lv=levels, rgb=a16, lod=None):
        return L.vsa_nt_shade_mip_fwd(plan, hit_slot, a16, a16, a16, a16, a16, texels, n, hit_t, density, spread2, L_,
                                      lv, rgb, a16, None, None, lod, None)
    assert shade(plan=None) == ERR_ARG
    assert shade(hit_slot=None) == ERR_ARG and shade(texels=None) == ERR_ARG and shade(hit_t=None) == ERR_ARG
    assert shade(density=None) == ERR_ARG and shade(lv=None) == ERR_ARG and shade(rgb=None) == ERR_ARG
    assert shade(texels=a16 + 4) == ERR_ARG and shade(hit_t=a16 + 4) == ERR_ARG and shade(lod=a16 + 8) == ERR_ARG
    assert shade(L_=0) == ERR_ARG and shade(L_=9) == ERR_ARG
    assert shade(L_=4) == ERR_ARG                                                             # 8 % 2^4
    assert shade(lv=(ctypes.c_void_p * 8)(b16, None, b16)) == ERR_ARG                         # a level without planes
    assert shade(lv=(ctypes.c_void_p * 8)(b16, b16 + 4, b16)) == ERR_ARG
    assert shade(n=-1) == ERR_ARG
    assert shade(spread2=-1.0) == ERR_ARG and shade(spread2=float("nan")) == ERR_ARG
    assert shade(spread2=float("inf")) == ERR_ARG
    assert shade(n=0) == 0                                                                    # nothing to do, no launch
    plan.alpha_degrees = 1
    assert shade() == ERR_UNSUPPORTED
    plan.alpha_degrees, plan.row_format = 2, 2
    assert shade() == ERR_UNSUPPORTED


def test_host_argument_errors():
    from volsurfs_amd import texture_mip
    assert texture_mip.default_levels((2048, 1024, 512, 256)) == 4
    assert texture_mip.default_levels((64, 32, 24)) == 3 and texture_mip.default_levels((6, 2)) == 1
    with pytest.raises(ValueError):
        texture_mip.default_levels((64, 33))
    for bad in (0, 9, 1.5, True):
        with pytest.raises(ValueError):
            texture_mip._check_levels(bad, (64,))
    with pytest.raises(ValueError):
        texture_mip._check_levels(3, (64, 36))


# ---------------------------------------------------------------------------------------------------------------------
# GPU

def _np_planes(planes):
    return {k: v.cpu().numpy() for k, v in planes.items()}


def _flat(planes, K, D):
    return torch.cat([planes[(s, d)].reshape(-1) for s in range(K) for d in range(D)]).contiguous()


def _plan_of(scene):
    bank = scene.baked
    K = bank.K
    solid, shared = bool(bank.plan.inner_solid), bool(bank.shared_alpha)
    return {"K": K, "D": bank.D, "res": [int(r) for r in bank.tex_res[:bank.D]],
            "sh_lo": [float(bank.plan.sh_lo[d]) for d in range(bank.D)],
            "sh_span": [float(bank.plan.sh_span[d]) for d in range(bank.D)], "anchor": bool(bank.anchor),
            "has_alpha": [not (solid and (s == 0 or shared)) for s in range(K)]}


@functools.lru_cache(maxsize=None)
def _random_scene(lerp=True, solid=False):
    """(scene with its chain, numpy planes): random bytes on the 320-face stack, coverage by owners."""
    meshes = _stack(2, 64, K=3)
    planes = _random_planes(3, RES, seed=5, solid=solid)
    scene = _scene(meshes, planes, lerp=lerp, solid=solid)
    scene.build_mips(levels=LEVELS)
    return scene, _np_planes(planes)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["masked", "masked-solid", "no-mask", "to-one-texel"])
def test_reduce_equals_the_restatement(case):
    from volsurfs_amd.texture_mip import mip_planes
    from volsurfs_amd.texture_export import plane_layout, plane_views
    # (32, 24, 8) over three levels: rows of 16 .. 4 texels go two texels per lane, the 24 -> 12 -> 6 -> 3 degree ends
    # on odd rows (one texel per lane).  (2, 8, 16) over one level: 2 -> 1 texel, and the degrees behind it start 4 bytes
    # into the buffer, where no 8-byte store is aligned.
    K, res = 2, {"to-one-texel": (2, 8, 16)}.get(case, (32, 24, 8))
    D, L = len(res), {"to-one-texel": 1}.get(case, 3)
    planes = _random_planes(K, res, seed=11, solid=case == "masked-solid")
    g = torch.Generator().manual_seed(3)
    cover = None if case == "no-mask" else {(s, d): (torch.rand(res[d], res[d], generator=g) < 0.3).to(torch.uint8).cuda()
                                            for s in range(K) for d in range(D)}
    flat_cover = None if cover is None else torch.cat([cover[(s, d)].reshape(-1) for s in range(K) for d in range(D)])
    level_planes, level_covers = mip_planes(_flat(planes, K, D), res, K, D, L, flat_cover)
    want = TM.mip_chain(_np_planes(planes), L, None if cover is None else _np_planes(cover))
    for l in range(1, L + 1):
        rl = [r >> l for r in res]
        got = plane_views(level_planes[l], plane_layout(rl, K, D)[0])
        off = 0
        for s in range(K):
            for d in range(D):
                assert np.array_equal(got[(s, d)].cpu().numpy(), want[l][0][(s, d)]), (case, l, s, d)
                if cover is not None:
                    m = level_covers[l][off:off + rl[d] ** 2].reshape(rl[d], rl[d]).cpu().numpy()
                    assert np.array_equal(m != 0, want[l][1][(s, d)]), (case, l, s, d)
                    off += rl[d] ** 2
        if case == "masked-solid":
            assert (got[(0, 0)][..., 3] == 255).all()             # the alpha of a shell without an alpha model


@pytest.mark.gpu
def test_reduce_down_to_one_texel():
    from volsurfs_amd.texture_mip import mip_planes
    res, K, D, L = (16, 8), 1, 2, 3
    planes = _random_planes(K, res, seed=2)
    level_planes, _ = mip_planes(_flat(planes, K, D), res, K, D, L)
    want = TM.mip_chain(_np_planes(planes), L)
    assert level_planes[3].numel() == 4 * 4 + 3 * 4
    assert np.array_equal(level_planes[3][:16].reshape(1, 2, 2, 4).cpu().numpy(), want[3][0][(0, 0)])
    assert np.array_equal(level_planes[3][16:].reshape(3, 1, 1, 4).cpu().numpy(), want[3][0][(0, 1)])


@pytest.mark.gpu
def test_build_mips_owner_coverage_and_density():
    from volsurfs_amd.texture_transfer import texel_owners
    scene, planes = _random_scene()
    chain = scene.mips
    assert chain.levels == LEVELS and not chain.stale(scene)
    tris, fuv = scene.raytracer.tris.cpu().numpy(), scene.face_uvs.cpu().numpy()
    assert np.array_equal(chain.slot_density.cpu().numpy().view(np.uint32), TM.density(tris, fuv).view(np.uint32))
    cover = {(s, d): (texel_owners(scene.tensor_meshes[s], RES[d], reach=1.5)[0] >= 0).cpu().numpy()
             for s in range(3) for d in range(3)}
    want = TM.mip_chain(planes, LEVELS, cover)
    for l in range(LEVELS + 1):
        got = chain.level_views(l, 3, 3)
        for i, (s, d) in enumerate((s, d) for s in range(3) for d in range(3)):
            assert np.array_equal(got[(s, d)].cpu().numpy(), want[l][0][(s, d)]), (l, s, d)
            assert chain.covered[l][i] == int(np.count_nonzero(want[l][1][(s, d)]))
    assert 0 < chain.covered[0][0] < 64 * 64                       # the atlas leaves texels no face can read


def _restated_frame(scene, planes, cam, supersample=1, cover="owners", restated_levels=None):
    """(device coeffs, lod, rgb, alpha), (restated coeffs, lod) and the hits of one camera through the trace.
    restated_levels: the levels of the restatement's chain when they are not the scene's (0: the bilinear fetch)."""
    from volsurfs_amd.camera import get_camera_rays
    from volsurfs_amd.texture_mip import shade_mip, spread2_of
    from volsurfs_amd.texture_transfer import texel_owners
    chain = scene.mips
    rays_o, rays_d, _ = get_camera_rays(cam, 1, False)
    hit_t, hit_slot, hit_uv = scene._trace_now(rays_o, rays_d)
    spread2 = spread2_of(cam, supersample)
    rgb, alpha, _, coeffs, lod = shade_mip(scene, chain, hit_t, hit_slot, hit_uv, rays_d, spread2, want_lod=True,
                                           want_coeffs=True)
    tex_uv = scene.baked.tex_uv_only(hit_slot, hit_uv, scene.face_uvs)
    K, D = scene.baked.K, scene.baked.D
    cov = None
    if cover == "owners":
        cov = {(s, d): (texel_owners(scene.tensor_meshes[s], RES[d], reach=1.5)[0] >= 0).cpu().numpy()
               for s in range(K) for d in range(D)}
    tris, fuv = scene.raytracer.tris.cpu().numpy(), scene.face_uvs.cpu().numpy()
    levels = chain.levels if restated_levels is None else restated_levels
    want = TM.shade_coefficients(TM.mip_chain(planes, levels, cov), _plan_of(scene), tris, TM.density(tris, fuv),
                                 hit_slot.cpu().numpy(), hit_t.cpu().numpy(), tex_uv.cpu().numpy(), rays_d.cpu().numpy(),
                                 np.float32(spread2))
    return (coeffs, lod, rgb, alpha), want, (hit_t, hit_slot, hit_uv, rays_d, tex_uv)


def _tail_of(scene, coeffs, hit_slot, rays_d):
    """(surfs_rgb, surfs_alpha) that vsa_nt_shade_fwd gives for per-hit fp16 SH coefficients [K, N, 64]: a bank of RAW
    f16 rows (row_format 2: a row IS the coefficient, no expansion) under anchor addressing, one texel per ray, so that
    the lerp returns fp16(0 + c * 1) = c and everything after it -- SH sum, sigmoid, alpha decay, scatter -- is the
    existing entry point's.  The restatement's coefficients get the library's own tail this way: the device's fast
    exponential has no numpy twin."""
    from volsurfs_amd.neural_textures import ALPHA_QUAD, MAX_DEG, ROW_QUADS, NeuralTextureBank
    src = scene.baked
    K, N = hit_slot.shape
    R = 64
    assert N <= R * R
    bank = NeuralTextureBank(K, NeuralTextureBank.full_capacity_rays([R] * 4), sh_degree=src.D - 1,
                             alpha_sh_degree=src.D - 1, textures_res=[R] * 4, inner_solid=bool(src.plan.inner_solid),
                             with_alpha_decay=bool(src.plan.with_alpha_decay), training=False, anchor=True, lerp=False,
                             quantize_output=False, squeeze_output=False, shared_alpha=bool(src.shared_alpha),
                             parameters=False)
    bank.compact_all(want_texel_of_slot=False)
    n = torch.arange(N, device="cuda")
    j0, i0 = n // R, n % R
    tex_uv = torch.stack([(j0 + 0.5) / R, (R - 1 - i0 + 0.5) / R], -1).float()[None].repeat(K, 1, 1).contiguous()
    seg = bank.seg_start.cpu().tolist()
    c16 = torch.as_tensor(coeffs).cuda().to(torch.float16)
    assert torch.equal(c16.float().cpu(), torch.as_tensor(coeffs))          # the coefficients are fp16 values
    for s in range(K):
        for d in range(src.D):
            sd, nn, W = s * MAX_DEG + d, 2 * d + 1, R + 2
            slots = bank.slot_of[int(bank.plan.dom_off[sd]) + (j0 + 1) * W + (i0 + 1)].long()
            e0 = (int(bank.plan.row_base[sd]) + (slots - seg[sd]) * ROW_QUADS[d]) * 4
            for ch in range(4):
                first = 4 * ALPHA_QUAD[d] if ch == 3 else ch * nn
                for i in range(nn):
                    bank.texels[e0 + first + i] = c16[s, :, ch * 16 + d * d + i]
    rgb, alpha, _, _ = bank.shade(hit_slot, tex_uv, rays_d, scene.raytracer.tris)
    return rgb, alpha


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("lerp, solid", [(True, False), (False, True)])
def test_every_level_equals_the_restatement(lerp, solid):
    scene, planes = _random_scene(lerp, solid)
    seen_l, seen_frac, seen_top, seen_graze = set(), False, False, False
    for eye in EYES:
        (coeffs, lod, rgb, alpha), (want_c, want_lod), (hit_t, hit_slot, _, rays_d, _) = _restated_frame(
            scene, planes, _camera(eye))
        # what the restatement alone shows about this distance
        hits = hit_slot.cpu().numpy() >= 0
        assert hits.any()
        wl = want_lod[hits]
        seen_l |= set(np.floor(wl).astype(int).ravel().tolist())
        seen_frac |= bool(((wl % 1) > 0).any())
        tris = scene.raytracer.tris.cpu().numpy()
        for s in range(3):
            h = np.nonzero(hits[s])[0]
            cs, _ = TM.cosine(tris, hit_slot[s].cpu().numpy()[h], rays_d.cpu().numpy()[h])
            seen_graze |= bool((cs < 0.125).any())
            A0 = TM.footprint_uv(hit_t[s].cpu().numpy()[h], 1.0 / 3600.0, scene.mips.slot_density.cpu().numpy()[
                hit_slot[s].cpu().numpy()[h]], np.fmax(cs, np.float32(0.125))) * np.float32(64.0 * 64.0)
            seen_top |= bool((A0 >= 4.0 ** (LEVELS + 1)).any())        # l0 > L: clamped to the top level
        # the device against it, bit for bit
        assert np.array_equal(lod.cpu().numpy().view(np.uint32), want_lod.view(np.uint32)), eye
        assert np.array_equal(coeffs.cpu().numpy().view(np.uint32), want_c.view(np.uint32)), eye
        want_rgb, want_alpha = _tail_of(scene, want_c, hit_slot, rays_d)
        assert torch.equal(_bits(rgb), _bits(want_rgb)) and torch.equal(_bits(alpha), _bits(want_alpha)), eye
    assert seen_l == set(range(LEVELS + 1)) and seen_frac and seen_top and seen_graze


@pytest.mark.gpu
@pytest.mark.parametrize("hits", ["trace", "raster"])
def test_magnification_is_the_bilinear_render(hits):
    scene, planes = _random_scene()
    cam = _camera(NEAR_EYE, focal=NEAR_FOCAL)
    _, (_, want_lod), (_, hit_slot, _, _, _) = _restated_frame(scene, planes, cam)
    hit = hit_slot.cpu().numpy() >= 0
    assert hit.any() and (want_lod[hit] == 0).all()                # the restatement: every hit is magnified
    a = scene.render_baked_camera(cam, hits=hits)
    b = scene.render_baked_camera(cam, hits=hits, filter="mip")
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(_bits(a[k].float()), _bits(b[k].float())), k


@pytest.mark.gpu
@pytest.mark.parametrize("solid", [False, True])
def test_constant_planes_render_the_same_bytes_at_any_distance(solid):
    from volsurfs_amd.texture_mip import hit_lod
    meshes = _stack(1, 64, K=3)
    scene = _scene(meshes, _constant_planes(3, RES, solid), solid=solid)
    scene.build_mips(levels=LEVELS, coverage=None)
    for eye in EYES[1:]:
        cam = _camera(eye)
        assert torch.nan_to_num(hit_lod(scene, cam)).max() > 0     # (not all magnified: the chain is read)
        for hits in ("trace", "raster"):
            a = scene.render_baked_camera(cam, hits=hits)
            b = scene.render_baked_camera(cam, hits=hits, filter="mip")
            for k in RENDER_KEYS:
                assert torch.equal(_bits(a[k].float()), _bits(b[k].float())), (eye, hits, k)


@pytest.mark.gpu
def test_mip_aliases_less_than_bilinear():
    """Noise planes from far away, coverage=None: against the 8 x 8 supersampled bilinear frame, one mip sample per pixel
    is closer than one bilinear sample per pixel.  The inequality only, first on the restatement's two frames (its
    coefficients -- with the chain, and with level 0 alone -- through vsa_nt_shade_fwd's tail and the composite), then
    on the device's.
    The restatement at this distance (eye 6 from the centre, the 64^2 degree at level 0.9 .. 1.4 over the disc):
    mse bilinear 1 spp 0.001075, mip 1 spp 0.000772 -- the mip frame's error is 72 % of the bilinear frame's."""
    meshes = _stack(2, 64, K=3)
    planes = _random_planes(3, RES, seed=9, no_alpha=False)
    scene = _scene(meshes, planes)
    scene.build_mips(levels=LEVELS, coverage=None)
    cam = _camera(FAR_EYE)
    target = scene.render_baked_camera(cam, supersample=8)["rgb"].float()

    def mse(frame):
        return float(((frame.float() - target) ** 2).mean())
    restated = {}
    for name, levels in (("bilinear", 0), ("mip", LEVELS)):
        _, (coeffs, _), (_, hit_slot, _, rays_d, _) = _restated_frame(scene, _np_planes(planes), cam, cover=None,
                                                                      restated_levels=levels)
        rgb_k, alpha_k = _tail_of(scene, coeffs, hit_slot, rays_d)
        restated[name] = scene._composite_baked(rgb_k, alpha_k, None)["rgb"]
    print(f"restated: mse bilinear 1 spp {mse(restated['bilinear']):.6f}, mip 1 spp {mse(restated['mip']):.6f}")
    assert mse(restated["mip"]) < mse(restated["bilinear"])
    bil = scene.render_baked_camera(cam)["rgb"]
    mip = scene.render_baked_camera(cam, filter="mip")["rgb"]
    print(f"device:   mse bilinear 1 spp {mse(bil):.6f}, mip 1 spp {mse(mip):.6f}")
    assert mse(mip) < mse(bil)
    assert torch.equal(_bits(bil.float()), _bits(restated["bilinear"].float()))
    assert torch.equal(_bits(mip.float()), _bits(restated["mip"].float()))


@pytest.mark.gpu
def test_missing_and_stale_chains_raise():
    from volsurfs_amd.texture_fit import TextureFit
    from volsurfs_amd.texture_export import _export_flat, _import_planes
    meshes = _stack(1, 64, K=3)
    scene = _scene(meshes, _random_planes(3, RES, seed=4))
    cam = _camera(EYES[1])
    with pytest.raises(ValueError, match="build_mips"):
        scene.render_baked_camera(cam, filter="mip")
    with pytest.raises(ValueError):
        scene.render_baked_camera(cam, filter="trilinear")
    scene.build_mips()
    assert scene.mips.levels == 4                                  # the largest L <= 4 that divides 64, 32, 16
    scene.render_baked_camera(cam, filter="mip")
    fit = TextureFit(scene)
    assert getattr(fit.scene, "mips", None) is None                # a fit's scene carries no chain
    with pytest.raises(ValueError, match="build_mips"):
        fit.scene.render_baked_camera(cam, filter="mip")
    flat, _ = _export_flat(scene.baked)
    _import_planes(scene.baked, flat.flip(0).contiguous())         # the bank's bytes change under the chain
    with pytest.raises(ValueError, match="stale"):
        scene.render_baked_camera(cam, filter="mip")
    scene.build_mips(levels=2)
    scene.render_baked_camera(cam, filter="mip", lod_bias=1.0)
    with pytest.raises(ValueError):
        scene.build_mips(levels=5)                                 # 16 is not divisible by 32
