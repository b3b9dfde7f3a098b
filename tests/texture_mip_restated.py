"""The texture-mip rule (include/volsurfs_hip.h "Texture mips") restated in numpy, written from the rule:
the chain in integers; the density, the footprint, the level and the blend in float32 with one rounding per operation in
the device's order (the build compiles without contraction; numpy's float32 sqrt and divide are IEEE, as the device's).
Nothing of the log / exp / pow family.  The yardstick of tests/test_texture_mip.py."""
import numpy as np

from texture_transfer_restated import expand_lut, f16, fetch

F32 = np.float32
THIRD = F32(0.333333343)
COS_CLAMP = F32(0.125)


# ---- the chain

def reduce_image(img, cover=None):
    """(dst [..., R/2, R/2, 4] uint8, dst_cover [R/2, R/2] bool) of img [..., R, R, 4] uint8 and cover [R, R] (None: all
    covered): per channel q = (2 sum + n) // (2 n) over the n covered children, over all four where n = 0."""
    R = img.shape[-3]
    assert R % 2 == 0 and img.shape[-2] == R and img.dtype == np.uint8
    h = R // 2
    c = img.reshape(*img.shape[:-3], h, 2, h, 2, 4).astype(np.int64)
    cv = np.ones((R, R), bool) if cover is None else np.asarray(cover) != 0
    cv = cv.reshape(h, 2, h, 2)
    n = cv.sum((1, 3))
    use = np.where((n == 0)[:, None, :, None], True, cv)
    nn = np.where(n == 0, 4, n)[..., None]
    s = (c * use[..., None]).sum((-4, -2))
    return ((2 * s + nn) // (2 * nn)).astype(np.uint8), n > 0


def mip_chain(planes, levels, cover=None):
    """[(planes, cover)] for level 0..levels.  planes: {(shell, degree): uint8 [2d+1, R, R, 4]}; cover: {(shell,
    degree): [R, R]} or None."""
    out = [(planes, cover)]
    for _ in range(levels):
        p, c = out[-1]
        np_, nc = {}, (None if c is None else {})
        for key, img in p.items():
            np_[key], m = reduce_image(img, None if c is None else c[key])
            if c is not None:
                nc[key] = m
        out.append((np_, nc))
    return out


# ---- the level of a hit

def cross_e1_e2(tris):
    """c = e1 x e2 of tracer records [S, 12] (v0.xyz, id, e1.xyz, 0, e2.xyz, 0), as vsa_nt_shade_fwd forms it."""
    e1, e2 = tris[:, 4:7].astype(F32), tris[:, 8:11].astype(F32)
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return cx, cy, cz


def density(tris, face_uvs):
    """[S] float32: uv area per world area of every slot; 0 where the world area is 0 or the quotient is not finite."""
    uv = face_uvs.astype(F32)
    du1, dv1, du2, dv2 = uv[:, 2] - uv[:, 0], uv[:, 3] - uv[:, 1], uv[:, 4] - uv[:, 0], uv[:, 5] - uv[:, 1]
    a2 = np.abs(du1 * dv2 - dv1 * du2)
    cx, cy, cz = cross_e1_e2(tris)
    with np.errstate(all="ignore"):
        a3 = np.sqrt((cx * cx + cy * cy) + cz * cz)
        q = a2 / a3
    assert q.dtype == F32
    return np.where((a3 > 0) & np.isfinite(q), q, F32(0.0)).astype(F32)


def cosine(tris, slot, rays_d):
    """(cos before the clamp, cos after it) of hits on `slot` [N] with directions rays_d [N, 3]."""
    cx, cy, cz = (c[slot] for c in cross_e1_e2(tris))
    dx, dy, dz = (rays_d[:, i].astype(F32) for i in range(3))
    nn = (cx * cx + cy * cy) + cz * cz
    dd = (dx * dx + dy * dy) + dz * dz
    nd = np.abs((cx * dx + cy * dy) + cz * dz)
    with np.errstate(all="ignore"):
        cs = nd / np.sqrt(nn * dd)
    assert cs.dtype == F32
    return cs, np.fmax(cs, COS_CLAMP)


def footprint_uv(t, spread2, dens, cos_clamped):
    """A_uv = (((t * t) * spread2) * density) / cos."""
    t = t.astype(F32)
    a = (((t * t) * F32(spread2)) * dens) / cos_clamped
    assert a.dtype == F32
    return a


def level_of(A, L):
    """(l int64, f float32) of footprints A (texels^2 of level 0) in a chain of L levels; no logarithm."""
    A = np.asarray(A, F32)
    mag = ~(A >= F32(1.0))                                   # magnification or NaN
    bits = np.where(mag, F32(1.0), A).view(np.uint32).astype(np.int64)
    l0 = ((bits >> 23) - 127) >> 1
    top = l0 >= L
    lc = np.where(top, 0, l0)
    scale = ((127 - 2 * lc) << 23).astype(np.uint32).view(F32)
    with np.errstate(all="ignore"):
        f = (np.where(mag, F32(1.0), A) * scale - F32(1.0)) * THIRD
    assert f.dtype == F32
    l = np.where(mag, 0, np.where(top, L, l0))
    f = np.where(mag | top, F32(0.0), f).astype(F32)
    return l, f


# ---- the coefficients of a call

def shade_coefficients(chain, plan, tris, dens, hit_slot, hit_t, tex_uv, rays_d, spread2):
    """(coeffs [K, N, 64] float32, lod [K, N, D] float32) of vsa_nt_shade_mip_fwd.
    chain: `mip_chain`'s list; plan: {"K", "D", "res", "sh_lo", "sh_span", "anchor", "has_alpha": [K]}.  Level 0 is
    fetched from chain[0] with the clamp-to-edge rule: a bank filled by vsa_nt_import_planes holds exactly that."""
    K, D, L = plan["K"], plan["D"], len(chain) - 1
    N = hit_slot.shape[1]
    coeffs = np.zeros((K, N, 64), F32)
    lod = np.full((K, N, D), np.nan, F32)
    for s in range(K):
        hit = np.nonzero(hit_slot[s] >= 0)[0]
        if hit.size == 0:
            continue
        slot = hit_slot[s, hit]
        _, cs = cosine(tris, slot, rays_d[hit])
        a_uv = footprint_uv(hit_t[s, hit], spread2, dens[slot], cs)
        u, v = tex_uv[s, hit, 0].astype(F32), tex_uv[s, hit, 1].astype(F32)
        for d in range(D):
            n, m0 = 2 * d + 1, d * d
            Rf = F32(plan["res"][d])
            l, f = level_of(a_uv * (Rf * Rf), L)
            lod[s, hit, d] = l.astype(F32) + f
            lut = expand_lut(plan["sh_lo"][d], plan["sh_span"][d])
            c = np.zeros((hit.size, n, 4), F32)
            for lv in range(L + 1):
                here = np.nonzero(l == lv)[0]
                if here.size == 0:
                    continue
                c0 = fetch(chain[lv][0][(s, d)], lut, u[here], v[here], plan["anchor"])
                up = here[f[here] > 0]
                if up.size:
                    # (two fetches for the blended hits: plain numpy, the clearer for it)
                    a = fetch(chain[lv][0][(s, d)], lut, u[up], v[up], plan["anchor"])
                    b = fetch(chain[lv + 1][0][(s, d)], lut, u[up], v[up], plan["anchor"])
                    fb = f[up][:, None, None]
                    blend = f16(a + fb * (b - a))
                    assert blend.dtype == F32
                    c0[np.searchsorted(here, up)] = blend
                c[here] = c0
            for ch in range(4):
                if ch == 3 and not plan["has_alpha"][s]:
                    continue
                coeffs[s, hit, ch * 16 + m0:ch * 16 + m0 + n] = c[:, :, ch]
    return coeffs, lod
