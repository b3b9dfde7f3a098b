"""The texture-transfer rule (include/volsurfs_hip.h "Texture transfer") restated in numpy, written from the
rule: every quantity in float32, one rounding per operation, in the device's order (the build compiles without
contraction); ownership and the closest source point by brute force over every face / record; the report's sums in
float64 in the rule's shape.  The yardstick of tests/test_texture_transfer.py."""
import numpy as np

import mesh_distance_restated as MD
from uv_raster_restated import covers as raster_covers   # the rasterizer's rule ("UV atlas", raster)

F32, F16 = np.float32, np.float16
TILE = 8
UNOWNED = np.uint64(0xFFFFFFFFFFFFFFFF)


def f16(x):
    return np.asarray(x, F32).astype(F16).astype(F32)


def expand_lut(sh_lo, sh_span):
    """[256] float32: fp16(sh_lo + fp16(sh_span * fp16(q / 255)))."""
    q = np.arange(256, dtype=F32)
    o = f16(q / F32(255.0))
    t = f16(F32(sh_span) * o)
    return f16(F32(sh_lo) + t)


def nearest_byte(lut, x):
    """The lowest q with the smallest |lut[q] - x| (one float32 subtract), for every x."""
    x = np.asarray(x, F32)
    d = np.abs(lut.reshape((256,) + (1,) * x.ndim) - x[None])
    assert d.dtype == F32
    return d.argmin(axis=0).astype(np.uint8)          # argmin: the first of equal minima


def texel_centre_uv(r, c, R):
    """uv at which the baked shade reads pixel (r, c) of a plane with both lerp fractions zero."""
    return (F32(c) + F32(0.5)) / F32(R), (F32(r) + F32(0.5)) / F32(R)


def uv_records(faces_uvs, R):
    """[F, 12] float32: the uv triangles in texel units as records with z = 0."""
    uv = np.asarray(faces_uvs, F32).reshape(-1, 3, 2)
    with np.errstate(all="ignore"):
        t = uv * F32(R)
        rec = np.zeros((uv.shape[0], 12), F32)
        rec[:, 0:2] = t[:, 0]
        rec[:, 4:6] = t[:, 1] - t[:, 0]
        rec[:, 8:10] = t[:, 2] - t[:, 0]
    return rec


def project(qx, qy, rec):
    """(d2, u, v) [N, T]: closest_on_triangle of the points (qx, qy, 0) on every record; d2 = 0 where the chain ends in
    the interior region.  The chain is written out once more (tests pin it to MD.closest_on_triangles)."""
    px, py = np.asarray(qx, F32).reshape(-1, 1), np.asarray(qy, F32).reshape(-1, 1)
    t = np.asarray(rec, F32).reshape(-1, 12)
    v0x, v0y = t[None, :, 0], t[None, :, 1]
    e1x, e1y, e2x, e2y = t[None, :, 4], t[None, :, 5], t[None, :, 8], t[None, :, 9]
    zero, one = F32(0.0), F32(1.0)

    def dot(ax, ay, bx, by):                          # dot3 with both z = 0: (ax bx + ay by) + 0
        return (ax * bx + ay * by) + zero

    with np.errstate(all="ignore"):
        ax, ay = px - v0x, py - v0y
        d1, d2 = dot(e1x, e1y, ax, ay), dot(e2x, e2y, ax, ay)
        bx, by = ax - e1x, ay - e1y
        d3, d4 = dot(e1x, e1y, bx, by), dot(e2x, e2y, bx, by)
        cx, cy = ax - e2x, ay - e2y
        d5, d6 = dot(e1x, e1y, cx, cy), dot(e2x, e2y, cx, cy)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        den_ab, den_ac = d1 - d3, d2 - d6
        t43, t56 = d4 - d3, d5 - d6
        den_bc = t43 + t56
        total = (va + vb) + vc
        inv = one / total
        v_bc = t43 / den_bc
        regions = [
            ((d1 <= zero) & (d2 <= zero), zero, zero),
            ((d3 >= zero) & (d4 <= d3), one, zero),
            ((vc <= zero) & (d1 >= zero) & (d3 <= zero) & (den_ab > zero), d1 / den_ab, zero),
            ((d6 >= zero) & (d5 <= d6), zero, one),
            ((vb <= zero) & (d2 >= zero) & (d6 <= zero) & (den_ac > zero), zero, d2 / den_ac),
            ((va <= zero) & (t43 >= zero) & (t56 >= zero) & (den_bc > zero), one - v_bc, v_bc),
            (total > zero, vb * inv, vc * inv),
        ]
        u = np.zeros(d1.shape, F32)
        v = np.zeros(d1.shape, F32)
        interior = np.zeros(d1.shape, bool)
        for k, (cond, ru, rv) in reversed(list(enumerate(regions))):
            u = np.where(cond, ru, u).astype(F32)
            v = np.where(cond, rv, v).astype(F32)
            interior = np.where(cond, k == 6, interior)
        rx = (ax - u * e1x) - v * e2x
        ry = (ay - u * e1y) - v * e2y
        dd = (rx * rx + ry * ry) + zero
        dd = np.where(interior, zero, dd).astype(F32)
    return dd, u, v


OUTSIDE = np.uint64(1) << np.uint64(63)


def face_records(vertices, faces):
    """[F, 12] float32: (v0, e1 = v1 - v0, e2 = v2 - v0) of the destination faces."""
    V, F = np.asarray(vertices, F32), np.asarray(faces, np.int64)
    rec = np.zeros((F.shape[0], 12), F32)
    with np.errstate(all="ignore"):
        rec[:, 0:3] = V[F[:, 0]]
        rec[:, 4:7] = V[F[:, 1]] - V[F[:, 0]]
        rec[:, 8:11] = V[F[:, 2]] - V[F[:, 0]]
    return rec


def texel_owners(faces_uvs, R, reach=1.5, recs=None):
    """{face [R, R] int32 (-1: unowned), bary [R, R, 2], d2 [R, R] (+inf: unowned), key [R, R] uint64}: a face is a
    candidate where the rasterizer's rule says it covers the texel (d2 = 0 then) or where the projection's d2 <= reach^2;
    the owner is the minimum over (not covered by the raster, d2 bits, face id); a face with a uv (or, given recs, a
    vertex) that is not finite is a candidate of nothing."""
    uv = np.asarray(faces_uvs, F32).reshape(-1, 3, 2)
    ok = np.isfinite(uv).all(axis=(1, 2))
    if recs is not None:
        ok &= np.isfinite(np.asarray(recs, F32).reshape(-1, 3, 4)[:, :, :3]).all(axis=(1, 2))
    rec = uv_records(uv, R)
    r, c = np.divmod(np.arange(R * R), R)
    qx, qy = c.astype(F32) + F32(0.5), r.astype(F32) + F32(0.5)
    reach2 = F32(reach) * F32(reach)
    key = np.full(R * R, UNOWNED, np.uint64)
    bu, bv = np.zeros(R * R, F32), np.zeros(R * R, F32)
    ids = np.arange(uv.shape[0], dtype=np.uint64)
    for s in range(0, R * R, 1024):
        dd, u, v = project(qx[s:s + 1024], qy[s:s + 1024], rec)
        covers = raster_covers(uv, R, c[s:s + 1024], r[s:s + 1024]) & ok[None, :]
        with np.errstate(all="ignore"):
            cand = (covers | (dd <= reach2)) & ok[None, :]
        k = OUTSIDE | (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None, :]
        k = np.where(covers, ids[None, :], k)                      # covered by the raster: first, with d2 = 0
        k = np.where(cand, k, UNOWNED)
        best = k.argmin(axis=1)
        rows = np.arange(k.shape[0])
        key[s:s + 1024] = k[rows, best]
        bu[s:s + 1024], bv[s:s + 1024] = u[rows, best], v[rows, best]
    owned = key != UNOWNED
    face = np.where(owned, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    bits = ((key >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).astype(np.uint32)
    d2 = np.where(owned, bits.view(F32), F32(np.inf)).astype(F32)
    bary = np.stack([np.where(owned, bu, 0), np.where(owned, bv, 0)], -1).astype(F32)
    return {"face": face.reshape(R, R), "bary": bary.reshape(R, R, 2), "d2": d2.reshape(R, R), "key": key.reshape(R, R)}


def interp_uv(fuv, bu, bv):
    """nt_interp_uv: fuv [N, 6], weights of the second and third corner."""
    one = F32(1.0)
    b0 = (one - bu) - bv
    return (b0 * fuv[:, 0] + bu * fuv[:, 2]) + bv * fuv[:, 4], (b0 * fuv[:, 1] + bu * fuv[:, 3]) + bv * fuv[:, 5]


def footprint(u, v, R, anchor):
    """nt_footprint: (i0, j0 int64, fx, fy float32)."""
    Rf = F32(R)
    a, b = u * Rf, v * Rf
    if anchor:
        i0 = (R - 1) - np.clip(np.floor(b).astype(np.int64), 0, R - 1)
        j0 = np.clip(np.floor(a).astype(np.int64), 0, R - 1)
        return i0, j0, np.zeros(a.shape, F32), np.zeros(a.shape, F32)
    ap, bp = Rf - b, a
    half = F32(0.5)
    flx, fly = np.floor(ap - half), np.floor(bp - half)
    fx, fy = ap - (flx + half), bp - (fly + half)
    return np.clip(flx.astype(np.int64), -1, R - 1), np.clip(fly.astype(np.int64), -1, R - 1), fx, fy


def fetch(plane, lut, u, v, anchor):
    """[N, n, 4] float32: the fp16 coefficients the rule fetches from plane [n, R, R, 4] (uint8) at source uvs."""
    R = plane.shape[1]
    i0, j0, fx, fy = footprint(u, v, R, anchor)
    step = 0 if anchor else 1
    one = F32(1.0)
    acc = np.zeros((u.shape[0], plane.shape[0], 4), F32)
    for ky in (0, 1):
        for kx in (0, 1):
            ix = np.clip(i0 + kx * step, 0, R - 1)
            iy = np.clip(j0 + ky * step, 0, R - 1)
            w = (fx if kx else one - fx) * (fy if ky else one - fy)
            byte = plane[:, R - 1 - ix, iy, :]                     # [n, N, 4]
            acc = acc + lut[byte.transpose(1, 0, 2)] * w[:, None, None]
    assert acc.dtype == F32
    return f16(acc)


def wave_sum(x):
    """The butterfly of 64 float64 lanes: s += s[lane ^ m], m = 32 .. 1; lane 0's value."""
    s = np.asarray(x, np.float64).copy()
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[lanes ^ m]
    return s[0]


def ordered_sum(partials):
    """vsa_surface_distance's shape: lane t of 1024 adds [t c, (t + 1) c) in order, lane 0 adds the 1024 sums."""
    p = np.asarray(partials, np.float64)
    n = p.size
    c = -(-n // 1024)
    total = np.float64(0.0)
    for t in range(1024):
        s = np.float64(0.0)
        for w in range(t * c, min((t + 1) * c, n)):
            s = s + p[w]
        total = total + s
    return total


def transfer_shell_degree(src_tris, src_face_uvs, plane, sh_lo, sh_span, anchor, has_alpha, dst_vertices, dst_faces,
                          dst_faces_uvs, R2, samples=1, reach=1.5, max_distance=np.inf):
    """One (shell, degree): (bytes [n, R2, R2, 4] uint8, report dict).  src_tris [T, 12] / src_face_uvs [T, 6]: the
    source shell's records and per-slot uvs; plane [n, R, R, 4]: its images of this degree."""
    n = plane.shape[0]
    lut = expand_lut(sh_lo, sh_span)
    recs = face_records(dst_vertices, dst_faces)
    own = texel_owners(dst_faces_uvs, R2, reach, recs)
    uvrec = uv_records(dst_faces_uvs, R2)
    owned = own["face"].reshape(-1) >= 0
    idx = np.nonzero(owned)[0]
    r, c = np.divmod(idx, R2)
    f = own["face"].reshape(-1)[idx]
    S = int(samples)
    Sf, half = F32(S), F32(0.5)
    total = np.zeros((idx.size, n, 4), F32)
    lane_s2 = np.zeros(R2 * R2, np.float64)
    far, dmax = 0, F32(0.0)
    for b in range(S):
        for a in range(S):
            qx = (c.astype(F32) + half) + ((F32(a) + half) / Sf - half)
            qy = (r.astype(F32) + half) + ((F32(b) + half) / Sf - half)
            _, bu, bv = project_rows(qx, qy, uvrec[f])             # each point on its own owner's record
            rec = recs[f]
            p = (rec[:, 0:3] + bu[:, None] * rec[:, 4:7]) + bv[:, None] * rec[:, 8:11]
            assert p.dtype == F32
            hit = MD.closest(p, src_tris)
            d = hit["dist"]
            lane_s2[idx] = lane_s2[idx] + hit["d2"].astype(np.float64)
            dmax = max(dmax, d.max()) if d.size else dmax
            far += int((d > F32(max_distance)).sum())
            su, sv = interp_uv(np.asarray(src_face_uvs, F32).reshape(-1, 6)[hit["slot"]], hit["u"], hit["v"])
            total = total + fetch(plane, lut, su, sv, anchor)
    x = total * (F32(1.0) / (Sf * Sf))
    q = nearest_byte(lut, x)
    out = np.zeros((n, R2, R2, 4), np.uint8)
    if not has_alpha:
        out[..., 3] = 255
        q[..., 3] = 255
    out[:, r, c, :] = q.transpose(1, 0, 2)
    tiles_x = -(-R2 // TILE)
    partials = []
    grid = np.zeros((tiles_x * TILE, tiles_x * TILE), np.float64)
    grid[:R2, :R2] = lane_s2.reshape(R2, R2)
    for ty in range(tiles_x):
        for tx in range(tiles_x):
            partials.append(wave_sum(grid[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].reshape(64)))
    report = {"texels": R2 * R2, "owned": int(owned.sum()), "covered": int((own["d2"] == 0).sum()),
              "samples": int(owned.sum()) * S * S, "max_distance": float(dmax), "far": far,
              "sum_d2": float(ordered_sum(partials))}
    return out, report


def project_rows(qx, qy, rec):
    """`project` of point k on record k alone, (d2, u, v) [N]: the diagonal of `project`, in blocks that keep the
    square small."""
    N = qx.shape[0]
    dd, u, v = np.empty(N, F32), np.empty(N, F32), np.empty(N, F32)
    for s in range(0, N, 256):
        sl = slice(s, s + 256)
        a, b, c = project(qx[sl], qy[sl], rec[sl])
        k = np.arange(a.shape[0])
        dd[sl], u[sl], v[sl] = a[k, k], b[k, k], c[k, k]
    return dd, u, v
