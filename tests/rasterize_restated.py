"""numpy restatement of the bin rule of csrc/shell_raster.hip (include/volsurfs_hip.h "Shell rasterization", DESIGN
§35) -- TEST INFRASTRUCTURE ONLY.  fp32 in the kernel's operation order: classification, boxes, tile lists and the four
statistics; plus the sample grid's rays (csrc/pinhole.h) and the reference hit, tri_test (csrc/trace_walk.h) over a
list of triangle records."""
import numpy as np

F32 = np.float32
TILE = 8
DROPPED, BEHIND, STRADDLING, FRONT = 0, 1, 2, 3


def records(vertices, faces):
    """Triangle records [F, 12] f32 in face order: v0.xyz, id | e1.xyz, 0 | e2.xyz, 0 (e = v1 - v0, v2 - v0 in fp32)."""
    v, f = np.asarray(vertices, F32), np.asarray(faces, np.int64)
    rec = np.zeros((f.shape[0], 12), F32)
    rec[:, 0:3] = v[f[:, 0]]
    rec[:, 3] = np.arange(f.shape[0], dtype=np.int32).view(F32)
    rec[:, 4:7] = v[f[:, 1]] - v[f[:, 0]]
    rec[:, 8:11] = v[f[:, 2]] - v[f[:, 0]]
    return rec


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def classify(tris, c2w, k, H, W, s):
    """(cls [F], box [F, 4] = tile x0, y0, x1, y1 inclusive; x0 > x1: in no tile's list)."""
    tris = np.asarray(tris, F32).reshape(-1, 12)
    c2w, k = np.asarray(c2w, F32).reshape(3, 4), np.asarray(k, F32).reshape(3, 3)
    n = tris.shape[0]
    sw, sh = W * s, H * s
    tiles_x, tiles_y = (sw + TILE - 1) // TILE, (sh + TILE - 1) // TILE
    with np.errstate(all="ignore"):
        v0, e1, e2 = tris[:, 0:3], tris[:, 4:7], tris[:, 8:11]
        verts = [v0, v0 + e1, v0 + e2]
        finite = np.ones(n, bool)
        for v in verts:
            finite &= (np.abs(v) < np.inf).all(1)
        cam = []
        for v in verts:
            w = [v[:, i] - c2w[i, 3] for i in range(3)]
            cam.append([_dot3(c2w[0, i], c2w[1, i], c2w[2, i], w[0], w[1], w[2]) for i in range(3)])
        zg = F32(1e-4) * max(F32(1.0), np.abs(c2w[:, 3]).max())
        behind = (cam[0][2] < -zg) & (cam[1][2] < -zg) & (cam[2][2] < -zg)
        front = (cam[0][2] > zg) & (cam[1][2] > zg) & (cam[2][2] > zg)
        lo_x = np.full(n, np.inf, F32)
        lo_y = np.full(n, np.inf, F32)
        hi_x = np.full(n, -np.inf, F32)
        hi_y = np.full(n, -np.inf, F32)
        ok = np.ones(n, bool)
        for p in cam:
            hx = _dot3(k[0, 0], k[0, 1], k[0, 2], p[0], p[1], p[2])
            hy = _dot3(k[1, 0], k[1, 1], k[1, 2], p[0], p[1], p[2])
            hw = _dot3(k[2, 0], k[2, 1], k[2, 2], p[0], p[1], p[2])
            u, v = hx / hw, hy / hw
            ok &= (hw > 0) & (np.abs(u) < np.inf) & (np.abs(v) < np.inf)
            lo_x, hi_x = np.fmin(lo_x, u), np.fmax(hi_x, u)
            lo_y, hi_y = np.fmin(lo_y, v), np.fmax(hi_y, v)
        fs = F32(s)
        x0, x1 = np.floor((lo_x - F32(1.0)) * fs), np.floor((hi_x + F32(1.0)) * fs)
        y0, y1 = np.floor((lo_y - F32(1.0)) * fs), np.floor((hi_y + F32(1.0)) * fs)
        max_x, max_y = F32(sw - 1), F32(sh - 1)
        cls = np.full(n, STRADDLING, np.int32)
        cls[front & ok] = FRONT
        cls[behind] = BEHIND
        cls[~finite] = DROPPED
        on = (cls == FRONT) & ~((x1 < 0) | (y1 < 0) | (x0 > max_x) | (y0 > max_y))
        box = np.tile(np.array([1, 1, 0, 0], np.int32), (n, 1))
        cl = lambda a, lo, hi: np.clip(np.where(on, a, 0), lo, hi).astype(np.int32)      # noqa: E731
        box[on, 0] = np.minimum(cl(x0, 0, max_x) // TILE, tiles_x - 1)[on]
        box[on, 1] = np.minimum(cl(y0, 0, max_y) // TILE, tiles_y - 1)[on]
        box[on, 2] = np.minimum(cl(x1, 0, max_x) // TILE, tiles_x - 1)[on]
        box[on, 3] = np.minimum(cl(y1, 0, max_y) // TILE, tiles_y - 1)[on]
    return cls, box


def stats(cls, box):
    """(behind, straddling, binned, pairs) as vsa_shell_raster_setup reports them."""
    on = box[:, 0] <= box[:, 2]
    pairs = ((box[:, 2] - box[:, 0] + 1).astype(np.int64) * (box[:, 3] - box[:, 1] + 1))[on].sum()
    return int((cls == BEHIND).sum()), int((cls == STRADDLING).sum()), int(on.sum()), int(pairs)


def tile_lists(cls, box, H, W, s):
    """{(tx, ty): sorted slots} of the non-empty tile lists, and the sorted straddling slots (in every tile's list)."""
    lists = {}
    for slot in np.nonzero(box[:, 0] <= box[:, 2])[0]:
        x0, y0, x1, y1 = box[slot]
        for ty in range(y0, y1 + 1):
            for tx in range(x0, x1 + 1):
                lists.setdefault((tx, ty), []).append(int(slot))
    return lists, [int(i) for i in np.nonzero(cls == STRADDLING)[0]]


def sample_points(H, W, s):
    """(x [N], y [N] f32 pixel coordinates, X [N], Y [N] sample indices) in the output order: pixel-major, a pixel's
    s^2 samples consecutive, j outer, i inner."""
    n = np.arange(H * W * s * s, dtype=np.int64)
    pixel, sub = n // (s * s), n % (s * s)
    row, col, j, i = pixel // W, pixel % W, sub // s, sub % s
    x = col.astype(F32) + (i.astype(F32) + F32(0.5)) / F32(s)
    y = row.astype(F32) + (j.astype(F32) + F32(0.5)) / F32(s)
    return x.astype(F32), y.astype(F32), col * s + i, row * s + j


def pinhole_rays(c2w, kinv, x, y):
    """(rays_o [N, 3], rays_d [N, 3]) f32: csrc/pinhole.h in its operation order."""
    c2w, kinv = np.asarray(c2w, F32).reshape(3, 4), np.asarray(kinv, F32).reshape(3, 3)
    dc = [(kinv[i, 0] * x + kinv[i, 1] * y) + kinv[i, 2] for i in range(3)]
    d = [(c2w[i, 0] * dc[0] + c2w[i, 1] * dc[1]) + c2w[i, 2] * dc[2] for i in range(3)]
    n = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    rays_d = np.stack([v / n for v in d], 1).astype(F32)
    return np.broadcast_to(c2w[:, 3], rays_d.shape).copy(), rays_d


def tri_test(tris, o, d, t_min=0.0):
    """tri_test of every ray against every record: (accept [N, F] bool, t, u, v [N, F] f32)."""
    tris = np.asarray(tris, F32).reshape(-1, 12)
    v0, e1, e2 = tris[None, :, 0:3], tris[None, :, 4:7], tris[None, :, 8:11]
    o, d = np.asarray(o, F32)[:, None, :], np.asarray(d, F32)[:, None, :]
    with np.errstate(all="ignore"):
        px = d[..., 1] * e2[..., 2] - d[..., 2] * e2[..., 1]
        py = d[..., 2] * e2[..., 0] - d[..., 0] * e2[..., 2]
        pz = d[..., 0] * e2[..., 1] - d[..., 1] * e2[..., 0]
        det = _dot3(e1[..., 0], e1[..., 1], e1[..., 2], px, py, pz)
        ok = ~(np.abs(det) < F32(1e-20))
        inv = F32(1.0) / det
        tx, ty, tz = o[..., 0] - v0[..., 0], o[..., 1] - v0[..., 1], o[..., 2] - v0[..., 2]
        u = _dot3(tx, ty, tz, px, py, pz) * inv
        ok &= (u >= 0) & (u <= 1)
        qx = ty * e1[..., 2] - tz * e1[..., 1]
        qy = tz * e1[..., 0] - tx * e1[..., 2]
        qz = tx * e1[..., 1] - ty * e1[..., 0]
        v = _dot3(d[..., 0], d[..., 1], d[..., 2], qx, qy, qz) * inv
        ok &= (v >= 0) & (u + v <= 1)
        t = _dot3(e2[..., 0], e2[..., 1], e2[..., 2], qx, qy, qz) * inv
        ok &= t > F32(t_min)
    return ok, t.astype(F32), u.astype(F32), v.astype(F32)


def accepted_pairs(tris, o, d, t_min=0.0, chunk=4096):
    """(ray index [P], record index [P]) of every pair tri_test accepts, by brute force."""
    rays, recs = [], []
    for a in range(0, o.shape[0], chunk):
        ok, _, _, _ = tri_test(tris, o[a:a + chunk], d[a:a + chunk], t_min)
        r, f = np.nonzero(ok)
        rays.append(r + a)
        recs.append(f)
    return np.concatenate(rays), np.concatenate(recs)


def closest_hit(tris, slots, o, d, t_min=0.0):
    """The hit record of ONE ray over the records `slots` (global indices into tris), in any order: smallest t, ties
    to the smallest original face id.  (t, slot, u, v); (0, -1, 0, 0) for a miss, as write_hit stores it."""
    slots = np.asarray(slots, np.int64)
    if slots.size == 0:
        return F32(0), -1, F32(0), F32(0)
    tris = np.asarray(tris, F32).reshape(-1, 12)
    ok, t, u, v = tri_test(tris[slots], np.asarray(o, F32)[None], np.asarray(d, F32)[None], t_min)
    ok, t, u, v = ok[0], t[0], u[0], v[0]
    if not ok.any():
        return F32(0), -1, F32(0), F32(0)
    ids = tris[slots, 3].copy().view(np.int32)
    cand = np.nonzero(ok)[0]
    best = min(cand, key=lambda c: (t[c], ids[c]))
    return t[best], int(slots[best]), u[best], v[best]


def adversarial_soup(eye, seed=7, per_kind=150):
    """4 x per_kind faces around the origin for a camera at `eye` looking at the origin: needles (one edge 1e-3 of the
    others), faces edge-on to the eye (the third vertex in the plane through the eye and the first two, up to fp32
    rounding), faces through the camera plane (vertices on both sides of the eye along the view axis), and faces of
    size 1e-4.  (vertices [3 F, 3] f32, faces [F, 3] i32)."""
    rng = np.random.default_rng(seed)
    eye = np.asarray(eye, np.float64)
    axis = -eye / np.linalg.norm(eye)
    tris = []
    for _ in range(per_kind):                                   # needles
        a = rng.uniform(-0.4, 0.4, 3)
        b = a + rng.uniform(-0.4, 0.4, 3)
        tris.append([a, b, a + 1e-3 * rng.uniform(-0.4, 0.4, 3)])
    for _ in range(per_kind):                                   # edge-on
        a, b = rng.uniform(-0.4, 0.4, 3), rng.uniform(-0.4, 0.4, 3)
        s, t = rng.uniform(0.2, 1.5, 2)
        tris.append([a, b, eye + s * (a - eye) + t * (b - eye)])
    for _ in range(per_kind):                                   # through the camera plane
        a = eye + rng.uniform(-0.3, 0.3, 3) + axis * rng.uniform(0.01, 0.5)
        b = eye + rng.uniform(-0.3, 0.3, 3) - axis * rng.uniform(0.0, 0.5)
        c = eye + rng.uniform(-0.3, 0.3, 3) + axis * rng.uniform(-0.2, 0.5)
        tris.append([a, b, c])
    for _ in range(per_kind):                                   # tiny
        a = rng.uniform(-0.4, 0.4, 3)
        tris.append([a, a + 1e-4 * rng.uniform(-1, 1, 3), a + 1e-4 * rng.uniform(-1, 1, 3)])
    v = np.asarray(tris, np.float64).reshape(-1, 3).astype(F32)
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)
