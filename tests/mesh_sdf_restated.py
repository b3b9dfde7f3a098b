"""The signed-distance rule (include/volsurfs_hip.h "Mesh signed distance") restated in numpy, written from
the rule, on top of tests/mesh_distance_restated.py: the region code out of the same chain of tests as (u, v), the
pseudonormal table in float64 from the float32 vertices (stored as float32), the sign of r . N in float32 in the
device's order.  Beside it an independent rule for closed meshes: the parity of the float64 generalised winding number
(the solid angles of Van Oosterom & Strackee), which knows nothing of closest features.  The yardstick of
tests/test_mesh_sdf.py."""
import numpy as np

import mesh_distance_restated as R

F32 = np.float32
A, B, C, AB, AC, BC, IN = range(7)
REGION_NAMES = ("A", "B", "C", "AB", "AC", "BC", "in")


def records(vertices, faces):
    """[F, 12] float32 records in face order (v0, id | e1, - | e2, -), as every builder forms them."""
    v = np.asarray(vertices, F32)
    f = np.asarray(faces, np.int64)
    rec = np.zeros((f.shape[0], 12), F32)
    rec[:, 0:3] = v[f[:, 0]]
    rec[:, 3] = np.arange(f.shape[0], dtype=np.int32).view(F32)
    rec[:, 4:7] = v[f[:, 1]] - v[f[:, 0]]
    rec[:, 8:11] = v[f[:, 2]] - v[f[:, 0]]
    return rec


def region_and_residual(points, recs):
    """(region [N] int, r [N, 3] float32, u, v [N] float32) of point i against record i: the first region that holds,
    in Ericson's order, with the weights it gives; "otherwise" is A."""
    p = np.asarray(points, F32).reshape(-1, 3)
    t = np.asarray(recs, F32).reshape(-1, 12)
    zero, one = F32(0.0), F32(1.0)
    with np.errstate(all="ignore"):
        a = p - t[:, 0:3]
        e1, e2 = t[:, 4:7], t[:, 8:11]
        dot = lambda x, y: R.dot3(x[:, 0], x[:, 1], x[:, 2], y[:, 0], y[:, 1], y[:, 2])
        d1, d2 = dot(e1, a), dot(e2, a)
        b = a - e1
        d3, d4 = dot(e1, b), dot(e2, b)
        c = a - e2
        d5, d6 = dot(e1, c), dot(e2, c)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        den_ab, den_ac = d1 - d3, d2 - d6
        t43, t56 = d4 - d3, d5 - d6
        den_bc = t43 + t56
        total = (va + vb) + vc
        inv = one / total
        v_bc = t43 / den_bc
        chain = [
            ((d1 <= zero) & (d2 <= zero), A, zero, zero),
            ((d3 >= zero) & (d4 <= d3), B, one, zero),
            ((vc <= zero) & (d1 >= zero) & (d3 <= zero) & (den_ab > zero), AB, d1 / den_ab, zero),
            ((d6 >= zero) & (d5 <= d6), C, zero, one),
            ((vb <= zero) & (d2 >= zero) & (d6 <= zero) & (den_ac > zero), AC, zero, d2 / den_ac),
            ((va <= zero) & (t43 >= zero) & (t56 >= zero) & (den_bc > zero), BC, one - v_bc, v_bc),
            (total > zero, IN, vb * inv, vc * inv),
        ]
        region = np.full(p.shape[0], A, np.int64)
        u = np.zeros(p.shape[0], F32)
        v = np.zeros(p.shape[0], F32)
        for cond, code, ru, rv in reversed(chain):
            region = np.where(cond, code, region)
            u = np.where(cond, ru, u).astype(F32)
            v = np.where(cond, rv, v).astype(F32)
        r = (a - u[:, None] * e1) - v[:, None] * e2
    assert r.dtype == F32
    return region, r, u, v


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def face_normals(vertices, faces):
    """[F, 3] float64: (e1 x e2) / |e1 x e2| on the float32 vertices, 0 where the length is not positive and finite."""
    v = np.asarray(vertices, F32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    n = _cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    length = np.sqrt(_dot(n, n))
    ok = (length > 0.0) & np.isfinite(length)
    with np.errstate(all="ignore"):
        return np.where(ok[:, None], n / length[:, None], 0.0)


def pseudonormal_table(vertices, faces):
    """[F, 7, 3] float32 by (face, region code): float64 sums in ascending face id, rounded once."""
    v = np.asarray(vertices, F32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    F, V = f.shape[0], v.shape[0]
    fn = face_normals(vertices, faces)
    nv = np.zeros((V, 3))
    for face in range(F):                                  # ascending face id; the first corner that names a vertex
        seen = set()
        for c in range(3):
            i = f[face, c]
            if i in seen:
                continue
            seen.add(i)
            a = v[f[face, (c + 1) % 3]] - v[i]
            b = v[f[face, (c + 2) % 3]] - v[i]
            cr = _cross(a[None], b[None])
            alpha = np.arctan2(np.sqrt(_dot(cr, cr))[0], _dot(a[None], b[None])[0])
            # (a vertex named twice by a face stands twice in its ring: the face is taken twice, at the first corner)
            times = int((f[face] == i).sum())
            for _ in range(times):
                nv[i] += alpha * fn[face]
    esum = {}
    for face in range(F):
        for c in range(3):
            x, y = f[face, c], f[face, (c + 1) % 3]
            key = (min(x, y), max(x, y))
            esum[key] = esum.get(key, np.zeros(3)) + fn[face]
    table = np.zeros((F, 7, 3), F32)
    corner_region = (AB, BC, AC)                           # corner c: the edge from vertex c to the next
    for face in range(F):
        for c in range(3):
            table[face, c] = nv[f[face, c]].astype(F32)
            x, y = f[face, c], f[face, (c + 1) % 3]
            table[face, corner_region[c]] = esum[(min(x, y), max(x, y))].astype(F32)
        table[face, IN] = fn[face].astype(F32)
    return table


def signed_distance(points, vertices, faces, table=None, chunk=256):
    """The rule by brute force: `mesh_distance_restated.closest` over the mesh's records in face order (slot = face),
    plus region [N], residual r [N, 3], normal N [N, 3] (the table's entry), s = r . N (float32), dist signed, and
    cos [N] float64 = the cosine between r and N (1 where r = 0: a point on the surface gets +0 whatever N)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    rec = records(vertices, faces)
    if table is None:
        table = pseudonormal_table(vertices, faces)
    out = R.closest(p, rec, chunk=chunk)
    region, r, u, v = region_and_residual(p, rec[out["slot"]])
    assert np.array_equal(u, out["u"]) and np.array_equal(v, out["v"])
    n = table[out["face"], region]
    s = R.dot3(r[:, 0], r[:, 1], r[:, 2], n[:, 0], n[:, 1], n[:, 2])
    assert s.dtype == F32
    r64, n64 = r.astype(np.float64), n.astype(np.float64)
    with np.errstate(all="ignore"):
        cos = (r64 * n64).sum(1) / (np.linalg.norm(r64, axis=1) * np.linalg.norm(n64, axis=1))
    cos = np.where(out["d2"] == 0, 1.0, cos)
    out.update(region=region, r=r, normal=n, s=s, cos=cos, unsigned=out["dist"],
               dist=np.where(s < 0, -out["dist"], out["dist"]).astype(F32))
    return out


def winding_number(points, vertices, faces, chunk=128):
    """[N] float64: the generalised winding number, sum over the faces of the signed solid angle / 4 pi
    (tan(omega / 2) = a . (b x c) / (|a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|)), all in float64.  ~1 inside a
    closed outward-wound mesh, ~0 outside."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    out = np.empty(p.shape[0])
    for s in range(0, p.shape[0], chunk):
        q = p[s:s + chunk, None, :]
        a, b, c = v[f[:, 0]][None] - q, v[f[:, 1]][None] - q, v[f[:, 2]][None] - q
        la, lb, lc = (np.linalg.norm(x, axis=2) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(2)
        den = la * lb * lc + (a * b).sum(2) * lc + (b * c).sum(2) * la + (c * a).sum(2) * lb
        out[s:s + chunk] = (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)
    return out


# ---- the meshes the tests share

def cube(h=0.25):
    """The axis-aligned cube of half-side h: 8 vertices, 12 faces wound outward."""
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def needle(radius=0.05, height=0.6):
    """A tetrahedron with a base of the given radius in z = 0 and its apex (vertex 3) at z = height; face 0 is the
    base, faces 1..3 the sides, all wound outward."""
    ang = np.array([0.0, 2.0, 4.0]) * np.pi / 3.0
    v = np.concatenate([np.stack([radius * np.cos(ang), radius * np.sin(ang), np.zeros(3)], 1), [[0.0, 0.0, height]]])
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    return v.astype(F32), f


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
