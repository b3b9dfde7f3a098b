"""The closest-point rule (include/volsurfs_hip.h "Mesh distance") restated in numpy, written from the rule:
every quantity in float32, one rounding per operation, in the device's order (the build compiles without contraction),
vectorised over (points x triangle records).  It takes the tracer's exported `tris` ([T, 12] f32: v0.xyz, id | e1.xyz, -
| e2.xyz, -), does the minimum over (d2, original face id) by brute force, and holds the statistics in float64.  The
yardstick of tests/test_mesh_distance.py."""
import numpy as np

F32 = np.float32


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def closest_on_triangles(points, tris):
    """(d2, u, v), each [N, T] float32: the closest point of every record to every point, by the seven regions."""
    p = np.asarray(points, F32).reshape(-1, 3)
    t = np.asarray(tris, F32).reshape(-1, 12)
    px, py, pz = (p[:, k, None] for k in range(3))
    v0x, v0y, v0z = (t[None, :, k] for k in (0, 1, 2))
    e1x, e1y, e1z = (t[None, :, k] for k in (4, 5, 6))
    e2x, e2y, e2z = (t[None, :, k] for k in (8, 9, 10))
    zero, one = F32(0.0), F32(1.0)
    with np.errstate(all="ignore"):
        ax, ay, az = px - v0x, py - v0y, pz - v0z
        d1 = dot3(e1x, e1y, e1z, ax, ay, az)
        d2 = dot3(e2x, e2y, e2z, ax, ay, az)
        bx, by, bz = ax - e1x, ay - e1y, az - e1z
        d3 = dot3(e1x, e1y, e1z, bx, by, bz)
        d4 = dot3(e2x, e2y, e2z, bx, by, bz)
        cx, cy, cz = ax - e2x, ay - e2y, az - e2z
        d5 = dot3(e1x, e1y, e1z, cx, cy, cz)
        d6 = dot3(e2x, e2y, e2z, cx, cy, cz)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        den_ab, den_ac = d1 - d3, d2 - d6
        t43, t56 = d4 - d3, d5 - d6
        den_bc = t43 + t56
        total = (va + vb) + vc
        inv = one / total
        v_bc = t43 / den_bc
        # regions in Ericson's order: the first that holds
        regions = [
            ((d1 <= zero) & (d2 <= zero), zero, zero),                                                   # A
            ((d3 >= zero) & (d4 <= d3), one, zero),                                                      # B
            ((vc <= zero) & (d1 >= zero) & (d3 <= zero) & (den_ab > zero), d1 / den_ab, zero),           # AB
            ((d6 >= zero) & (d5 <= d6), zero, one),                                                      # C
            ((vb <= zero) & (d2 >= zero) & (d6 <= zero) & (den_ac > zero), zero, d2 / den_ac),           # AC
            ((va <= zero) & (t43 >= zero) & (t56 >= zero) & (den_bc > zero), one - v_bc, v_bc),          # BC
            (total > zero, vb * inv, vc * inv),                                                          # interior
        ]
        u = np.zeros(d1.shape, F32)
        v = np.zeros(d1.shape, F32)
        for cond, ru, rv in reversed(regions):
            u = np.where(cond, ru, u).astype(F32)
            v = np.where(cond, rv, v).astype(F32)
        rx = (ax - u * e1x) - v * e2x
        ry = (ay - u * e1y) - v * e2y
        rz = (az - u * e1z) - v * e2z
        dd = dot3(rx, ry, rz, rx, ry, rz)
    assert dd.dtype == F32 and u.dtype == F32 and v.dtype == F32
    return dd, u, v


def closest(points, tris, chunk=256):
    """Brute force: {d2, dist, u, v [N] float32, slot [N] (row of `tris`), face [N] (original id)} by the minimum over
    (d2, id) of all the records given."""
    p = np.asarray(points, F32).reshape(-1, 3)
    t = np.asarray(tris, F32).reshape(-1, 12)
    ids = np.ascontiguousarray(t[:, 3]).view(np.int32).astype(np.int64)
    N = p.shape[0]
    out = {"d2": np.empty(N, F32), "u": np.empty(N, F32), "v": np.empty(N, F32), "slot": np.empty(N, np.int64)}
    for s in range(0, N, chunk):
        dd, u, v = closest_on_triangles(p[s:s + chunk], t)
        best = dd.min(axis=1, keepdims=True)
        masked = np.where(dd == best, ids[None, :], np.iinfo(np.int64).max)
        slot = masked.argmin(axis=1)                    # smallest id among the ties (argmin: the first of equal ids)
        rows = np.arange(dd.shape[0])
        out["d2"][s:s + chunk] = dd[rows, slot]
        out["u"][s:s + chunk] = u[rows, slot]
        out["v"][s:s + chunk] = v[rows, slot]
        out["slot"][s:s + chunk] = slot
    out["dist"] = np.sqrt(out["d2"])
    out["face"] = ids[out["slot"]]
    assert out["dist"].dtype == F32
    return out


def statistics(dist, thresholds=()):
    """{n, min, max, within (exact), mean, rms (float64 sums)} of float32 distances; thresholds compared in float32."""
    d = np.asarray(dist, F32).reshape(-1)
    d64 = d.astype(np.float64)
    return {"n": d.size, "min": float(d.min()), "max": float(d.max()),
            "within": tuple(int((d <= F32(t)).sum()) for t in thresholds),
            "mean": float(d64.sum() / d.size), "rms": float(np.sqrt((d64 * d64).sum() / d.size))}


def face_areas(tris):
    """[T] float64: 0.5 |e1 x e2| in float64 from the float32 edges of the records."""
    t = np.asarray(tris, F32).reshape(-1, 12).astype(np.float64)
    n = np.cross(t[:, 4:7], t[:, 8:11])
    return 0.5 * np.sqrt((n * n).sum(1))


def sample_positions(tris, slot, bary):
    """[n, 3] float32: (v0 + u e1) + v e2 in float32 from records, slots and weights."""
    t = np.asarray(tris, F32).reshape(-1, 12)[np.asarray(slot, np.int64)]
    b = np.asarray(bary, F32).reshape(-1, 2)
    u, v = b[:, :1], b[:, 1:]
    out = (t[:, 0:3] + u * t[:, 4:7]) + v * t[:, 8:11]
    assert out.dtype == F32
    return out
