"""The mesh-crossing rule (include/volsurfs_hip.h "Mesh crossings") restated in numpy float64, operation for
operation, as a brute force over all pairs of faces.  The reference has no such stage: the rule is this library's own
and unpinned.  Every comparison of the device with this file is exact equality.

Triangles are [.., 3, 3] arrays (face, vertex, xyz) of the float32 bits of the meshes' vertex arrays."""
import numpy as np


def triangles(vertices, faces):
    """[F, 3, 3] float64: the vertices of every face, the float32 values converted."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    return v[np.asarray(faces, np.int64)]


def orient(a, b, c, d):
    """det[a - d; b - d; c - d], expanded along its first row, in the header's order."""
    ax, ay, az = a[..., 0] - d[..., 0], a[..., 1] - d[..., 1], a[..., 2] - d[..., 2]
    bx, by, bz = b[..., 0] - d[..., 0], b[..., 1] - d[..., 1], b[..., 2] - d[..., 2]
    cx, cy, cz = c[..., 0] - d[..., 0], c[..., 1] - d[..., 1], c[..., 2] - d[..., 2]
    m0 = by * cz - bz * cy
    m1 = bx * cz - bz * cx
    m2 = bx * cy - by * cx
    return (ax * m0 - ay * m1) + az * m2


def _opposite(s, t):
    return ((s < 0) & (t > 0)) | ((s > 0) & (t < 0))


def _one_sign(x, y, z):
    return ((x >= 0) & (y >= 0) & (z >= 0)) | ((x <= 0) & (y <= 0) & (z <= 0))


def pierces(A, B):
    """(pierce [6, ...] bool, sA [3, ...], sB [3, ...]) of triangles A and B (broadcast against each other): does
    edge 0, 1, 2 of A pierce B, does edge 0, 1, 2 of B pierce A; the sides of B's vertices of A's plane and of A's
    vertices of B's plane."""
    with np.errstate(all="ignore"):
        sB = [orient(B[..., 0, :], B[..., 1, :], B[..., 2, :], A[..., i, :]) for i in range(3)]
        sA = [orient(A[..., 0, :], A[..., 1, :], A[..., 2, :], B[..., j, :]) for j in range(3)]
        e = [[orient(A[..., i, :], A[..., (i + 1) % 3, :], B[..., j, :], B[..., (j + 1) % 3, :]) for j in range(3)]
             for i in range(3)]
        numbers = np.ones(np.broadcast(sA[0], sB[0]).shape, bool)
        for s in sA + sB:
            numbers &= s == s
        out = []
        for i in range(3):
            out.append(numbers & _opposite(sB[i], sB[(i + 1) % 3]) & _one_sign(e[i][0], e[i][1], e[i][2]))
        for j in range(3):
            out.append(numbers & _opposite(sA[j], sA[(j + 1) % 3]) & _one_sign(e[0][j], e[1][j], e[2][j]))
    return np.stack(out), np.stack(sA), np.stack(sB)


def crosses(A, B):
    """bool [...]: do A and B cross (any of the six edges pierces)."""
    return pierces(A, B)[0].any(0)


def segment(A, B):
    """[..., 2, 3] float64: the piercing point of the first and of the last piercing edge in the order A's edges 0, 1,
    2, then B's; NaN where nothing pierces."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    pierce, sA, sB = pierces(A, B)
    shape = pierce.shape[1:]
    first = np.full(shape + (3,), np.nan)
    last = np.full(shape + (3,), np.nan)
    found = np.zeros(shape, bool)
    with np.errstate(all="ignore"):
        for k in range(6):
            T, s, i = (A, sB, k) if k < 3 else (B, sA, k - 3)
            p, q = np.broadcast_to(T[..., i, :], shape + (3,)), np.broadcast_to(T[..., (i + 1) % 3, :], shape + (3,))
            t = s[i] / (s[i] - s[(i + 1) % 3])
            x = p + t[..., None] * (q - p)
            on = pierce[k]
            first[on & ~found] = x[on & ~found]
            last[on] = x[on]
            found |= on
    return np.stack([first, last], -2)


def mesh_crossings(va, fa, vb, fb, chunk=64):
    """Brute force over all pairs: {pairs [P, 2] int64 sorted by (face_a, face_b), count_a [Fa] int32, count_b [Fb]
    int32, segments [P, 2, 3] float64}."""
    A, B = triangles(va, fa), triangles(vb, fb)
    pairs = []
    for lo in range(0, A.shape[0], chunk):
        m = crosses(A[lo:lo + chunk, None], B[None])
        i, j = np.nonzero(m)
        pairs.append(np.stack([i + lo, j], 1))
    pairs = np.concatenate(pairs).astype(np.int64) if pairs else np.zeros((0, 2), np.int64)
    seg = segment(A[pairs[:, 0]], B[pairs[:, 1]]) if len(pairs) else np.zeros((0, 2, 3))
    return {"pairs": pairs, "count_a": np.bincount(pairs[:, 0], minlength=A.shape[0]).astype(np.int32),
            "count_b": np.bincount(pairs[:, 1], minlength=B.shape[0]).astype(np.int32), "segments": seg}


def self_crossings(v, f, chunk=64):
    """The pairs i < j of one mesh's faces that cross, face i as A: {pairs, count [F] int32 (partners per face),
    segments}."""
    T = triangles(v, f)
    pairs = []
    for lo in range(0, T.shape[0], chunk):
        m = crosses(T[lo:lo + chunk, None], T[None])
        i, j = np.nonzero(m)
        keep = j > i + lo
        pairs.append(np.stack([i[keep] + lo, j[keep]], 1))
    pairs = np.concatenate(pairs).astype(np.int64) if pairs else np.zeros((0, 2), np.int64)
    seg = segment(T[pairs[:, 0]], T[pairs[:, 1]]) if len(pairs) else np.zeros((0, 2, 3))
    count = (np.bincount(pairs[:, 0], minlength=T.shape[0]) + np.bincount(pairs[:, 1], minlength=T.shape[0]))
    return {"pairs": pairs, "count": count.astype(np.int32), "segments": seg}
