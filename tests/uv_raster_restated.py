"""The atlas raster rule (include/volsurfs_hip.h "UV atlas", raster; csrc/uv_raster.h) restated in numpy, once: which
texel centres of an R x R atlas a uv triangle covers.  Corners are clamped to [0, 1] in float32 (a NaN clamps to 0, as
fminf(fmaxf(x, 0), 1) does), snapped in float64 to 1/256 texel (rint of uv * 256 R), and tested with int64 edge functions
under the top-left rule; a face whose snapped signed area is <= 0 covers nothing.  The yardstick of tests/test_atlas.py
(`raster`) and tests/texture_transfer_restated.py (`covers`)."""
import numpy as np

SNAP = 256


def snap(faces_uvs, R):
    """(X, Y) int64 [F, 3]: the snapped corners."""
    uv = np.asarray(faces_uvs, np.float32).reshape(-1, 3, 2)
    uv = np.where(np.isnan(uv), np.float32(0), uv)
    s = np.rint(np.clip(uv, np.float32(0), np.float32(1)).astype(np.float64) * (float(SNAP) * R)).astype(np.int64)
    return s[:, :, 0], s[:, :, 1]


def front(X, Y):
    """Is the snapped signed area > 0?"""
    return (X[..., 1] - X[..., 0]) * (Y[..., 2] - Y[..., 0]) - (Y[..., 1] - Y[..., 0]) * (X[..., 2] - X[..., 0]) > 0


def edge_in(ax, ay, bx, by, px, py):
    """Is (px, py) on the inner side of the edge a -> b, or on it when it is a top or a left edge?"""
    dx, dy = bx - ax, by - ay
    e = dx * (py - ay) - dy * (px - ax)
    return (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx < 0))))


def _inside(X, Y, px, py):
    """The three edge tests of texel centres (px, py) against corners X, Y [..., 3] (shapes that broadcast)."""
    out = front(X, Y)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        out = out & edge_in(X[..., a], Y[..., a], X[..., b], Y[..., b], px, py)
    return out


def covers(faces_uvs, R, i, j):
    """[N, F] bool: does face f cover texel (i[n], j[n])?"""
    X, Y = snap(faces_uvs, R)
    px = (np.asarray(i, np.int64) * SNAP + SNAP // 2)[:, None]
    py = (np.asarray(j, np.int64) * SNAP + SNAP // 2)[:, None]
    return _inside(X[None], Y[None], px, py)


def boxes(X, Y, R):
    """(i0, i1, j0, j1) [F]: the inclusive box of the texels whose centres lie within the snapped corners' bounds, cut
    to the atlas; empty in i (i1 = i0 - 1) when the snapped area is <= 0."""
    h = SNAP // 2
    i0 = np.maximum(-((-(X.min(1) - h)) // SNAP), 0)
    i1 = np.minimum((X.max(1) - h) // SNAP, R - 1)
    j0 = np.maximum(-((-(Y.min(1) - h)) // SNAP), 0)
    j1 = np.minimum((Y.max(1) - h) // SNAP, R - 1)
    return i0, np.where(front(X, Y), i1, i0 - 1), j0, j1


def raster(faces_uvs, R):
    """(face_id [R, R] (the lowest covering face, -1: none), count [R, R], pair faces, pair texel index): every
    (face, covered texel) pair, found by walking each face's box."""
    X, Y = snap(faces_uvs, R)
    i0, i1, j0, j1 = boxes(X, Y, R)
    ni, nj = np.maximum(i1 - i0 + 1, 0), np.maximum(j1 - j0 + 1, 0)
    n = ni * nj
    f = np.repeat(np.arange(len(X)), n)
    k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    i = i0[f] + k % np.maximum(ni[f], 1)
    j = j0[f] + k // np.maximum(ni[f], 1)
    inside = _inside(X[f], Y[f], i * SNAP + SNAP // 2, j * SNAP + SNAP // 2)
    f, t = f[inside], (j * R + i)[inside]
    count = np.bincount(t, minlength=R * R).astype(np.int32)
    fid = np.full(R * R, np.iinfo(np.int64).max)
    np.minimum.at(fid, t, f)
    fid[count == 0] = -1
    return fid.reshape(R, R).astype(np.int32), count.reshape(R, R), f, t
