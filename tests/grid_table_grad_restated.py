"""Float64 restatement of the hash grid's table gradient, and float32 emulations of the
float -> 62-bit fixed-point conversion of the large-batch paths (csrc/grid_encode.hip,
csrc/permuto_encode.hip).  CPU only; used by tests/test_grid_table_grad.py and tests/test_permuto.py.

The corner weights and entry indices are formed in fp32 exactly as oracle/tcnn_like.grid_forward_f32
forms them (pos = x*scale + 0.5, weight ((w0*w1)*w2), GridGeometryND.index); only the product
weight x gradient and the sum over the samples are float64, so that the result is the exact sum of
the numbers the kernels are meant to add, to ~2^-53 of the sum of their magnitudes.
"""
import numpy as np
import torch

SLICE_LOG2 = 13           # the kernels' table slice: 2^13 entries (GS_SLICE_LOG2)


def level_corners(geom, l, x):
    """Level l: entry indices [2^D, B] int64 (within the level) and corner weights [2^D, B] fp32."""
    D = geom.n_dims
    pos = x * np.float32(geom.scale[l]) + np.float32(0.5)
    cell = torch.floor(pos)
    frac = pos - cell
    c = cell.to(torch.int64) & 0xFFFFFFFF
    idx, ws = [], []
    for corner in range(1 << D):
        w, cc = None, []
        for d in range(D):
            bit = (corner >> d) & 1
            wd = frac[:, d] if bit else 1 - frac[:, d]
            w = wd if w is None else w * wd
            cc.append((c[:, d] + bit) & 0xFFFFFFFF)
        idx.append(geom.index(l, cc))
        ws.append(w)
    return torch.stack(idx).numpy(), torch.stack(ws).numpy()


def table_grad_f64(geom, x, g):
    """x [B, D] fp32, g [B, >= 2L] fp32 (columns past 2L are never read).  Per table float
    [n_entries, 2]: the float64 sum of float64(w) * float64(g), A = the sum of their magnitudes,
    n = the number of nonzero contributions (int64).  A non-finite gradient makes the floats its
    corners touch non-finite in sum and A (0 * inf included: the kernels form w * g as well)."""
    assert x.dtype == torch.float32 and g.dtype == torch.float32
    N = geom.offset[-1]
    s, a, n = np.zeros((N, 2)), np.zeros((N, 2)), np.zeros((N, 2), np.int64)
    g64 = g.numpy().astype(np.float64)
    for l in range(geom.n_levels):
        idx, w = level_corners(geom, l, x)
        lo, size = geom.offset[l], geom.size[l]
        for f in range(2):
            with np.errstate(invalid="ignore"):
                c = (w.astype(np.float64) * g64[None, :, 2 * l + f]).ravel()
            i = idx.ravel()
            nz = c != 0                                   # (nan != 0)
            s[lo:lo + size, f] = np.bincount(i[nz], weights=c[nz], minlength=size)
            a[lo:lo + size, f] = np.bincount(i[nz], weights=np.abs(c[nz]), minlength=size)
            n[lo:lo + size, f] = np.bincount(i[nz], minlength=size)
    return s, a, n


def bin_records(geom, x, g):
    """[L, max slices] int64: the records the binned path writes into the bin (level, entry >> 13) —
    2^D per sample whose gradient pair of that level is not (0, 0), zero-weight corners included."""
    slices = max((sz + (1 << SLICE_LOG2) - 1) >> SLICE_LOG2 for sz in geom.size)
    out = np.zeros((geom.n_levels, slices), np.int64)
    gn = g.numpy()
    for l in range(geom.n_levels):
        idx, _ = level_corners(geom, l, x)
        act = (gn[:, 2 * l] != 0) | (gn[:, 2 * l + 1] != 0)
        out[l] = np.bincount((idx[:, act] >> SLICE_LOG2).ravel(), minlength=slices)
    return out


def per_entry(geom, per_bin):
    """[L, slices] values of the bins -> [n_entries, 1], every entry with its bin's value."""
    out = np.zeros((geom.offset[-1], 1), per_bin.dtype)
    for l in range(geom.n_levels):
        sl = np.arange(geom.size[l]) >> SLICE_LOG2
        out[geom.offset[l]:geom.offset[l + 1], 0] = per_bin[l][sl]
    return out


def grad_exponent(g, n_cols):
    """E with 2^(E-1) <= max finite |g[:, :n_cols]| < 2^E (frexp), or None without a nonzero finite one."""
    a = np.abs(g.numpy()[:, :n_cols].astype(np.float64))
    a = a[np.isfinite(a)]
    if a.size == 0 or a.max() == 0:
        return None
    return int(np.frexp(a.max())[1])


def count_bits(worst):
    """The host code's rule: the smallest cb >= 1 with 2^cb >= worst."""
    cb = 1
    while (1 << cb) < worst:
        cb += 1
    return cb


# ---- the conversion, emulated in float32 (int64 results; |v| < 2^62)

def _u32_saturating(v):
    """float32 -> uint32 as the hardware conversion does it: truncation, clamped to [0, 2^32 - 1]."""
    v = np.trunc(v.astype(np.float64))
    return np.clip(v, 0.0, 4294967295.0).astype(np.uint64).astype(np.int64)


def fixed62_signed_split(v):
    """The conversion the kernels used before: the SIGNED value is split, lo = r - floor(r / 2^32) * 2^32
    formed in float32.  For a negative r above -2^31, lo lies in (2^31, 2^32) where floats are 256
    apart, so it rounds; at 2^32 the conversion saturates."""
    v = np.asarray(v, np.float32)
    r = np.rint(v)
    hi = np.floor(r * np.float32(2.0 ** -32))
    lo = (r - hi * np.float32(2.0 ** 32)).astype(np.float32)
    return hi.astype(np.int64) * (1 << 32) + _u32_saturating(lo)


def fixed62_magnitude_split(v):
    """The conversion of csrc/common.h (vsa_fixed62): |r| is split, both halves exact, the integer negated."""
    v = np.asarray(v, np.float32)
    a = np.abs(np.rint(v))
    hi = np.floor(a * np.float32(2.0 ** -32))
    lo = (a - hi * np.float32(2.0 ** 32)).astype(np.float32)
    m = hi.astype(np.int64) * (1 << 32) + _u32_saturating(lo)
    return np.where(v < 0, -m, m)


def table_grad_fixed_point(geom, x, g, convert, cb):
    """The fixed-point paths' arithmetic with ONE partial sum per table float, emulated: the fp32 product
    w * g, scaled by 2^(62 - cb - E), converted by `convert`, summed as integers, scaled back in double
    and rounded to float32.  Finite gradients only."""
    L = geom.n_levels
    E = grad_exponent(g, 2 * L)
    scale = np.float32(2.0 ** (62 - cb - E))
    out = np.zeros((geom.offset[-1], 2), np.float32)
    gn = g.numpy()
    for l in range(L):
        idx, w = level_corners(geom, l, x)
        lo, size = geom.offset[l], geom.size[l]
        for f in range(2):
            q = convert(((w * gn[None, :, 2 * l + f]).astype(np.float32) * scale).ravel())
            acc = np.zeros(size, np.int64)
            np.add.at(acc, idx.ravel(), q)
            out[lo:lo + size, f] = (acc.astype(np.float64) / np.float64(scale)).astype(np.float32)
    return out


# ---- test inputs shared by the grid and the permuto tests

def dynamic_range_gradient(rows, cols, seed):
    """One element exactly 1.0, all others +-u * 2^-k with u in [1, 2), integer k uniform in [16, 34]."""
    r = np.random.default_rng(seed)
    u = 1.0 + r.random((rows, cols))
    k = r.integers(16, 35, (rows, cols))
    sgn = np.where(r.random((rows, cols)) < 0.5, -1.0, 1.0)
    g = (sgn * u * np.exp2(-k.astype(np.float64))).astype(np.float32)
    g[rows // 2, cols // 3] = 1.0
    return torch.from_numpy(g)
