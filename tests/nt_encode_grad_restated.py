"""Float64 restatement of the neural-texture hash grid's table gradient (csrc/nt_encode.hip,
enc_bwd_piece), its rounding bound, and a numpy emulation of the kernel's 32-bit fixed-point arithmetic
with three deliberately wrong variants.  CPU only; used by tests/test_nt_encode_grad.py, whose docstring
derives the bound.

The corner weights and entry indices are oracle/tcnn_like._grid_cells: fp32, the operations the kernel
restates (cell_ref / cell_indices of csrc/nt_enc_common.h).  dF goes from half to float64 exactly; only
the product weight x dF and the sums are float64.

A `Frame` is what the kernel reads besides dF: the slots' texel centres, the (shell, degree) segment
starts and which logical texture adds into which parameter texture.
"""
import numpy as np
import torch

from oracle.tcnn_like import _grid_cells

MAX_DEG = 4
UNIT = 256            # ENC_UNIT: the persistent work split cuts a segment at multiples of 256 slots only
UNROLL = 8            # ENC_UNROLL: consecutive slots of one lane
BLOCK = 1024          # ENC_BLOCK
LDS_ENTRIES = 32768
U = 2.0 ** -24


# ---- the level classes of nt_encode.hip (level_hashed, enc_both_features, `copies`, `merge`)

def level_hashed(res, size):
    return not (res <= size and res * res <= size)


def level_classes(geom):
    """Per level: (hashed, NF, copies) as nt_encode_bwd_body / enc_bwd_piece choose them."""
    out = []
    for l in range(geom.n_levels):
        hashed = level_hashed(geom.res[l], geom.size[l])
        nf = 2 if (not hashed and geom.size[l] * 2 <= LDS_ENTRIES) else 1
        copies = 1
        if not hashed:
            while copies < 32 and geom.size[l] * copies * 2 * nf <= LDS_ENTRIES:
                copies *= 2
        out.append((hashed, nf, copies))
    return out


def merges(geom, level, tex_res):
    """enc_bwd_piece's MERGE of the one-feature instances: cells coarser than texels."""
    return np.float32(geom.scale[level]) < np.float32(tex_res)


# ---- inputs

def texel_centres(R, texels):
    """Texel t of the (R + 2)^2 extended grid (row-major, x fastest) -> its normalised centre, fp32, as
    vsa_nt_compact_frame writes it (R a power of two: an exact scaling)."""
    t = np.asarray(texels, np.int64)
    W = R + 2
    cx = (t % W - 1).astype(np.float32) + np.float32(0.5)
    cy = (t // W - 1).astype(np.float32) + np.float32(0.5)
    return np.stack([cx / np.float32(R), cy / np.float32(R)], axis=1).astype(np.float32)


class Frame:
    """K shells, MAX_DEG degrees, both types active at every degree.  seg [4 K + 1] slot starts,
    xy [>= seg[-1], 2] fp32, tex_res [4]; shared_rgb / shared_alpha: every shell's texture of that type adds
    into shell 0's (nt_param_tex)."""

    def __init__(self, K, seg, xy, tex_res, shared_rgb=False, shared_alpha=False):
        self.K, self.seg, self.xy, self.tex_res = K, [int(s) for s in seg], np.asarray(xy, np.float32), tuple(tex_res)
        self.shared = (bool(shared_rgb), bool(shared_alpha))
        self.n_tex = K * 2 * MAX_DEG
        assert len(self.seg) == K * MAX_DEG + 1

    def pieces(self):
        """(logical texture, parameter texture, type, degree, first slot, last slot) of every non-empty segment."""
        for sd in range(self.K * MAX_DEG):
            a, b = self.seg[sd], self.seg[sd + 1]
            if b <= a:
                continue
            shell, deg = divmod(sd, MAX_DEG)
            for typ in range(2):
                tex = (shell * 2 + typ) * MAX_DEG + deg
                yield tex, (tex % (2 * MAX_DEG) if self.shared[typ] else tex), typ, deg, a, b


def abs_sum_rounded_up(dF, frame):
    """[n_tex, 32] fp32: per logical texture and feature column 2 level + f, the float64 sum of |dF| over the
    texture's slots, rounded UP to fp32 (what a producer that never under-reports would hand over)."""
    out = np.zeros((frame.n_tex, 32), np.float32)
    for tex, _, typ, _, a, b in frame.pieces():
        s = np.abs(dF[typ, :, a:b, :].astype(np.float64)).sum(axis=1).reshape(32)     # [level, f] -> 2 level + f
        r = s.astype(np.float32)
        r = np.where(r.astype(np.float64) < s, np.nextafter(r, np.float32(np.inf)), r)
        out[tex] = r
    return out


def quantum_exponent(dfsum):
    """e of the kernel's `total = fl(dfsum * 1.001f) = m 2^e`, m in [0.5, 1) (frexpf); None where total is 0."""
    total = (np.float32(dfsum) * np.float32(1.001)).astype(np.float32)
    return int(np.frexp(total)[1]) if total > 0 else None


# ---- the reference

def table_grad_f64(geom, frame, dF, dfsum):
    """dF [2 types, 16 levels, >= seg[-1] slots, 2] float16, dfsum [n_tex, 32] fp32 (the value the kernel is
    GIVEN).  Per float of the gradient tables [n_tex, n_entries, 2], indexed by the PARAMETER texture, in
    units of dF (not yet divided by grad_scale):
      S  the float64 sum of w g,  A the sum of |w g|,  n the contributions with g != 0 (int64),
      H  the sum over those contributions of q / 2, q = 2^(e - 30) the quantum of the contributing LOGICAL
         texture's (level, feature)  (shared models: K logical textures with K quanta add into one float),
      P  the 256-slot units of the contributing segments, at most n: the float adds of ONE launch over all shells.
    Asserts what the fixed point needs: sum |g| 2^(30 - e) + n / 2 < 2^31 per logical (texture, level, feature)
    with n = 4 corners x the nonzero slots, and that a nonzero dF never meets a zero dfsum."""
    N = geom.offset[-1]
    shape = (frame.n_tex, N, 2)
    S, A, H = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    n, P = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    xy = torch.from_numpy(frame.xy)
    cells = {}
    for tex, pt, typ, deg, a, b in frame.pieces():
        units = (b - a + UNIT - 1) // UNIT
        for l in range(geom.n_levels):
            if (l, a, b) not in cells:
                idx, w = _grid_cells(geom, l, xy[a:b])
                assert w.dtype == torch.float32
                cells[(l, a, b)] = idx.numpy().ravel(), w.numpy().astype(np.float64)
            i, w = cells[(l, a, b)]
            lo, size = geom.offset[l], geom.size[l]
            for f in range(2):
                g = dF[typ, l, a:b, f].astype(np.float64)
                assert np.isfinite(g).all(), "non-finite dF is outside this reference"
                nz_slots = int((g != 0).sum())
                if nz_slots == 0:
                    continue
                e = quantum_exponent(dfsum[tex, 2 * l + f])
                assert e is not None, "nonzero dF under a zero dfeat_abs_sum"
                assert np.abs(g).sum() * 2.0 ** (30 - e) + 2 * nz_slots < 2.0 ** 31
                c = (w * g[None, :]).ravel()
                nz = np.broadcast_to(g != 0, w.shape).ravel()
                cnt = np.bincount(i[nz], minlength=size)
                S[pt, lo:lo + size, f] += np.bincount(i[nz], weights=c[nz], minlength=size)
                A[pt, lo:lo + size, f] += np.bincount(i[nz], weights=np.abs(c[nz]), minlength=size)
                n[pt, lo:lo + size, f] += cnt
                H[pt, lo:lo + size, f] += cnt * 2.0 ** (e - 31)
                P[pt, lo:lo + size, f] += np.minimum(cnt, units)
    return S, A, n, H, P


def bound(A, H, P, prefill, grad_scale, launches=1):
    """The bound of the test module's docstring, in units of the OUTPUT (divided by grad_scale), for `launches`
    equal launches in a row into a buffer that held `prefill`."""
    m = float(launches)
    A1 = m * (A + H)
    Pm = m * P
    p1 = np.abs(prefill.astype(np.float64)) * grad_scale          # the held value in units of dF
    b = m * H + U * m * A + (2 + Pm) * U * A1 + Pm * U * p1
    if np.frexp(grad_scale)[0] != 0.5:                            # fl(1 / grad_scale): one more rounding
        b = b + U * A1
    return b / grad_scale


# ---- the kernel's arithmetic, emulated (ONE piece per segment: one flush, P = 1, into a zero buffer)

def emulate(geom, frame, dF, dfsum, grad_scale, mutant=None):
    """fp32 product w * (dF 2^(30 - e)), floor(x + 0.5), integer sum, conversion to float, product with
    2^(e - 30) * fl(1 / grad_scale).  Returns float32 [n_tex, n_entries, 2].
    mutant: "truncate"     the product is truncated toward zero instead of rounded;
            "drop_corner"  corner 3 of the LAST slot of every segment is lost;
            "drop_copy"    of the `copies` LDS planes of a dense level, the last one is left out of the flush
                           (a lane's plane is lane & (copies - 1), a lane owns 8 consecutive slots from the
                           segment's 8-aligned start)."""
    assert not any(frame.shared)
    out = np.zeros((frame.n_tex, geom.offset[-1], 2), np.float32)
    rinv = np.float32(1.0) / np.float32(grad_scale)
    xy = torch.from_numpy(frame.xy)
    classes = level_classes(geom)
    for tex, pt, typ, deg, a, b in frame.pieces():
        lane = ((np.arange(a, b) - (a & ~(UNROLL - 1))) // UNROLL) % BLOCK
        for l in range(geom.n_levels):
            idx, w = _grid_cells(geom, l, xy[a:b])
            idx, w = idx.numpy(), w.numpy()
            lo, size = geom.offset[l], geom.size[l]
            copies = classes[l][2]
            for f in range(2):
                e = quantum_exponent(dfsum[tex, 2 * l + f])
                if e is None:
                    continue
                gv = dF[typ, l, a:b, f].astype(np.float32) * np.float32(2.0 ** (30 - e))       # exact
                prod = (w * gv[None, :]).astype(np.float32).astype(np.float64)
                v = np.trunc(prod) if mutant == "truncate" else np.floor(prod + 0.5)
                if mutant == "drop_corner":
                    v[3, -1] = 0
                if mutant == "drop_copy" and copies > 1:
                    v[:, (lane & (copies - 1)) == copies - 1] = 0
                vi = np.bincount(idx.ravel(), weights=v.ravel(), minlength=size)                 # integers < 2^31: exact
                assert np.abs(vi).max() < 2.0 ** 31
                s_inv = np.float32(2.0 ** (e - 30)) * rinv
                out[pt, lo:lo + size, f] = vi.astype(np.float32) * s_inv
    return out


# ---- dF values

def gradient_normal(rng, n_slots):
    """Normal values divided by the slot count, as half."""
    return (rng.standard_normal((16, n_slots, 2)) / max(n_slots, 1)).astype(np.float16)


def gradient_dynamic_range(rng, n_slots):
    """+-10^-4 .. 1 (log-uniform), one in ten an exact zero, one in twenty an fp16 subnormal (k 2^-24)."""
    shape = (16, n_slots, 2)
    g = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * 10.0 ** (-4.0 * rng.random(shape))
    kind = rng.random(shape)
    sub = rng.integers(1, 1024, shape) * 2.0 ** -24 * np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    g = np.where(kind < 0.10, 0.0, np.where(kind < 0.15, sub, g))
    return g.astype(np.float16)
