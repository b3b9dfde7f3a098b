"""Restatement of the texture fit (csrc/texel_fit.hip), written from the rule in include/volsurfs_hip.h "Texture fit".
CPU only, numpy; used by tests/test_texture_fit.py.  The step has no float atomics, is built without contraction and
with IEEE division and square root, so what is written here, one correctly rounded fp32 operation after the other,
is what it must produce BIT FOR BIT in p, m, v, texels, grad_rows and stats.

A bank is described by `segments(...)`: per (shell, degree) the resolution R, the quads per row, the first element of
the segment's rows and the [R+2, R+2] table of row indices (-1: the texel's slot lies outside the segment).
"""
import collections

import numpy as np

from adam_restated import coefficients

ROW_QUADS = (2, 4, 8, 8)      # VSA_NT_ROW_QUADS(d)
MAX_DEG = 4

Segment = collections.namedtuple("Segment", "shell degree R quads row0 rows")


def segments(K, D, tex_res, row_base, dom_off, seg_start, slot_of):
    """row_base / dom_off: the plan's [K * 4 + 1 or more] arrays (quads / texels); seg_start: [K * 4 + 1]; slot_of: the
    whole domain array.  Rows are found as vsa_nt_export_planes finds them."""
    out = []
    for s in range(K):
        for d in range(D):
            sd, R, Q = s * MAX_DEG + d, int(tex_res[d]), ROW_QUADS[d]
            W = R + 2
            nrows = (int(row_base[sd + 1]) - int(row_base[sd])) // Q
            rel = np.asarray(slot_of[int(dom_off[sd]):int(dom_off[sd]) + W * W], np.int64).reshape(W, W) - int(seg_start[sd])
            rows = np.where((rel >= 0) & (rel < nrows), rel, -1)
            out.append(Segment(s, d, R, Q, int(row_base[sd]) * 4, rows))
    return out


def clamp_target(ay, ax, R):
    """The interior texel (domain coordinates 1..R) apron texel (ay, ax) of the (R+2)^2 domain folds into."""
    return min(max(ay, 1), R), min(max(ax, 1), R)


def apron_texels(R):
    """The apron texels of an (R+2)^2 domain in row-major order."""
    W = R + 2
    return [(ay, ax) for ay in range(W) for ax in range(W) if ay in (0, W - 1) or ax in (0, W - 1)]


def fold_sets(R):
    """{interior (Y, X): [apron (ay, ax), ...]} in the order the fold adds them (row-major)."""
    out = {(Y, X): [] for Y in range(1, R + 1) for X in range(1, R + 1)}
    for a in apron_texels(R):
        out[clamp_target(*a, R)].append(a)
    return out


def _quad_elems(seg, row):
    """[quads, 4] element indices of row `row` of the segment."""
    return seg.row0 + row * seg.quads * 4 + np.arange(seg.quads * 4).reshape(seg.quads, 4)


def init(segs, texels):
    """-> (p, m, v, texels'): p = byte / 255 on interior texels (zero elsewhere, as are m and v), the apron rows of
    texels' the rows of their clamped interior texels."""
    texels = np.array(texels, np.uint8)
    p = np.zeros(texels.size, np.float32)
    for seg in segs:
        R = seg.R
        for Y in range(1, R + 1):
            for X in range(1, R + 1):
                if seg.rows[Y, X] >= 0:
                    e = _quad_elems(seg, seg.rows[Y, X])
                    p[e] = texels[e].astype(np.float32) / np.float32(255.0)
        for ay, ax in apron_texels(R):
            Y, X = clamp_target(ay, ax, R)
            if seg.rows[ay, ax] >= 0 and seg.rows[Y, X] >= 0:
                texels[_quad_elems(seg, seg.rows[ay, ax])] = texels[_quad_elems(seg, seg.rows[Y, X])]
    return p, np.zeros_like(p), np.zeros_like(p), texels


def step(segs, grad_rows, inv_grad_scale, p, m, v, texels, lr, beta1, beta2, eps, step_nr):
    """One step.  grad_rows: float16 (or its uint16 bits).  Returns (p', m', v', texels', grad_rows' as uint16 bits,
    stats [4]): quads updated, gradient elements not finite, interior bytes changed, elements clamped."""
    f = np.float32
    gbits = np.array(np.asarray(grad_rows).view(np.uint16), np.uint16)
    p, m, v = (np.array(a, f) for a in (p, m, v))
    texels = np.array(texels, np.uint8)
    step_size, ibc = coefficients(lr, beta1, beta2, step_nr)
    b1, b2, eps, inv = f(beta1), f(beta2), f(eps), f(inv_grad_scale)
    omb1, omb2 = f(1) - b1, f(1) - b2
    stats = [0, 0, 0, 0]
    with np.errstate(all="ignore"):
        for seg in segs:
            R, sets = seg.R, fold_sets(seg.R)
            for Y in range(1, R + 1):
                for X in range(1, R + 1):
                    if seg.rows[Y, X] < 0:
                        continue
                    own = _quad_elems(seg, seg.rows[Y, X])
                    sources = [own] + [_quad_elems(seg, seg.rows[a]) for a in sets[(Y, X)] if seg.rows[a] >= 0]
                    g = np.zeros((seg.quads, 4), f)
                    for e in sources:                              # fold, in order; consume
                        live = (gbits[e] != 0).any(axis=1)
                        g[live] = g[live] + gbits[e].view(np.float16).astype(f)[live]
                        gbits[e[live]] = 0
                    g = g * inv
                    bad = ~np.isfinite(g)
                    stats[1] += int(bad.sum())
                    g[bad] = 0
                    for q in np.nonzero((g != 0).any(axis=1))[0]:  # lazy: idle quads are left alone
                        e, gq = own[q], g[q]
                        m1 = m[e] + omb1 * (gq - m[e])
                        v1 = v[e] * b2 + (omb2 * gq) * gq
                        denom = np.sqrt(v1) * ibc + eps
                        p1 = p[e] - step_size * (m1 / denom)
                        stats[3] += int((~((p1 >= 0) & (p1 <= 1))).sum())
                        p1 = np.fmin(np.fmax(p1, f(0)), f(1))
                        byte = np.rint(f(255.0) * p1).astype(np.uint8)
                        stats[0] += 1
                        stats[2] += int((byte != texels[e]).sum())
                        p[e], m[e], v[e] = p1, m1, v1
                        for src in sources:                        # tie
                            texels[src[q]] = byte
    return p, m, v, texels, gbits, stats
