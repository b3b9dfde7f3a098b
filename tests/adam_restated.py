"""Restatement of the fused Adam step (csrc/adam.hip), written from the formulas of its header
comment and of include/volsurfs_hip.h.  CPU only; used by tests/test_adam_step.py.

  m' = m + (1 - beta1) (s g - m)
  v' = beta2 v + (1 - beta2) (s g)^2
  p' = p - lr / (1 - beta1^t) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)

with s = grad_scale, an f16 copy of p' and a cleared gradient.  Two forms:

`emulate` does the step in numpy float32, one correctly rounded operation after the other in the
order the kernel documents.  The kernel is elementwise, has no atomics, is built without
contraction, with IEEE division and square root and with denormals kept, so `emulate` is what it
must produce BIT FOR BIT.

`reference` does the same step in float64 from the same fp32 inputs and the same coefficients, and
bounds how far any fp32 evaluation in that operation order can lie from it.
"""
import collections
import math

import numpy as np

CHUNK = 4096            # elements per workgroup (vsa_adam_chunk_elems)
GROUP = 4               # elements per lane and array: the granularity of the idle skip
U32 = 2.0 ** -24        # unit roundoff of float32
U64 = 2.0 ** -53

# what the kernel receives besides eps and grad_scale (AdamCoef in adam.hip).  np.float32 scalars
# from `coef`; Python floats (doubles) where the float64 reference is compared with torch.optim.Adam
Coef = collections.namedtuple("Coef", "step_size beta1 beta2 inv_bc2_sqrt")


def coefficients(lr, beta1, beta2, step):
    """(step_size, inv_bc2_sqrt) as the host entry points form them: lr and the betas arrive as
    floats, the bias corrections 1 - beta^step are formed in double (libm pow, as torch.optim.Adam
    forms them on the host) and the two results are rounded to float."""
    lr, b1, b2 = float(np.float32(lr)), float(np.float32(beta1)), float(np.float32(beta2))
    bc1 = 1.0 - math.pow(b1, float(step))
    bc2 = 1.0 - math.pow(b2, float(step))
    return np.float32(lr / bc1), np.float32(1.0 / math.sqrt(bc2))


def coef(lr, beta1, beta2, step):
    step_size, inv_bc2_sqrt = coefficients(lr, beta1, beta2, step)
    return Coef(step_size, np.float32(beta1), np.float32(beta2), inv_bc2_sqrt)


def idle_groups(g, m, v):
    """bool [ceil(n / 4)]: the 4-element groups, counted from the tensor's start, in which g, m and
    v are all zero (either sign).  The last group of a ragged tensor counts its valid elements only.
    The kernel issues none of its five stores for such a group."""
    n = g.size
    pad = (-n) % GROUP
    z = (np.ravel(g) == 0) & (np.ravel(m) == 0) & (np.ravel(v) == 0)
    return np.concatenate([z, np.ones(pad, bool)]).reshape(-1, GROUP).all(axis=1)


def idle_elements(g, m, v):
    """bool [n]: `idle_groups` per element."""
    return np.repeat(idle_groups(g, m, v), GROUP)[:g.size]


def emulate(p, g, m, v, coef, eps, grad_scale, h=None):
    """One step in float32 on flat fp32 arrays.  Returns (p', m', v', h'), h' = half(p').
    Idle groups keep p, m, v and — where the f16 copy's previous content `h` is given — h."""
    f = np.float32
    p, g, m, v = (np.ascontiguousarray(a, f).ravel() for a in (p, g, m, v))
    step_size, b1, b2, ibc = f(coef.step_size), f(coef.beta1), f(coef.beta2), f(coef.inv_bc2_sqrt)
    eps, s = f(eps), f(grad_scale)
    omb1, omb2 = f(1) - b1, f(1) - b2
    with np.errstate(all="ignore"):
        gk = g * s
        m1 = m + omb1 * (gk - m)
        v1 = v * b2 + (omb2 * gk) * gk
        denom = np.sqrt(v1) * ibc + eps
        p1 = p - step_size * (m1 / denom)
        idle = idle_elements(g, m, v)
        p1, m1, v1 = np.where(idle, p, p1), np.where(idle, m, m1), np.where(idle, v, v1)
        h1 = p1.astype(np.float16)                 # round to nearest even, subnormals and infinities included
    if h is not None:
        h1 = np.where(idle, np.ascontiguousarray(h, np.float16).ravel(), h1)
    assert p1.dtype == m1.dtype == v1.dtype == f
    return p1, m1, v1, h1


def _gamma(k, u):
    """Any product of k factors (1 + d)^(+-1), |d| <= u — a factor (1 + d)^(+-1/2) counting as half
    a factor — lies in [1 - k u, 1 / (1 - k u)] (Bernoulli), that is within k u / (1 - k u) of 1."""
    return k * u / (1.0 - k * u)


def reference(p, g, m, v, coef, eps, grad_scale, u=U32):
    """The same step in float64.  Returns (p', m', v'), (e_p, e_m, e_v): the step evaluated in
    float64 on the given inputs with the given coefficients (1 - beta is formed in the coefficients'
    own type, as the kernel forms it in float), and per element how far an evaluation may lie from
    it that performs the operations of `emulate` in its order, each rounded to nearest with unit
    roundoff u, provided none of them underflows, v >= 0 and eps >= 0.

    Derivation (fl(x) = x (1 + d), |d| <= u; hats are computed values):
      gk^ = fl(g s)                                  |gk^ - gk| <= e_gk = u |gk|
      d^  = fl(gk^ - m)                              |d^ - (gk - m)| <= e_d = (1 + u) e_gk + u |gk - m|
      t^  = fl(omb1 d^)                              |t^ - omb1 (gk - m)| <= e_t = (1 + u) omb1 e_d + u |omb1 (gk - m)|
      m'^ = fl(m + t^)                               |m'^ - m'| <= e_m = (1 + u) e_t + u |m'|
    To first order e_m = omb1 e_gk + omb1 u |gk - m| + u |omb1 (gk - m)| + u |m'|.
      v'^ = fl(fl(v beta2) + fl(fl(omb2 gk^) gk^))   both terms are >= 0, the first carries 2 roundings and
                                                     the second 5 (gk^ twice): v'^ = v' (1 + th), |th| <= gamma(5)
      den^ = fl(fl(fl(sqrt(v'^)) ibc) + eps)         sqrt halves th and adds a rounding (3.5), the product one (4.5),
                                                     the sum one (5.5); eps >= 0 carries only the last:
                                                     den^ = den (1 + ph), |ph| <= gamma(5.5)
      r^  = fl(step_size fl(m'^ / den^))             = step_size m'^ / den (1 + ps), |ps| <= gamma(7.5)
                                                     |r^ - upd| <= e_r = gamma(7.5) |upd| + (1 + gamma(7.5)) step_size e_m / den
      p'^ = fl(p - r^)                               |p'^ - p'| <= e_p = (1 + u) e_r + u |p'|
    To first order e_p = 7.5 u |upd| + step_size e_m / den + u |p'|.
    The float64 evaluation itself is off by the same formula at 2^-53, 2^-29 of this bound."""
    d = np.float64
    p, g, m, v = (np.asarray(a).astype(d).ravel() for a in (p, g, m, v))
    one = type(coef.beta1)(1)
    omb1, omb2 = d(one - coef.beta1), d(one - coef.beta2)
    step_size, b2, ibc = d(coef.step_size), d(coef.beta2), d(coef.inv_bc2_sqrt)
    s = d(grad_scale)
    eps = d(eps)
    with np.errstate(all="ignore"):
        gk = g * s
        dm = gk - m
        t = omb1 * dm
        m1 = m + t
        v1 = v * b2 + (omb2 * gk) * gk
        den = np.sqrt(v1) * ibc + eps
        upd = step_size * (m1 / den)
        p1 = p - upd
        e_gk = u * np.abs(gk)
        e_d = (1 + u) * e_gk + u * np.abs(dm)
        e_t = (1 + u) * omb1 * e_d + u * np.abs(t)
        e_m = (1 + u) * e_t + u * np.abs(m1)
        e_v = _gamma(5, u) * v1
        e_r = _gamma(7.5, u) * np.abs(upd) + (1 + _gamma(7.5, u)) * step_size * e_m / den
        e_p = (1 + u) * e_r + u * np.abs(p1)
    return (p1, m1, v1), (e_p, e_m, e_v)


def smallest_normal_margin(p, g, m, v, coef, eps, grad_scale):
    """The smallest nonzero magnitude among the intermediates of `emulate` (products, quotient and
    square root: sums and differences are exact where they fall below the normal range).  The bound
    of `reference` assumes it is a normal number (>= 2^-126)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, f).ravel() for a in (p, g, m, v))
    omb1, omb2 = f(1) - f(coef.beta1), f(1) - f(coef.beta2)
    with np.errstate(all="ignore"):
        gk = g * f(grad_scale)
        t = omb1 * (gk - m)
        m1 = m + t
        a, hq = v * f(coef.beta2), omb2 * gk
        q = hq * gk
        w = np.sqrt(a + q) * f(coef.inv_bc2_sqrt)
        quo = m1 / (w + f(eps))
        r = f(coef.step_size) * quo
    mags = np.abs(np.concatenate([gk, t, a, hq, q, w, quo, r]).astype(np.float64))
    mags = mags[(mags > 0) & np.isfinite(mags)]
    return float(mags.min()) if mags.size else float("inf")


# ---- descriptors: what the entry points read from device memory

def descriptors(entries):
    """entries: (param, grad, exp_avg, exp_avg_sq, param_f16 or None, n) device addresses as ints —
    any address inside an allocation, n no larger than what lies behind it.  Returns the bytes of the
    `vsa_adam_tensor` array."""
    from volsurfs_amd.optim import AdamTensor
    arr = (AdamTensor * max(len(entries), 1))()
    for i, (p, g, m, v, h, n) in enumerate(entries):
        assert all(a % 16 == 0 for a in (p, g, m, v)) and (h is None or h % 8 == 0) and n >= 1
        arr[i] = AdamTensor(p, g, m, v, h, n)
    return bytes(arr)


def chunk_list(ns, chunk=CHUNK):
    """int32 [nr_chunks, 2]: (tensor index, chunk index within the tensor), tensor after tensor."""
    out = [(i, c) for i, n in enumerate(ns) for c in range((n + chunk - 1) // chunk)]
    return np.asarray(out, np.int32).reshape(-1, 2)
