"""The fused Adam step (csrc/adam.hip) against tests/adam_restated.py on every path of the kernel.

The GPU tests compare BITS: `adam_restated.emulate` performs the documented operations in numpy
float32, and the kernel — elementwise, no atomics, no contraction, IEEE division and square root,
denormals kept — must reproduce it exactly.  The CPU tests tie that emulation to Adam: it holds a
derived rounding bound against a float64 evaluation, the float64 evaluation equals
torch.optim.Adam in float64, and every input set the GPU tests use tells the emulation from the
plausible wrong kernels.
"""
import collections
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import adam_restated as R

F = np.float32
Hyper = collections.namedtuple("Hyper", "lr beta1 beta2 eps step grad_scale")
T = collections.namedtuple("T", "p g m v half")          # flat fp32 arrays; half: does it own an f16 copy
Case = collections.namedtuple("Case", "name hyper tensors blind")

GUARD = 64                                                # sentinel elements behind every array
SENT32 = np.array([0xDEADBEEF], np.uint32).view(np.int32)[0]      # -6.26e18 as a float: finite, unlike any state
SENT16 = np.int16(0x7BCD)                                 # 63 904 as a half
VARIANTS = ("contracted_m", "eps_in_sqrt", "bc2_on_v", "scale_dropped", "half_from_old_p", "beta2_step_minus_1")


def _hyper_coef(hy):
    return R.coef(hy.lr, hy.beta1, hy.beta2, hy.step)


# ---------------------------------------------------------------------------------------------
# input sets (numpy, deterministic): shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------

def _states(n, rng, lo=-6.0, hi=3.0, zero_frac=0.1):
    """p, g, m of either sign and v >= 0 with magnitudes 10^[lo, hi]; m = v = 0 on zero_frac of the
    elements (entries whose first gradient arrives now)."""
    def mag():
        return 10.0 ** rng.uniform(lo, hi, n)

    def sgn():
        return np.where(rng.random(n) < 0.5, -1.0, 1.0)
    p, g, m, v = (sgn() * mag()).astype(F), (sgn() * mag()).astype(F), (sgn() * mag()).astype(F), mag().astype(F)
    fresh = rng.random(n) < zero_frac
    m[fresh] = 0
    v[fresh] = 0
    return p, g, m, v


SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 12288 + 1027]


@functools.lru_cache(None)
def sizes_case():
    """Whole chunks, the per-trip path and the scalar tail, with and without an f16 copy in turn."""
    rng = np.random.default_rng(11)
    ts = [T(*_states(n, rng), half=(i % 2 == 0)) for i, n in enumerate(SIZES)]
    return Case("sizes", Hyper(2.5e-3, 0.9, 0.99, 1e-15, 3, 1.0 / 2500), ts, frozenset())


HYPER_GRID = [Hyper(3e-3, b1, b2, eps, step, gs)
              for step in (1, 2, 7, 1000, 10 ** 6)
              for (b1, b2) in ((0.9, 0.99), (0.9, 0.999), (0.0, 0.5))
              for eps in (1e-15, 1e-8)
              for gs in (1.0, 1.0 / 4096, 1.0 / 2500, 16.0 * 4096)]


@functools.lru_cache(None)
def hyper_tensors():
    rng = np.random.default_rng(12)
    return [T(*_states(1025, rng), half=False), T(*_states(4097, rng), half=True)]


def _blind_by_construction(hy):
    """The variants a set of hyper-parameters cannot tell from the kernel, whatever the states."""
    blind = set()
    if F(hy.grad_scale) == 1:
        blind.add("scale_dropped")                       # nothing to drop
    if _bc2_variant(hy) == R.coefficients(hy.lr, hy.beta1, hy.beta2, hy.step)[1]:
        blind.add("beta2_step_minus_1")                  # beta2^step and beta2^(step-1) both vanish beside 1
    if F(1.0 - math.pow(float(F(hy.beta2)), float(hy.step))) == 1:
        blind.add("bc2_on_v")                            # the bias correction is 1 wherever it is applied
    # the smallest v' the states of `_states` (magnitudes >= 1e-6) can give: a fresh entry's (1 - beta2) (s g)^2
    # or an old one's beta2 v; an eps below half an ulp of it is as invisible under the root as beside it
    omb2 = float(F(1) - F(hy.beta2))
    if hy.eps < 2.0 ** -25 * min(omb2 * (float(F(hy.grad_scale)) * 1e-6) ** 2, float(F(hy.beta2)) * 1e-6):
        blind.add("eps_in_sqrt")
    return frozenset(blind)


def hyper_cases():
    return [Case("hyper%r" % (tuple(hy),), hy, hyper_tensors(), _blind_by_construction(hy)) for hy in HYPER_GRID]


@functools.lru_cache(None)
def idle_case():
    """g = m = v = 0 on whole 4-groups (idle: nothing is stored) and on one, two or three elements of
    others (not idle: all four are stored); a group with g = m = 0 but v != 0 (not idle); the ragged
    last group idle on one tensor and half-zeroed on another."""
    rng = np.random.default_rng(13)
    ts = []
    for n, half, tail in ((4096 + 1024 + 6, True, "idle"), (8192, True, None), (4096 + 7, False, "one"), (7, True, "idle")):
        p, g, m, v = _states(n, rng)
        for k in range((n + 3) // 4):
            i = 4 * k
            kind = k % 10
            if kind in (0, 5):
                g[i:i + 4] = m[i:i + 4] = v[i:i + 4] = 0                 # idle
            elif kind in (1, 2, 3):
                g[i:i + kind] = m[i:i + kind] = v[i:i + kind] = 0        # 1, 2 or 3 elements: the group is live
            elif kind == 9:
                g[i:i + 4] = m[i:i + 4] = 0                              # v alone keeps it live; p' = p there
        last = 4 * ((n - 1) // 4)
        if tail == "idle":
            g[last:] = m[last:] = v[last:] = 0
        elif tail == "one":
            p2, g2, m2, v2 = _states(n - last, rng, zero_frac=0.0)
            g[last:], m[last:], v[last:] = g2, m2, v2
            g[last] = m[last] = v[last] = 0
        ts.append(T(p, g, m, v, half))
    return Case("idle", Hyper(1e-3, 0.9, 0.99, 1e-15, 5, 1.0 / 4096), ts, frozenset())


GRID_SIZES = [3 * 4096 + 5, 4097, 8192, 100]              # 4 + 2 + 2 + 1 = 9 chunks


@functools.lru_cache(None)
def grid_case():
    rng = np.random.default_rng(14)
    ts = [T(*_states(n, rng), half=(i % 2 == 1)) for i, n in enumerate(GRID_SIZES)]
    return Case("grid", Hyper(1e-3, 0.9, 0.99, 1e-15, 2, 1.0 / 2500), ts, frozenset())


F16_TARGETS = [65504.0, float(np.nextafter(F(65520), F(0))), 65520.0, 1e5, 2.0 ** -24, 2.0 ** -25,
               2.0 ** -25 * (1 + 2.0 ** -10), -0.0]


@functools.lru_cache(None)
def f16_case():
    """p' landing exactly on the edges of the half format.  A live element with g = m = 0 has m' = 0 and
    p' = p - step_size * (0 / denom) = p, so p' IS the target (the test asserts it); its float
    neighbours and its negative go the same way, and further copies take a real update of +-lr from the
    target, which moves them across the rounding boundaries of the half."""
    p = []
    for t in F16_TARGETS:
        t = F(t)
        p += [t, np.nextafter(t, F(np.inf)), np.nextafter(t, F(-np.inf)), -t]
    exact = len(p)
    p = np.array(p + p + p, F)
    n = p.size
    g, m, v = np.zeros(n, F), np.zeros(n, F), np.ones(n, F)
    g[exact:2 * exact] = 1e-3                            # |upd| ~ lr: a real step down
    g[2 * exact:] = -30.0                                # ... and up
    v[exact:] = 0
    # once in a whole chunk (behind healthy states), once as a small tensor that ends in a ragged group
    rng = np.random.default_rng(15)
    big = [np.concatenate([x, y]) for x, y in zip((p, g, m, v), _states(4096 - n, rng))]
    pad = [np.concatenate([x, y]) for x, y in zip((p, g, m, v), _states(3, rng))]
    ts = [T(*big, half=True), T(*pad, half=True)]
    # for the half copy: the elements that cross a half rounding boundary tell it from half(old p)
    return Case("f16_edges", Hyper(1e-3, 0.9, 0.99, 1e-15, 4, 1.0), ts,
                frozenset({"scale_dropped"})), exact


@functools.lru_cache(None)
def denormal_case():
    """Gradients of 1e-20 .. 1e-23 on fresh entries: (1 - beta2) g^2 = 1e-42 .. 1e-48 is denormal or zero
    in float, its square root is normal again.  Excluded from the float64 bound (which assumes no
    underflow); bit equality holds under the kernel's denormal mode (denormals kept, as numpy keeps them)."""
    rng = np.random.default_rng(16)
    n = 4096 + 1024 + 3
    p = (rng.standard_normal(n)).astype(F)
    g = (np.where(rng.random(n) < 0.5, -1, 1) * 10.0 ** rng.uniform(-23, -20, n)).astype(F)
    m, v = np.zeros(n, F), np.zeros(n, F)
    old = rng.random(n) < 0.3                            # some with denormal moments already
    v[old] = (10.0 ** rng.uniform(-44, -39, int(old.sum()))).astype(F)
    m[old] = (10.0 ** rng.uniform(-44, -39, int(old.sum()))).astype(F)
    return Case("denormal", Hyper(1e-3, 0.9, 0.99, 1e-15, 2, 1.0), [T(p, g, m, v, True)], frozenset(VARIANTS))


@functools.lru_cache(None)
def nonfinite_case():
    """One NaN, one +Inf and one -Inf gradient, each alone in a 4-group of healthy elements: in whole
    chunks (first trip, second trip, second chunk) and in three ragged last groups."""
    rng = np.random.default_rng(17)
    big = list(_states(8192 + 3, rng))
    where = {"big": [(5, np.nan), (1024 + 6, np.inf), (4096 + 2048 + 3, -np.inf), (8192 + 1, np.nan)]}
    big[1][[i for i, _ in where["big"]]] = [x for _, x in where["big"]]
    ts = [T(*big, half=True)]
    for bad, half in ((np.inf, False), (-np.inf, True)):
        s = list(_states(7, rng))
        s[1][5] = bad
        ts.append(T(*s, half=half))
    return Case("nonfinite", Hyper(1e-3, 0.9, 0.99, 1e-15, 3, 1.0 / 4096), ts, frozenset())


TRAJ_SHAPES = [(3, 1000, 2), (4097,), (1,), (64, 66)]
TRAJ_HALF = (0, 3)
TRAJ_STEPS = 40


@functools.lru_cache(None)
def trajectory():
    """The schedule of tests/test_optim.py::test_fused_adam_matches_torch_adam (warm-up, a decay step, a power of
    ten per tensor and step, every second column zeroed on some iterations) with a gradient scale on some
    steps; rows 60.. of the last tensor never receive a gradient.  Returns the initial parameters and per step
    (Hyper, gradients, [(p, m, v, h) expected after the step])."""
    rng = np.random.default_rng(18)
    init = [rng.standard_normal(s).astype(F) for s in TRAJ_SHAPES]
    state = [(x.ravel().copy(), np.zeros(x.size, F), np.zeros(x.size, F), x.ravel().astype(np.float16)) for x in init]
    steps = []
    for it in range(TRAJ_STEPS):
        lr = 1e-3 * (0.5 if it >= 15 else 1.0) * min(1.0, it / 5.0)
        gs = 1.0 / 2500 if it % 3 == 1 else (16.0 * 4096 if it % 5 == 0 else 1.0)
        hy = Hyper(lr, 0.9, 0.99, 1e-15, it + 1, gs)
        grads, after = [], []
        for s, st in zip(TRAJ_SHAPES, state):
            gr = (rng.standard_normal(s) * 10.0 ** int(rng.integers(-6, 2))).astype(F)
            if it % 7 == 3:
                gr[..., ::2] = 0
            if s == (64, 66):
                gr[60:] = 0
            grads.append(gr)
            p, m, v, h = st
            after.append(R.emulate(p, gr.ravel(), m, v, _hyper_coef(hy), hy.eps, hy.grad_scale, h=h))
        steps.append((hy, grads, after, state))
        state = after
    return init, steps


CTL_STEPS = (1, 7, 1000, 10 ** 6)
CTL_LR = 1.2345e-3


def ctl_cases():
    return [Case("ctl%d" % s, Hyper(CTL_LR, 0.9, 0.99, 1e-15, s, 1.0 / 4096), hyper_tensors(),
                 _blind_by_construction(Hyper(CTL_LR, 0.9, 0.99, 1e-15, s, 1.0 / 4096))) for s in CTL_STEPS]


def single_step_cases():
    """Every input set a GPU test hands to one launch."""
    return [sizes_case(), idle_case(), grid_case(), f16_case()[0], denormal_case(), nonfinite_case()] \
        + hyper_cases() + ctl_cases()


# ---------------------------------------------------------------------------------------------
# the emulation of a case, and the wrong kernels
# ---------------------------------------------------------------------------------------------

def _h0(t):
    return np.full(t.p.size, SENT16, np.int16).view(np.float16)


def _emulate_case(case, c=None):
    hy = case.hyper
    c = c or _hyper_coef(hy)
    return [R.emulate(t.p, t.g, t.m, t.v, c, hy.eps, hy.grad_scale, h=_h0(t)) for t in case.tensors]


def _bc2_variant(hy):
    bc2 = 1.0 - math.pow(float(F(hy.beta2)), float(hy.step - 1))
    return F(1.0 / math.sqrt(bc2)) if bc2 > 0 else F(np.inf)


def _step32(t, h, hy, kind=None):
    """The float32 step once more, with one deviation `kind` of VARIANTS (None: none — equals emulate)."""
    c = _hyper_coef(hy)
    s = F(1) if kind == "scale_dropped" else F(hy.grad_scale)
    ibc = _bc2_variant(hy) if kind == "beta2_step_minus_1" else c.inv_bc2_sqrt
    eps, b1, b2 = F(hy.eps), c.beta1, c.beta2
    omb1, omb2 = F(1) - b1, F(1) - b2
    with np.errstate(all="ignore"):
        gk = t.g * s
        m1 = b1 * t.m + omb1 * gk if kind == "contracted_m" else t.m + omb1 * (gk - t.m)
        v1 = t.v * b2 + (omb2 * gk) * gk
        if kind == "eps_in_sqrt":
            denom = np.sqrt(v1 + eps) * ibc
        elif kind == "bc2_on_v":
            bc2 = F(1.0 - math.pow(float(b2), float(hy.step)))
            denom = np.sqrt(v1 / bc2) + eps
        else:
            denom = np.sqrt(v1) * ibc + eps
        p1 = t.p - c.step_size * (m1 / denom)
        idle = R.idle_elements(t.g, t.m, t.v)
        p1, m1, v1 = np.where(idle, t.p, p1), np.where(idle, t.m, m1), np.where(idle, t.v, v1)
        h1 = np.where(idle, h, (t.p if kind == "half_from_old_p" else p1).astype(np.float16))
    return p1, m1, v1, h1


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    assert a.dtype == b.dtype and a.size == b.size, (a.dtype, b.dtype, a.size, b.size)
    na, nb = np.isnan(a), np.isnan(b)
    iv = np.int32 if a.dtype == np.float32 else np.int16
    return (na == nb) & (na | (a.view(iv) == b.view(iv)))


def _differs(x, y, halves):
    """Do two results (p, m, v, h) of one tensor differ in a bit (the f16 copy counts where there is one)?"""
    return any(not _same_bits(a, b).all() for a, b in list(zip(x, y))[:4 if halves else 3])


def _caught(case):
    """The variants that differ from the emulation somewhere in the case."""
    hy = case.hyper
    out = set()
    for t in case.tensors:
        h = _h0(t)
        good = R.emulate(t.p, t.g, t.m, t.v, _hyper_coef(hy), hy.eps, hy.grad_scale, h=h)
        assert not _differs(good, _step32(t, h, hy), True)               # the switchboard itself is the emulation
        out |= {k for k in VARIANTS if _differs(good, _step32(t, h, hy, k), t.half)}
    return out


# ---------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------

def test_numpy_keeps_float_denormals():
    """The emulation relies on it (a library built with fast-math can switch the process to flush-to-zero)."""
    x = F(1e-20) * F(1e-20)
    assert x > 0 and x < F(2.0 ** -126) and np.sqrt(x) * np.sqrt(x) > 0


def _check_bound(tag, t, hy):
    c = _hyper_coef(hy)
    got = R.emulate(t.p, t.g, t.m, t.v, c, hy.eps, hy.grad_scale)
    ref, err = R.reference(t.p, t.g, t.m, t.v, c, hy.eps, hy.grad_scale)
    idle = R.idle_elements(t.g, t.m, t.v)
    worst = 0.0
    for name, a, r, e in zip("pmv", got, ref, err):
        ok = np.isfinite(r) & np.isfinite(e)             # (the non-finite set: its healthy elements)
        assert ok.sum() >= ok.size - 4 and np.isfinite(a[ok]).all(), (tag, name)
        d = np.abs(a[ok].astype(np.float64) - r[ok])
        assert (d <= e[ok]).all(), (tag, name, float((d / np.maximum(e[ok], 1e-300)).max()))
        live = ok & ~idle & (e > 0)
        if live.any():
            worst = max(worst, float((np.abs(a[live].astype(np.float64) - r[live]) / e[live]).max()))
    return worst


def test_emulation_holds_the_float64_bound():
    """Every input set of the GPU tests but the denormal one (the bound assumes that no product, quotient
    or square root underflows: asserted here for the sets that are run)."""
    worst = {}
    for case in single_step_cases():
        if case.name == "denormal":
            continue
        hy = case.hyper
        for i, t in enumerate(case.tensors):
            fin = np.isfinite(t.g)
            small = R.smallest_normal_margin(t.p[fin], t.g[fin], t.m[fin], t.v[fin], _hyper_coef(hy), hy.eps, hy.grad_scale)
            assert small >= 2.0 ** -126, (case.name, i, small)
            key = case.name.split("(")[0]
            worst[key] = max(worst.get(key, 0.0), _check_bound((case.name, i), t, hy))
    _, steps = trajectory()
    for hy, grads, _, before in steps:
        for i, (gr, st) in enumerate(zip(grads, before)):
            t = T(st[0], gr.ravel(), st[1], st[2], False)
            assert R.smallest_normal_margin(t.p, t.g, t.m, t.v, _hyper_coef(hy), hy.eps, hy.grad_scale) >= 2.0 ** -126
            worst["trajectory"] = max(worst.get("trajectory", 0.0), _check_bound(("trajectory", hy.step, i), t, hy))
    print("largest |emulation - float64| / bound:", {k: round(x, 4) for k, x in worst.items()})
    assert max(worst.values()) > 0.5          # the bound is not slack: some element comes within a factor 2 of it


def test_float64_reference_is_adam():
    """`reference` with double coefficients (1 / (1 - beta^t) formed in double) against torch.optim.Adam on
    float64 CPU parameters, 10 steps, both running free from the same start.

    Allowed difference: float64 rounding.  Per step each of the two evaluations lies within the bound
    formula at u = 2^-53 of the exact step (torch: lerp, mul + addcmul, sqrt / sqrt(bc2) + eps, addcdiv — the
    same count of roundings per quantity in another order), so the two differ by at most twice the formula;
    1 / sqrt(bc2) carries two roundings of its own and torch's sqrt(bc2) one, which the formula (coefficients
    are inputs to it) does not count: 3 u |upd| more.  Over the steps the differences carry over — to first
    order, m' = beta1 m + ..: D_m' = beta1 D_m + d_m;  D_v' = beta2 D_v + d_v;
    D_p' = D_p + d_p + step_size D_m' / denom + |upd| D_v' / (2 v')  (the last: the relative change of
    sqrt(v'), which bounds that of denom as eps >= 0).  Second-order terms are 2^-53 of these and are
    covered by rounding every factor up by 1e-6."""
    rng = np.random.default_rng(3)
    n = 3000
    p0 = rng.standard_normal(n)
    b1, b2, eps, lr = 0.9, 0.99, 1e-15, 1e-3
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=0.0)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    Dp, Dm, Dv = np.zeros(n), np.zeros(n), np.zeros(n)
    u = R.U64
    for step in range(1, 11):
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2, n)
        if step % 3 == 0:
            g[::2] = 0
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        c = R.Coef(lr / (1.0 - b1 ** step), b1, b2, 1.0 / math.sqrt(1.0 - b2 ** step))
        (p, m, v), (ep, em, ev) = R.reference(p, g, m, v, c, eps, 1.0, u=u)
        denom = np.sqrt(v) * c.inv_bc2_sqrt + eps
        upd = np.abs(c.step_size * m / denom)
        k = 1 + 1e-6
        Dm = k * (b1 * Dm + 2 * em)
        Dv = k * (b2 * Dv + 2 * ev)
        Dp = k * (Dp + 2 * ep + 3 * u * upd + c.step_size * Dm / denom + upd * Dv / (2 * v))
        st = opt.state[q]
        for name, mine, theirs, D in (("p", p, q.detach().numpy(), Dp), ("m", m, st["exp_avg"].numpy(), Dm),
                                     ("v", v, st["exp_avg_sq"].numpy(), Dv)):
            assert (np.abs(mine - theirs) <= D).all(), (step, name, float(np.abs(mine - theirs).max()))
    # rounding-sized (10 steps x 2 x u |p|, |p| < 5, is 1e-14) against ten real updates of lr each
    assert float(Dp.max()) < 2e-14 and float(np.abs(p - p0).max()) > 5e-3


def test_inputs_discriminate():
    """On every input set of the GPU tests each wrong kernel that the set's hyper-parameters can expose at all
    (`blind`: derived from the hyper-parameters alone) differs from the emulation in at least one bit."""
    for case in single_step_cases():
        # sizes, idle, grid, hyper*, ctl*: there for all six variants (ragged tails and whole chunks alike);
        # nonfinite: all six, on its healthy neighbours
        # f16_edges: there for half_from_old_p and the rounding of the copy (its grad_scale is 1);
        # denormal: there for the build's denormal mode, not for a variant (all `blind`)
        must = set(VARIANTS) - case.blind
        missed = must - _caught(case)
        assert not missed, (case.name, missed)
    assert "half_from_old_p" in _caught(f16_case()[0])
    # the trajectory: each variant shows in at least one single step from the chain's own states, and the half
    # copy and the contracted moment in every step after the warm-up's lr = 0.  (The variants that move the
    # denominator by an ulp show only where |upd| is not small beside ulp(p), eps only while a second moment
    # is still small beside it: not in every step.)
    _, steps = trajectory()
    seen = set()
    for hy, grads, _, before in steps:
        case = Case("traj", hy, [T(st[0], gr.ravel(), st[1], st[2], i in TRAJ_HALF)
                                 for i, (gr, st) in enumerate(zip(grads, before))], None)
        got = _caught(case)
        seen |= got
        if hy.step > 1:
            assert {"contracted_m", "half_from_old_p"} <= got, (hy.step, got)
    assert seen == set(VARIANTS), set(VARIANTS) - seen


def test_f16_targets_are_reached_exactly():
    """The edge set's first block lands on its targets in the emulation, and numpy rounds them to half as
    IEEE round-to-nearest-even does."""
    case, exact = f16_case()
    for t, res in zip(case.tensors, _emulate_case(case)):
        assert np.array_equal(res[0][:exact].view(np.int32), t.p[:exact].view(np.int32))
        h = dict(zip([float(x) for x in t.p[:exact]], res[3][:exact]))
        assert h[65504.0] == 65504 and h[float(np.nextafter(F(65520), F(0)))] == 65504      # below the tie: largest half
        assert np.isposinf(h[65520.0]) and np.isposinf(h[float(F(1e5))]) and np.isneginf(h[-65520.0])   # the tie goes to even = overflow
        assert h[2.0 ** -24] == 2.0 ** -24 and h[2.0 ** -25] == 0 and h[2.0 ** -25 * (1 + 2.0 ** -10)] == 2.0 ** -24
        hz = res[3][:exact]                                # the last target's block: -0.0, its neighbours, +0.0
        assert hz[-4] == 0 and np.signbit(hz[-4]) and hz[-1] == 0 and not np.signbit(hz[-1])   # zeros keep their signs


def test_argument_checks():
    """Every refusal of the three entry points comes before any launch: no GPU needed."""
    from volsurfs_amd import _lib
    from volsurfs_amd.trainer import TrainCtl
    L = _lib.lib()
    null, f = ctypes.c_void_p(0), ctypes.c_float
    some = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))         # never dereferenced
    ctl_obj = TrainCtl()
    ctl = ctypes.c_void_p(ctypes.addressof(ctl_obj))
    ERR, OK = -1, 0

    def shared(desc=some, ck=some, n=3, b1=0.9, b2=0.99, step=1, wg=0):
        return L.vsa_adam_step_shared(desc, ck, n, f(1e-3), f(b1), f(b2), f(1e-15), step, f(1.0), 1, wg, null)

    def plain(desc=some, ck=some, n=3, b1=0.9, b2=0.99, step=1):
        return L.vsa_adam_step(desc, ck, n, f(1e-3), f(b1), f(b2), f(1e-15), step, f(1.0), 1, null)

    def by_ctl(desc=some, ck=some, n=3, b1=0.9, b2=0.99, wg=0, c=ctl):
        return L.vsa_adam_step_ctl(desc, ck, n, f(b1), f(b2), f(1e-15), f(1.0), 1, wg, c, null)

    for step in (0, -1, -2 ** 31):
        assert shared(step=step) == ERR and plain(step=step) == ERR
    for bad in (1.0, 1.5, -0.1, float("nan"), float("inf"), -float("inf")):
        for fn in (shared, plain, by_ctl):
            assert fn(b1=bad) == ERR and fn(b2=bad) == ERR, (fn.__name__, bad)
    assert shared(wg=-1) == ERR and by_ctl(wg=-1) == ERR
    assert shared(wg=-1, n=0) == ERR and by_ctl(wg=-1, n=0) == ERR
    for fn in (shared, plain, by_ctl):
        assert fn(n=-1) == ERR
        assert fn(desc=null) == ERR and fn(ck=null) == ERR and fn(desc=null, ck=null) == ERR
        assert fn(n=0) == OK and fn(n=0, desc=null, ck=null) == OK
    assert by_ctl(c=null) == ERR and by_ctl(c=null, n=0) == ERR
    assert plain(step=0, n=0) == ERR                                                   # as tests/test_optim.py has it


# ---------------------------------------------------------------------------------------------
# GPU harness: every array in its own sentinel-filled allocation, one launch for all tensors
# ---------------------------------------------------------------------------------------------

class Launch:
    """The device side of a case: per tensor five allocations of n + GUARD elements filled with a sentinel, the
    arrays copied to their heads; descriptors and chunk list as the entry points read them."""

    def __init__(self, tensors, chunk_order=None):
        self.tensors = tensors
        self.bufs = []
        for t in tensors:
            n = t.p.size
            b = {k: torch.full((n + GUARD,), int(SENT32), dtype=torch.int32, device="cuda") for k in "pgmv"}
            b["h"] = torch.full((n + GUARD,), int(SENT16), dtype=torch.int16, device="cuda") if t.half else None
            self.bufs.append(b)
        self.reset()
        entries = [tuple(b[k].data_ptr() for k in "pgmv") + (b["h"].data_ptr() if b["h"] is not None else None, t.p.size)
                   for t, b in zip(tensors, self.bufs)]
        self.desc = torch.frombuffer(bytearray(R.descriptors(entries)), dtype=torch.uint8).cuda()
        ck = R.chunk_list([t.p.size for t in tensors], chunk=R.CHUNK)
        if chunk_order is not None:
            ck = ck[chunk_order]
        assert all(0 <= c * R.CHUNK < tensors[i].p.size for i, c in ck)     # no chunk past a tensor's end
        self.nr_chunks = len(ck)
        self.chunks = torch.from_numpy(np.ascontiguousarray(ck)).cuda()

    def reset(self):
        for t, b in zip(self.tensors, self.bufs):
            n = t.p.size
            for k, a in zip("pgmv", (t.p, t.g, t.m, t.v)):
                b[k].fill_(int(SENT32))
                b[k][:n] = torch.from_numpy(a.view(np.int32).copy()).cuda()
            if b["h"] is not None:
                b["h"].fill_(int(SENT16))

    def run(self, hy, zero_grads=1, max_workgroups=None, ctl=None):
        from volsurfs_amd import _lib
        assert _lib.lib().vsa_adam_chunk_elems() == R.CHUNK
        sp = _lib.stream_ptr()
        if ctl is not None:
            _lib.call("vsa_adam_step_ctl", self.desc, self.chunks, self.nr_chunks, hy.beta1, hy.beta2, hy.eps,
                      hy.grad_scale, zero_grads, max_workgroups or 0, ctl, sp)
        elif max_workgroups is None:
            _lib.call("vsa_adam_step", self.desc, self.chunks, self.nr_chunks, hy.lr, hy.beta1, hy.beta2, hy.eps,
                      hy.step, hy.grad_scale, zero_grads, sp)
        else:
            _lib.call("vsa_adam_step_shared", self.desc, self.chunks, self.nr_chunks, hy.lr, hy.beta1, hy.beta2,
                      hy.eps, hy.step, hy.grad_scale, zero_grads, max_workgroups, sp)
        torch.cuda.synchronize()
        out = []
        for b in self.bufs:
            o = {k: b[k].cpu().numpy().view(np.float32) for k in "pgmv"}
            o["h"] = b["h"].cpu().numpy().view(np.float16) if b["h"] is not None else None
            out.append(o)
        return out


def _assert_bits(got, want, what):
    ok = _same_bits(got, want)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError("%s: %d of %d elements differ, first at %d: got %r, expected %r"
                             % (what, int((~ok).sum()), ok.size, i, got.ravel()[i], want.ravel()[i]))


def _check_launch(case, out, zero_grads=1, expected=None, tag=""):
    """Heads equal the emulation, guards untouched, gradient cleared (or kept), f16 copies as emulated."""
    expected = expected or _emulate_case(case)
    for i, (t, o, e) in enumerate(zip(case.tensors, out, expected)):
        n = t.p.size
        what = "%s%s tensor %d (n = %d)" % (case.name, tag, i, n)
        for k, want in zip("pmv", e):
            _assert_bits(o[k][:n], want, what + " " + k)
        idle = R.idle_elements(t.g, t.m, t.v)
        _assert_bits(o["g"][:n], np.where(idle | (not zero_grads), t.g, F(0)), what + " grad")
        for k in "pgmv":
            assert (o[k][n:].view(np.int32) == SENT32).all(), what + ": wrote behind the end of " + k
        if t.half:
            _assert_bits(o["h"][:n], e[3], what + " f16 copy")
            assert (o["h"][n:].view(np.int16) == SENT16).all(), what + ": wrote behind the end of the f16 copy"


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("zero_grads", [1, 0])
def test_sizes_and_paths(zero_grads):
    """n = 1 .. 13 315 in one launch of vsa_adam_step: whole chunks, per-trip groups, scalar tails; the 64
    elements behind every array keep their sentinel; the gradient is cleared, or with zero_grads = 0 kept."""
    case = sizes_case()
    _check_launch(case, Launch(case.tensors).run(case.hyper, zero_grads=zero_grads), zero_grads=zero_grads)


@pytest.mark.gpu
def test_hyper_parameters():
    """step x betas x eps x grad_scale (120 launches of 5 122 elements), each bit-equal to the emulation."""
    launch = Launch(hyper_tensors())
    for k, case in enumerate(hyper_cases()):
        if k:
            launch.reset()
        _check_launch(case, launch.run(case.hyper))


@pytest.mark.gpu
def test_idle_groups_are_not_stored():
    """A 4-group with g = m = v = 0 keeps p, m, v and — none of the five stores being issued — whatever its
    f16 copy held; every other group is written in full, its zero-gradient elements included."""
    case = idle_case()
    out = Launch(case.tensors).run(case.hyper)
    _check_launch(case, out)
    for t, o in zip(case.tensors, out):                   # once more without the emulation's help
        n = t.p.size
        idle = R.idle_elements(t.g, t.m, t.v)
        assert 0.15 * n < idle.sum() < 0.3 * n or n == 7
        for k, a in zip("pmv", (t.p, t.m, t.v)):
            assert np.array_equal(o[k][:n][idle].view(np.int32), a[idle].view(np.int32))
        if t.half:
            assert (o["h"][:n][idle].view(np.int16) == SENT16).all()
            assert (o["h"][:n][~idle].view(np.int16) != SENT16).all()
        live_zero = ~idle & (t.g == 0) & (t.m == 0) & (t.v == 0)       # zeroed elements of live groups: p' = p, written
        assert live_zero.sum() >= 1 or n == 7                            # (the 7-element tensor is idle as a whole)
        assert np.array_equal(o["p"][:n][live_zero].view(np.int32), t.p[live_zero].view(np.int32))
        if t.half:
            assert np.array_equal(o["h"][:n][live_zero].view(np.int16), t.p[live_zero].astype(np.float16).view(np.int16))
    tails = [(t.p.size, R.idle_groups(t.g, t.m, t.v)[-1]) for t in case.tensors]
    assert tails == [(4096 + 1024 + 6, True), (8192, False), (4096 + 7, False), (7, True)]     # ragged last groups: idle, -, live, idle


@pytest.mark.gpu
def test_bounded_grid_visits_every_chunk_once():
    """vsa_adam_step_shared over 9 chunks from 1 .. 90 workgroups, and with the chunk list permuted: every run
    equals the emulation of ONE step (a chunk skipped shows as no step, one done twice as a second step)."""
    case = grid_case()
    expected = _emulate_case(case)
    launch = Launch(case.tensors)
    assert launch.nr_chunks == 9
    for k, wg in enumerate((0, 1, 2, 3, 8, 9, 10, 90)):
        if k:
            launch.reset()
        _check_launch(case, launch.run(case.hyper, max_workgroups=wg), expected=expected, tag=" max_workgroups=%d" % wg)
    order = np.random.default_rng(5).permutation(9)
    assert (order != np.arange(9)).any()
    for wg in (2, 4):
        _check_launch(case, Launch(case.tensors, chunk_order=order).run(case.hyper, max_workgroups=wg),
                      expected=expected, tag=" permuted, max_workgroups=%d" % wg)


@pytest.mark.gpu
def test_f16_copy_at_the_edges_of_half():
    """p' on 65504, around 65520 (the overflow tie), 1e5, 2^-24, 2^-25 (a tie to zero), just above it and -0.0:
    the copy is the round-to-nearest-even conversion, infinities and signed zeros included."""
    case, _ = f16_case()
    _check_launch(case, Launch(case.tensors).run(case.hyper))


@pytest.mark.gpu
def test_denormal_second_moments():
    """v' denormal: equality holds under the kernel's denormal mode (denormals kept).  A mismatch here is a
    finding about the build flags, not a tolerance to widen."""
    case = denormal_case()
    e = _emulate_case(case)[0]
    tiny = (e[2] > 0) & (e[2] < F(2.0 ** -126))
    assert tiny.sum() > 1000 and (e[2] == 0).sum() > 100         # denormal v', and some flushed by the arithmetic itself
    _check_launch(case, Launch(case.tensors).run(case.hyper))


@pytest.mark.gpu
def test_nonfinite_gradient_stays_in_its_element():
    """A NaN / +Inf / -Inf gradient makes its own element non-finite exactly where the emulation's is; the
    three neighbours of its 4-group (whole chunk or scalar tail) equal the emulation like everything else."""
    case = nonfinite_case()
    out = Launch(case.tensors).run(case.hyper)
    _check_launch(case, out)
    for t, o in zip(case.tensors, out):
        bad = ~np.isfinite(t.g)
        n = t.p.size
        assert bad.sum() in (1, 4)
        assert np.isnan(o["p"][:n][bad]).all() and np.isfinite(o["p"][:n][~bad]).all()
        assert not np.isfinite(o["m"][:n][bad]).any() and np.isfinite(o["m"][:n][~bad]).all()
        assert not np.isfinite(o["v"][:n][bad]).any() and np.isfinite(o["v"][:n][~bad]).all()
        assert (o["g"][:n] == 0).all()


def _run_trajectory(make_opt, step_fn):
    init, steps = trajectory()
    ps = [torch.nn.Parameter(torch.from_numpy(x.copy()).cuda()) for x in init]
    halves = {ps[i]: ps[i].detach().half() for i in TRAJ_HALF}
    opt = make_opt(ps, halves)
    for p in ps:
        p.grad = torch.zeros_like(p)
    for hy, grads, after, _ in steps:
        opt.param_groups[0]["lr"] = hy.lr
        for p, gr in zip(ps, grads):
            p.grad += torch.from_numpy(gr).cuda()                            # accumulate, as autograd does
        opt.mark_grads_dirty()
        step_fn(opt, hy.grad_scale)
        torch.cuda.synchronize()
        assert opt.param_groups[0]["step"] == hy.step
        for i, (p, e) in enumerate(zip(ps, after)):
            what = "step %d tensor %d" % (hy.step, i)
            st = opt.state[p]
            _assert_bits(p.detach().cpu().numpy(), e[0], what + " p")
            _assert_bits(st["exp_avg"].cpu().numpy(), e[1], what + " m")
            _assert_bits(st["exp_avg_sq"].cpu().numpy(), e[2], what + " v")
            if p in halves:
                _assert_bits(halves[p].cpu().numpy(), e[3], what + " f16 copy")
            assert not p.grad.view(-1).view(torch.int32).any(), what + " gradient not cleared"
        assert opt.grads_are_clean()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["FusedAdam", "side_stream", "ShardedFusedAdam"])
def test_trajectory_through_the_classes(how):
    """40 steps of the schedule of test_fused_adam_matches_torch_adam: after every step the parameters, both
    moments and the f16 copies equal the chain of emulated steps bit for bit and the gradients are zero."""
    from volsurfs_amd import optim
    kw = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
    if how == "ShardedFusedAdam":
        _run_trajectory(lambda ps, hs: optim.ShardedFusedAdam(ps, 1, 0, half_copies=hs, **kw),
                        lambda opt, gs: opt.step(grad_scale=gs))
    elif how == "side_stream":
        side = torch.cuda.Stream()

        def make(ps, hs):
            opt = optim.FusedAdam(ps, half_copies=hs, **kw)
            opt.shared_workgroups = 3                     # 7 chunks: the strided walk
            return opt
        _run_trajectory(make, lambda opt, gs: torch.cuda.current_stream().wait_event(opt.step(grad_scale=gs, stream=side)))
    else:
        _run_trajectory(lambda ps, hs: optim.FusedAdam(ps, half_copies=hs, **kw), lambda opt, gs: opt.step(grad_scale=gs))


def _ctl_bytes(adam_step, adam_lr, adam_pending):
    from volsurfs_amd.trainer import TrainCtl
    ctl = TrainCtl()
    ctl.iter, ctl.nr_rays, ctl.capacity = 3, 1, 1
    ctl.adam_step, ctl.adam_lr, ctl.adam_pending = adam_step, adam_lr, adam_pending
    return torch.frombuffer(bytearray(bytes(ctl)), dtype=torch.uint8).cuda()


def _ulp_neighbours(x):
    return [np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))]


@pytest.mark.gpu
@pytest.mark.parametrize("step", CTL_STEPS)
def test_control_block_entry(step):
    """vsa_adam_step_ctl forms step_size and inv_bc2_sqrt on the device with its own double pow, which may differ
    from the host's in the last place of a double: either float may be one float ulp from `coefficients`.  There
    is exactly ONE such pair under which the whole launch — every element of every tensor — equals the emulation."""
    case = [c for c in ctl_cases() if c.hyper.step == step][0]
    hy = case.hyper
    out = Launch(case.tensors).run(hy, max_workgroups=2, ctl=_ctl_bytes(step, CTL_LR, 1))
    s0, i0 = R.coefficients(hy.lr, hy.beta1, hy.beta2, hy.step)
    matched = []
    for ds, s in zip((-1, 0, 1), _ulp_neighbours(s0)):
        for di, ibc in zip((-1, 0, 1), _ulp_neighbours(i0)):
            e = _emulate_case(case, R.Coef(s, F(hy.beta1), F(hy.beta2), ibc))
            if all(_same_bits(o[k][:t.p.size], x).all() for t, o, x3 in zip(case.tensors, out, e)
                   for k, x in zip("pmv", x3)):
                matched.append(((ds, di), e))
    print("vsa_adam_step_ctl step %d: (step_size, inv_bc2_sqrt) ulps from the host's = %s" % (step, [m[0] for m in matched]))
    assert len(matched) == 1, [m[0] for m in matched]
    _check_launch(case, out, expected=matched[0][1], tag=" pair %s" % (matched[0][0],))


@pytest.mark.gpu
@pytest.mark.parametrize("adam_step,pending", [(5, 0), (0, 1), (-3, 1)])
def test_control_block_entry_without_a_pending_update(adam_step, pending):
    """adam_pending = 0 (the first replay) or no step yet: every buffer keeps its bits — the gradient under
    zero_grads = 1 and the f16 sentinel too."""
    case = ctl_cases()[0]
    out = Launch(case.tensors).run(case.hyper, max_workgroups=2, ctl=_ctl_bytes(adam_step, CTL_LR, pending))
    for t, o in zip(case.tensors, out):
        n = t.p.size
        for k, a in zip("pgmv", (t.p, t.g, t.m, t.v)):
            assert np.array_equal(o[k][:n].view(np.int32), a.view(np.int32)) and (o[k][n:].view(np.int32) == SENT32).all()
        if t.half:
            assert (o["h"].view(np.int16) == SENT16).all()
