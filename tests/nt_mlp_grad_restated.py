"""Float64 restatement of the neural-texture MLP backward (csrc/nt_mlp.hip: nt_mlp_bwd_pc_kernel, entry point
vsa_nt_mlp_bwd), the condition under which the kernel's fp32 arithmetic is exact, and independent packers for
the two layouts the kernel reads and writes.  CPU only (numpy); used by tests/test_nt_mlp_grad.py.

One texture: features X [n, 32] (feature k = 2 level + j), gradient rows G [n, C], weights W1 [64, 32],
W2 [64, 64], W3 [32, 64] (rows >= C zero), all f16.  `mlp_backward_f64` walks the kernel's chain in float64 and
rounds to f16 exactly where the kernel converts to `_Float16`:

    H1 = f16(relu(W1 X))      H2 = f16(relu(W2 H1))      out = f16(W3 H2)
    dOut = G                                  (row_format 2: raw rows, bit for bit)
         = f16(G (s - s^2)), s = sigmoid(out) (row_formats 0 and 1)
    dH2 = f16(where(H2 > 0, W3^T dOut, 0))    dH1 = f16(where(H1 > 0, W2^T dH2, 0))    dX = W1^T dH1
    dW3 = sum dOut H2^T (rows < C)    dW2 = sum dH2 H1^T    dW1 = sum dH1 X^T     (x weight_grad_scale)
    dabs[f] = sum over slots |dX[f]|, of the UNROUNDED dX

THE ReLU RULE.  The kernel lets a gradient pass where the recomputed ReLU output has non-zero bits: the
derivative at a pre-activation of exactly 0 (and at one that rounds to 0 in f16) is 0.  `where(H > 0, ., 0)` on
the f16 activations says the same; the select also keeps a non-finite gradient out of a masked element, as the
kernel's integer multiply by min(bits, 1) does.

EXACTNESS.  With small integers (or small multiples of a power of two) every f16 product is exact in fp32 and an
fp32 sum whose terms are all multiples of a quantum q and whose sum of magnitudes A satisfies A / q < 2^24 is
exact in every order: every partial sum is a multiple of q below 2^24 q.  `Restated.A[name]` and
`Restated.q[name]` hold A and a lower bound of q per output element (the smallest quantum of the left operand's
row times that of the right operand's column, over their non-zero entries: never above the smallest quantum
among the terms, so the condition asked is never weaker than the true one).  `assert_exact` checks it for every
accumulator of a case.
"""
import numpy as np

MAX_DEG = 4
N_LEVELS = 16
FBLOCK = 256                         # slots per block of the feature planes
ROW_QUADS = (2, 4, 8, 8)             # quads (4 elements) of one slot's row, per degree
ALPHA_QUAD = (1, 3, 4, 6)            # first quad of the alpha coefficients in such a row
WEIGHTS_PER_TEX = 8192
W1_OFF, W2_OFF, W3_OFF = 0, 2048, 6144
F16_U = 2.0 ** -11                   # unit roundoff of f16
EXACT_LIMIT = 2.0 ** 24


def f16(x):
    """Round-to-nearest-even to f16, returned as float64 (overflow goes to inf, as v_cvt_f16_f32 does)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def quantum(x):
    """Per element: the largest power of two that divides x (inf for 0 and for non-finite x)."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(np.where(np.isfinite(x), x, 0.0))
    im = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = (im & -im).astype(np.float64)
    with np.errstate(over="ignore"):
        q = low * np.exp2((e - 53).astype(np.float64))
    return np.where(im == 0, np.inf, q)


def _matmul_aq(a, b):
    """a @ b in float64 with, per output element, A = |a| @ |b| and the lower bound of the terms' quantum."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = a @ b
        A = np.abs(a) @ np.abs(b)
    q = quantum(a).min(axis=1, initial=np.inf)[:, None] * quantum(b).min(axis=0, initial=np.inf)[None, :]
    return v, A, q


class Restated:
    """What mlp_backward_f64 returns.  Activations and gradients are float64 arrays holding f16 values (dX:
    the unrounded value, dX16 its f16 rounding); dW1 [64, 32], dW2 [64, 64], dW3 [C, 64] and dabs [32] are float64.
    A / q: dicts over 'pre1', 'pre2', 'pre3', 'dH2', 'dH1', 'dX', 'dW1', 'dW2', 'dW3', 'dabs' (see the module
    docstring); `pre` holds the unrounded accumulator values of 'pre1', 'pre2', 'pre3', 'dH2', 'dH1' and 'dX'."""


def mlp_backward_f64(w1, w2, w3, X, G, C, row_format, weight_grad_scale):
    w1, w2, w3 = (np.asarray(w, np.float64) for w in (w1, w2, w3))
    X, G = np.asarray(X, np.float64), np.asarray(G, np.float64)
    n = X.shape[0]
    assert w1.shape == (64, 32) and w2.shape == (64, 64) and w3.shape == (32, 64)
    assert X.shape == (n, 32) and G.shape == (n, C) and 0 < C <= 32
    assert not w3[C:].any(), "rows >= C of W3 are zero"
    r = Restated()
    r.A, r.q, r.pre = {}, {}, {}

    def layer(name, a, b):
        v, r.A[name], r.q[name] = _matmul_aq(a, b)
        r.pre[name] = v
        return v

    # forward recompute; a zero of the ReLU is +0 (the kernel takes the maximum on the bit patterns)
    r.H1 = f16(np.maximum(layer("pre1", X, w1.T), 0.0)) + 0.0
    r.H2 = f16(np.maximum(layer("pre2", r.H1, w2.T), 0.0)) + 0.0
    r.out = f16(layer("pre3", r.H2, w3[:C].T))
    if row_format == 2:
        r.dOut = G.copy()
    else:
        s = 1.0 / (1.0 + np.exp(-r.out))
        r.dOut = f16(G * (s - s * s))
    with np.errstate(invalid="ignore"):
        r.dH2 = f16(np.where(r.H2 > 0, layer("dH2", r.dOut, w3[:C]), 0.0))
        r.dH1 = f16(np.where(r.H1 > 0, layer("dH1", r.dH2, w2), 0.0))
        r.dX = layer("dX", r.dH1, w1)
    r.dX16 = f16(r.dX)
    gs = float(weight_grad_scale)
    for name, a, b in (("dW3", r.dOut, r.H2), ("dW2", r.dH2, r.H1), ("dW1", r.dH1, X)):
        v, A, q = _matmul_aq(a.T, b)
        setattr(r, name, v * gs)
        r.A[name], r.q[name] = A * gs, q * gs
    with np.errstate(invalid="ignore"):
        r.dabs = np.abs(r.dX).sum(axis=0)
    r.A["dabs"] = r.dabs.copy()
    r.q["dabs"] = quantum(r.dX).min(axis=0, initial=np.inf)
    return r


# ---------------------------------------------------------------- the bank's bookkeeping, restated

class Layout:
    """Texture indices, channel counts, slot capacity and row bases of a NeuralTextureBank, from its
    constructor arguments alone (texture x = (shell * 2 + type) * 4 + degree; type 0 colour, 1 alpha)."""

    def __init__(self, K, max_rays, sh_degree=3, alpha_sh_degree=3, textures_res=(64, 32, 16, 8),
                 inner_solid=False, shared_rgb=False, shared_alpha=False):
        self.K, self.max_rays, self.tex_res = K, max_rays, tuple(textures_res)
        self.rgb_degrees, self.alpha_degrees = sh_degree + 1, alpha_sh_degree + 1
        self.D = max(self.rgb_degrees, self.alpha_degrees)
        self.inner_solid, self.shared = bool(inner_solid), (bool(shared_rgb), bool(shared_alpha))
        self.n_tex = K * 2 * MAX_DEG
        self.seg_capacity, self.row_base = [], []
        quads, cap = 0, 0
        for s in range(K):
            for d in range(MAX_DEG):
                self.row_base.append(quads)
                c = min(4 * max_rays, (self.tex_res[d] + 2) ** 2) if d < self.D else 0
                self.seg_capacity.append(c)
                cap += c
                quads += (c * ROW_QUADS[d] + 7) // 8 * 8
        self.row_base.append(quads)
        self.row_quads_total = quads
        self.slot_capacity = (cap + FBLOCK - 1) // FBLOCK * FBLOCK + FBLOCK

    def kwargs(self):
        """The NeuralTextureBank constructor arguments this layout stands for."""
        return dict(nr_shells=self.K, max_rays=self.max_rays, sh_degree=self.rgb_degrees - 1,
                    alpha_sh_degree=self.alpha_degrees - 1, textures_res=self.tex_res, inner_solid=self.inner_solid,
                    shared_rgb=self.shared[0], shared_alpha=self.shared[1])

    @staticmethod
    def split(x):
        return x // (2 * MAX_DEG), (x // MAX_DEG) & 1, x % MAX_DEG       # shell, type, degree

    def channels(self, x):
        shell, typ, deg = self.split(x)
        if typ == 0:
            return 3 * (2 * deg + 1) if deg < self.rgb_degrees else 0
        if self.inner_solid and (shell == 0 or self.shared[1]):
            return 0
        return 2 * deg + 1 if deg < self.alpha_degrees else 0

    def param_tex(self, x):
        return x % (2 * MAX_DEG) if self.shared[(x // MAX_DEG) & 1] else x

    @staticmethod
    def own_quads(x):
        """(first quad, number of quads) of a slot's row that belong to texture x."""
        _, typ, deg = Layout.split(x)
        return (ALPHA_QUAD[deg], ROW_QUADS[deg] - ALPHA_QUAD[deg]) if typ else (0, ALPHA_QUAD[deg])


# ---------------------------------------------------------------- packers

def pack_features(dense):
    """[2, capacity, 32] (type, slot, feature 2 level + j) -> the blocked planes [2, capacity / 256, 16, 256, 2]."""
    t, cap, f = dense.shape
    assert t == 2 and f == 2 * N_LEVELS and cap % FBLOCK == 0
    out = np.empty((2, cap // FBLOCK, N_LEVELS, FBLOCK, 2), dense.dtype)
    for typ in range(2):
        for blk in range(cap // FBLOCK):
            for lvl in range(N_LEVELS):
                out[typ, blk, lvl] = dense[typ, blk * FBLOCK:(blk + 1) * FBLOCK, 2 * lvl:2 * lvl + 2]
    return out


def unpack_features(planes):
    """The inverse of pack_features."""
    t, blocks, lv, fb, two = planes.shape
    assert (t, lv, fb, two) == (2, N_LEVELS, FBLOCK, 2)
    out = np.empty((2, blocks * FBLOCK, 2 * N_LEVELS), planes.dtype)
    for typ in range(2):
        for blk in range(blocks):
            for lvl in range(N_LEVELS):
                out[typ, blk * FBLOCK:(blk + 1) * FBLOCK, 2 * lvl:2 * lvl + 2] = planes[typ, blk, lvl]
    return out


def rows_slice(layout, seg, x):
    """(offset, n, stride, width) in ELEMENTS of texture x's own quads in the flat row buffer: slot i of its
    segment owns elements offset + i * stride ... + width."""
    shell, typ, deg = Layout.split(x)
    sd = shell * MAX_DEG + deg
    q0, nq = Layout.own_quads(x)
    return layout.row_base[sd] * 4 + q0 * 4, seg[sd + 1] - seg[sd], ROW_QUADS[deg] * 4, nq * 4


def pack_rows(layout, seg, per_tex, fill, dtype=np.uint16):
    """Flat row buffer [row_quads_total * 4]: `fill` everywhere, then per_tex[x] [n, own quads * 4] (own
    elements of every slot of x's segment; columns >= channels are the row's padding) for the textures given."""
    out = np.full(layout.row_quads_total * 4, fill, dtype)
    for x, rows in per_tex.items():
        off, n, stride, width = rows_slice(layout, seg, x)
        assert rows.shape == (n, width), (x, rows.shape, n, width)
        out[off + np.arange(n)[:, None] * stride + np.arange(width)[None, :]] = rows
    return out


def unpack_rows(layout, seg, flat, x):
    """Texture x's own elements [n, own quads * 4] out of the flat row buffer."""
    off, n, stride, width = rows_slice(layout, seg, x)
    return flat[off + np.arange(n)[:, None] * stride + np.arange(width)[None, :]]


def unpack_weights(w):
    return w[W1_OFF:W2_OFF].reshape(64, 32), w[W2_OFF:W3_OFF].reshape(64, 64), w[W3_OFF:].reshape(32, 64)


# ---------------------------------------------------------------- a whole launch

class Case:
    """Everything one launch of vsa_nt_mlp_bwd reads.  layout; seg [4 K + 1] slot starts; weights [n_tex, 8192]
    float64 holding f16 values; X {x: [n, 32]}, G {x: [n, own quads * 4]} (f16 values; columns >= channels are
    padding the kernel reads but must not let through) for every active texture with a non-empty segment;
    prefill [n_tex, 8192] float32, the weight-gradient buffer before the launch; grad_scale; row_format."""

    def __init__(self, layout, seg, weights, X, G, prefill, grad_scale, row_format=2):
        self.layout, self.seg, self.weights, self.X, self.G = layout, [int(s) for s in seg], weights, X, G
        self.prefill, self.grad_scale, self.row_format = prefill, float(grad_scale), row_format
        assert len(self.seg) == layout.K * MAX_DEG + 1
        for sd in range(layout.K * MAX_DEG):
            assert 0 <= self.seg[sd + 1] - self.seg[sd] <= layout.seg_capacity[sd], "segment beyond its capacity"
        assert self.seg[-1] <= layout.slot_capacity - FBLOCK

    def textures(self):
        return sorted(self.X)

    def slots(self, x):
        shell, _, deg = Layout.split(x)
        return self.seg[shell * MAX_DEG + deg], self.seg[shell * MAX_DEG + deg + 1]


def restate_case(case):
    """{x: Restated} for every texture of the case."""
    lay, out = case.layout, {}
    for x in case.textures():
        C = lay.channels(x)
        w1, w2, w3 = unpack_weights(case.weights[lay.param_tex(x)])
        out[x] = mlp_backward_f64(w1, w2, w3, case.X[x], case.G[x][:, :C], C, case.row_format, 1.0 / case.grad_scale)
    return out


def weight_grad_sums(case, res):
    """Per parameter texture p: (S, A, q), each [8192] float64 — the restated gradient summed over ALL logical
    textures that share p (rows >= C of W3: S = A = 0, q = inf), its sum of magnitudes and quantum bound."""
    lay, out = case.layout, {}
    for x, r in res.items():
        p, C = lay.param_tex(x), lay.channels(x)
        if p not in out:
            out[p] = (np.zeros(WEIGHTS_PER_TEX), np.zeros(WEIGHTS_PER_TEX), np.full(WEIGHTS_PER_TEX, np.inf))
        S, A, q = out[p]
        for name, off, size in (("dW1", W1_OFF, 2048), ("dW2", W2_OFF, 4096), ("dW3", W3_OFF, C * 64)):
            S[off:off + size] += getattr(r, name).ravel()
            A[off:off + size] += r.A[name].ravel()
            q[off:off + size] = np.minimum(q[off:off + size], r.q[name].ravel())
    return out


def expected_weight_grads(case, res):
    """(expected, no_terms): the weight-gradient buffer after the launch, float64 — prefill + restated sum —
    and the entries that receive no non-zero term at all (A = 0: untouched rows included).  Those keep their
    BITS: every workgroup's partial sum is 0 and the kernel skips v == 0.  An entry whose terms cancel to 0 keeps
    its VALUE (p + a - a = p exactly) but not the sign of a -0: whether its partial sums are non-zero depends on
    which workgroup owns which tile."""
    exp = case.prefill.astype(np.float64)
    no_terms = np.ones(exp.shape, bool)
    for p, (S, A, _) in weight_grad_sums(case, res).items():
        live = A != 0
        with np.errstate(invalid="ignore"):
            exp[p][live] = exp[p][live] + S[live]
        no_terms[p] = ~live
    return exp, no_terms


class NotExact(AssertionError):
    pass


def _check_sum(what, A, q):
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(A == 0, 0.0, A / q)
    if not (ratio < EXACT_LIMIT).all():
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise NotExact("%s: sum of |terms| / quantum = %g >= 2^24 at %s" % (what, ratio[i], (i,)))


def _check_f16(what, v):
    """v is handed on as f16: f16-exact, or an fp32-exact value inside the f16 range (one unambiguous rounding)."""
    v = np.asarray(v, np.float64)
    ok = (f16(v) == v) | ((v.astype(np.float32).astype(np.float64) == v) & (np.abs(v) < 65520.0))
    if not ok.all():
        i = np.unravel_index(np.argmin(ok), ok.shape)
        raise NotExact("%s: %r at %s is neither f16-exact nor an fp32-exact value in range" % (what, v[i], (i,)))


def assert_exact(case, res=None):
    """Raise NotExact unless no fp32 accumulator of the launch can round: the precondition of the bit-for-bit
    comparison.  Weight gradients: over all slots of all shells that share the parameter row, the pre-filled
    value included (the flushes are fp32 adds into it)."""
    res = restate_case(case) if res is None else res
    for x, r in res.items():
        handed = {"pre1": np.maximum(r.pre["pre1"], 0), "pre2": np.maximum(r.pre["pre2"], 0),
                  "dH2": np.where(r.H2 > 0, r.pre["dH2"], 0), "dH1": np.where(r.H1 > 0, r.pre["dH1"], 0),
                  "dX": r.pre["dX"]}
        if case.row_format != 2:                       # raw rows: the network output is formed but not used
            handed["pre3"] = r.pre["pre3"]
        for name in ("pre1", "pre2", "pre3", "dH2", "dH1", "dX", "dabs"):
            _check_sum("texture %d %s" % (x, name), r.A[name], r.q[name])
        for name, v in handed.items():
            _check_f16("texture %d %s" % (x, name), v)
    for p, (S, A, q) in weight_grad_sums(case, res).items():
        live = W3_OFF + case.layout.channels(p) * 64            # (rows >= C of W3 are never added to)
        pre = case.prefill[p, :live].astype(np.float64)
        _check_sum("parameter texture %d weight gradient" % p, A[:live] + np.abs(pre), np.minimum(q[:live], quantum(pre)))


# ---------------------------------------------------------------- comparison helpers

def bits_zero_normalised(a):
    """Integer view of a float array with -0 mapped to +0 and nothing else changed."""
    a = np.ascontiguousarray(a)
    iv = a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
    iv[a == 0] = 0
    return iv
