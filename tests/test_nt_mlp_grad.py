"""The neural-texture MLP backward (csrc/nt_mlp.hip: nt_mlp_bwd_pc_kernel, entry point vsa_nt_mlp_bwd) on its
own, against the float64 restatement of nt_mlp_grad_restated.mlp_backward_f64.  The test writes everything the
kernel reads on a NeuralTextureBank — seg_start, the feature planes, the weights, the gradient rows and
weights.grad — and calls only bank.backward_mlp: no trace, mark / compact, encode (leg B excepted), shade.

LEG A, bit for bit.  With raw rows (row_format 2) the kernel takes dOut = G as it stands, and with features and
gradient rows that are integers in [-2, 2] and weights from {-1, 0, 1} 2^-k (k = 0, 1, 2) every f16 product is
exact in fp32, every fp32 sum is exact in any order (R.assert_exact checks sum |terms| / quantum < 2^24 for every
accumulator of every case, on the CPU) and every conversion to f16 is a no-op or one rounding of an exact value.
The four outputs — dF (written over `features`), weights.grad, dfeat_abs_sum and the cleared grad_rows — are
then independent of summation order, atomic order and work split and must equal the restatement BIT FOR BIT.
No tolerance appears anywhere in leg A.

Zeros.  The kernel's zeros are +0: a masked gradient is the bit pattern 0, and an fp32 sum that starts from +0
and is rounded to nearest never yields -0.  A float64 product or BLAS sum may yield -0, so the comparison maps
-0 to +0 on both sides, for zeros only; every other element is compared by its bits.  weights.grad entries that
receive no non-zero term (the kernel skips a sum v == 0) are compared by their raw bits, -0 included: the
pre-filled buffer holds some.  An entry whose terms cancel to 0 over the whole texture keeps its value, but a
pre-filled -0 may come out as +0 there: the workgroups that share the texture add their non-zero partial sums
one after the other (-0 + a - a = +0).

Sentinels.  Every buffer is filled with a NaN bit pattern (f16 0x7e5a, f32 0x7fc5a5a5) before the inputs are
written, so the whole-buffer comparison also shows that nothing is written (and, through the NaN, that nothing
is read into a result) outside: feature planes of slots past the segments and of the other type where that
texture is inactive, gradient rows past a segment's end and of inactive textures, weights.grad of inactive
textures, of the non-owning shells of a shared model and of W3's rows >= C.  The padding elements INSIDE a
texture's own quads (row elements >= C, which the kernel does read) hold small integers: they meet W3's zero
rows and must not reach any flushed output.

Width instances.  The producer's tile loop is compiled for 1-4 groups of 8 output channels and the consumer's
for 1 or 2 k-steps.  sh_degree = alpha_sh_degree = 3 gives C = 3, 9, 15, 21 (colour: 1, 2, 2, 3 groups; 1, 1, 1, 2
k-steps) and 1, 3, 5, 7 (alpha: one group).  The producer's fourth instance (more than 24 channels) cannot be
reached: the widest texture any configuration builds has 21.  No shape is invented for it.

Trips.  A wave pair handles 32 slots, four pairs make one trip of 128, and the hand-off buffers alternate with
the trip number.  In a small frame the work split (nt_for_each_piece: one workgroup per CU) hands every
workgroup about one tile, so trips beyond the first and the wrap of the buffer index need ONE long texture:
see _long_layout for the length derived from the split rule.

LEG B, rounding.  Leg A never runs dOut = G sigmoid'(out) (hardware exp2 / rcp, mixed-precision FMAs that round
straight to f16) nor ordinary rounding.  Leg B runs row_formats 0 and 1 on data at the bank's own scale
against the same restatement.  Its constants are measured on the MI355X and asserted at twice the measured
maximum, the margin this suite uses for measured parity constants; the cap on the share of dF elements more
than one f16 ulp off (1 %) is a cap, not a measurement.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import nt_mlp_grad_restated as R

SENT16, SENT32 = 0x7E5A, 0x7FC5A5A5
GRAD_SCALE = 128.0
MI355X_CUS = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- cases

def _sparse(rng, shape, density):
    """{-1, 0, 1} 2^-k, k in {0, 1, 2}: asymmetric in sign, size and position."""
    v = rng.choice([-1.0, 1.0], shape) * np.exp2(-rng.integers(0, 3, shape))
    return v * (rng.random(shape) < density)


def _make_case(layout, seg_len, seed, dens=(1 / 8, 1 / 8, 1 / 2), g_density=1.0, row_format=2):
    rng = np.random.default_rng(seed)
    seg = np.concatenate([[0], np.cumsum(seg_len)])
    weights = np.zeros((layout.n_tex, R.WEIGHTS_PER_TEX))
    prefill = np.full((layout.n_tex, R.WEIGHTS_PER_TEX), SENT32, np.uint32)
    X, G = {}, {}
    for x in range(layout.n_tex):
        C = layout.channels(x)
        if C == 0:
            continue
        if layout.param_tex(x) == x:                 # a shell that reads shell 0's shared model owns no rows
            w3 = np.zeros((32, 64))
            w3[:C] = _sparse(rng, (C, 64), dens[2])
            weights[x] = np.concatenate([_sparse(rng, (64, 32), dens[0]).ravel(),
                                         _sparse(rng, (64, 64), dens[1]).ravel(), w3.ravel()])
            # exact, non-zero accumulation targets: multiples of 1/8, a few -0 among them
            pre = rng.integers(-3, 4, R.W3_OFF + C * 64).astype(np.float32) / 8
            pre[rng.random(pre.size) < 0.05] = -0.0
            prefill[x, :pre.size] = pre.view(np.uint32)
        shell, _, deg = R.Layout.split(x)
        n = int(seg_len[shell * R.MAX_DEG + deg])
        if n == 0:
            continue
        X[x] = rng.integers(-2, 3, (n, 32)).astype(np.float64)
        g = rng.integers(-2, 3, (n, R.Layout.own_quads(x)[1] * 4)).astype(np.float64)
        G[x] = g * (rng.random(g.shape) < g_density)
    return R.Case(layout, seg, weights, X, G, prefill.view(np.float32), GRAD_SCALE, row_format)


def _pc_run_cost():
    src = open(os.path.join(ROOT, "volsurfs_amd", "csrc", "nt_mlp.hip")).read()
    return int(re.search(r"#define NT_PC_RUN_COST (\d+)", src).group(1))


def _long_layout(n_cus, degree):
    """ONE active texture (K = 1, inner_solid: no alpha; every segment but `degree`'s empty) long enough that a
    workgroup's piece makes three trips, so that the `it & 1` buffer index wraps.
    nt_for_each_piece lays the launch on one axis: NT_PC_RUN_COST units of spacing per non-empty texture, then
    one unit per 32-slot tile, and cuts it evenly over n_cus workgroups (a fresh bank has no measured balance).
    With T tiles a workgroup's stretch is (cost + T) / n_cus units; a tile belongs to the workgroup whose
    stretch holds its start, so a stretch of s units past the spacing holds at least floor(s) >= 9 tiles once
    (cost + T) / n_cus >= 10: T = 10 n_cus - cost, iters = ceil(tiles / 4) = 3 for 9-12 tiles (the first workgroup
    loses the spacing).  The last tile holds ONE slot: n = 32 T - 31.  256 CUs: T = 2486, n = 79 521 slots,
    10 MB of feature planes.  Returns (layout, segment lengths)."""
    cost = _pc_run_cost()
    T = 10 * n_cus - cost
    assert (cost + T) // n_cus >= 10
    n = 32 * T - 31
    res = [8, 8, 8, 8]
    res[degree] = 512
    assert (res[degree] + 2) ** 2 >= n
    lay = R.Layout(1, (n + 3) // 4, sh_degree=degree, alpha_sh_degree=0, textures_res=res, inner_solid=True)
    seg_len = [0, 0, 0, 0]
    seg_len[degree] = n
    return lay, seg_len


SMALL = dict(max_rays=1200, textures_res=(64, 32, 16, 8))          # segment capacities 4356, 1156, 324, 100

# name -> (layout, segment lengths, seed, keyword arguments of _make_case).  The lengths 1, 31, 32, 33, 127, 128,
# 129, 257 are spread over the degrees (257 and 129: a lone slot in the third / second trip's tile range); `edges_b`
# has an empty segment between non-empty ones.
CASES = {
    "widths_a": lambda n_cus: (R.Layout(1, **SMALL), [257, 129, 127, 33], 1, {}),
    "edges_b": lambda n_cus: (R.Layout(1, **SMALL), [1, 0, 128, 32], 2, {}),
    "edges_c": lambda n_cus: (R.Layout(1, **SMALL), [31, 33, 129, 1], 3, {}),
    "long_deg0": lambda n_cus: _long_layout(n_cus, 0) + (4, {}),
    # (21 channels over 80 000 slots: sparser rows and W3 keep sum |dF| below 2^24 quanta)
    "long_deg3": lambda n_cus: _long_layout(n_cus, 3) + (5, dict(dens=(1 / 8, 1 / 8, 1 / 4), g_density=1 / 4)),
    "shared": lambda n_cus: (R.Layout(2, shared_rgb=True, shared_alpha=True, **SMALL),
                             [65, 40, 33, 9, 130, 0, 31, 64], 6, {}),
    "independent": lambda n_cus: (R.Layout(3, **SMALL), [40, 33, 0, 7, 1, 70, 32, 31, 129, 5, 64, 2], 7, {}),
    "inner_solid": lambda n_cus: (R.Layout(2, inner_solid=True, **SMALL), [70, 33, 40, 9, 50, 31, 0, 12], 8, {}),
}


@functools.lru_cache(maxsize=None)
def _case(name, n_cus=MI355X_CUS):
    lay, seg_len, seed, kw = CASES[name](n_cus)
    case = _make_case(lay, seg_len, seed, **kw)
    return case, R.restate_case(case)


# ---------------------------------------------------------------- buffers before and after

def _bits16(v):
    return np.asarray(v, np.float64).astype(np.float16).view(np.uint16)


def _buffers(case, res):
    """(inputs, expected outputs) of the launch as whole buffers: `features` [2, capacity, 32] u16 bits (dense;
    pack_features lays them out), `rows` flat u16 bits, `wgrad` [n_tex, 8192] f32, `dabs` [n_tex, 32] f32 and
    `touched`, the weights.grad entries that receive a non-zero term (all others keep their raw bits)."""
    lay = case.layout
    f_in = np.full((2, lay.slot_capacity, 32), SENT16, np.uint16)
    f_out = f_in.copy()
    dabs = np.zeros((lay.n_tex, 32), np.float32)
    for x in case.textures():
        a, b = case.slots(x)
        typ = R.Layout.split(x)[1]
        f_in[typ, a:b] = _bits16(case.X[x])
        with np.errstate(invalid="ignore"):
            f_out[typ, a:b] = _bits16(res[x].dX16)
            dabs[x] = res[x].dabs.astype(np.float32)
    rows_in = R.pack_rows(lay, case.seg, {x: _bits16(case.G[x]) for x in case.textures()}, SENT16)
    rows_out = R.pack_rows(lay, case.seg, {x: np.zeros_like(case.G[x], np.uint16) for x in case.textures()}, SENT16)
    exp, no_terms = R.expected_weight_grads(case, res)
    touched = ~no_terms
    wgrad = case.prefill.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        wgrad[touched] = exp[touched].astype(np.float32)
    ins = dict(features=f_in, rows=rows_in, wgrad=case.prefill)
    return ins, dict(features=f_out, rows=rows_out, wgrad=wgrad, dabs=dabs, touched=touched)


def _new_bank(case):
    from volsurfs_amd.neural_textures import NeuralTextureBank
    lay, fmt = case.layout, case.row_format
    bank = NeuralTextureBank(device="cuda", quantize_output=fmt == 0, squeeze_output=fmt != 2, **lay.kwargs())
    # the restated bookkeeping is the bank's
    assert bank.row_format == fmt and bank.slot_capacity == lay.slot_capacity
    assert bank.row_quads_total == lay.row_quads_total
    assert [int(bank.plan.row_base[i]) for i in range(lay.K * R.MAX_DEG + 1)] == lay.row_base
    assert all(bank.tex_channels(x) == lay.channels(x) and bank.param_tex(x) == lay.param_tex(x)
               for x in range(lay.n_tex))
    return bank


def _load(bank, case, ins):
    """Steps 1-5 of driving the kernel alone: segment starts, feature planes, weights, gradient rows, weights.grad."""
    with torch.no_grad():
        bank.seg_start.copy_(torch.tensor(case.seg, dtype=torch.int32))
        bank.features.view(torch.int16).copy_(torch.from_numpy(R.pack_features(ins["features"]).view(np.int16)))
        bank.weights.copy_(torch.from_numpy(case.weights.astype(np.float32)))
        bank.refresh_half_params()
        assert torch.equal(bank.weights_h.cpu().double(), torch.from_numpy(case.weights))
        bank.grad_rows.view(torch.int16).copy_(torch.from_numpy(ins["rows"].view(np.int16)))
        bank.weights.grad = torch.from_numpy(ins["wgrad"].copy()).cuda()


def _read(bank):
    torch.cuda.synchronize()
    return dict(features=R.unpack_features(bank.features.view(torch.int16).cpu().numpy().view(np.uint16)),
                rows=bank.grad_rows.view(torch.int16).cpu().numpy().view(np.uint16),
                wgrad=bank.weights.grad.cpu().numpy(), dabs=bank._dfsum.cpu().numpy())


def _run(case, ins):
    bank = _new_bank(case)
    _load(bank, case, ins)
    bank.backward_mlp(case.grad_scale)
    return bank, _read(bank)


def _where(case, key, idx):
    """A readable place for an offending element of buffer `key`."""
    if key == "features":
        typ, slot, f = idx
        sd = int(np.searchsorted(case.seg, slot, side="right")) - 1
        if sd >= len(case.seg) - 1:
            return "type %d slot %d (past the last segment) feature %d" % (typ, slot, f)
        shell, deg = divmod(sd, R.MAX_DEG)
        return "texture %d (shell %d type %d degree %d) slot %d (%d of its segment) level %d feature %d" % (
            (shell * 2 + typ) * R.MAX_DEG + deg, shell, typ, deg, slot, slot - case.seg[sd], f // 2, f % 2)
    if key == "wgrad":
        x, i = idx
        for name, off, cols in (("W3", R.W3_OFF, 64), ("W2", R.W2_OFF, 64), ("W1", R.W1_OFF, 32)):
            if i >= off:
                return "texture %d d%s[%d][%d]" % (x, name, (i - off) // cols, (i - off) % cols)
    if key == "dabs":
        return "texture %d feature %d" % idx
    return "element %d" % idx


def _assert_bits(case, key, got, ref, raw=None):
    """got == ref bit for bit, -0 taken for +0 (module docstring); `raw`: a mask of elements compared by their
    raw bits instead."""
    if got.dtype.kind == "f":
        g, r = R.bits_zero_normalised(got), R.bits_zero_normalised(ref)
        if raw is not None:
            g[raw], r[raw] = got.view(g.dtype)[raw], ref.view(r.dtype)[raw]
    else:
        g, r = got, ref
    bad = np.argwhere(g != r)
    if len(bad):
        as_f = (lambda a, i: float(a.view(np.float16)[i])) if got.dtype == np.uint16 else (lambda a, i: float(a[i]))
        lines = ["%s: kernel %r (0x%x), restated %r (0x%x)" % (_where(case, key, tuple(int(j) for j in i)),
                                                                as_f(got, tuple(i)), int(g[tuple(i)]),
                                                                as_f(ref, tuple(i)), int(r[tuple(i)]))
                 for i in bad[:8]]
        raise AssertionError("%s: %d elements differ\n  " % (key, len(bad)) + "\n  ".join(lines))


def _assert_outputs(case, got, exp):
    _assert_bits(case, "features", got["features"], exp["features"])
    _assert_bits(case, "rows", got["rows"], exp["rows"])
    _assert_bits(case, "wgrad", got["wgrad"], exp["wgrad"], raw=~exp["touched"])
    _assert_bits(case, "dabs", got["dabs"], exp["dabs"])


# ---------------------------------------------------------------- CPU: the restatement, the packers, exactness

def test_restatement_equals_float64_autograd():
    """Integer data make the f16 roundings no-ops, so the chain is linear layers and ReLUs: dW and dX of the
    restatement equal torch's float64 autograd of sum(out * G) exactly, ReLU'(0) = 0 on both sides."""
    case, res = _case("widths_a")
    n_zero = 0
    for x in case.textures():
        C, r = case.layout.channels(x), res[x]
        w1, w2, w3 = (torch.tensor(w, dtype=torch.float64, requires_grad=True)
                      for w in R.unpack_weights(case.weights[x]))
        X = torch.tensor(case.X[x], requires_grad=True)
        G = torch.tensor(case.G[x][:, :C])
        pre1 = X @ w1.T
        h2 = torch.relu(torch.relu(pre1) @ w2.T)
        ((h2 @ w3[:C].T) * G).sum().backward()
        n_zero += int((pre1 == 0).sum())
        s = 1.0 / case.grad_scale
        assert np.array_equal(r.dX, X.grad.numpy()) and np.array_equal(r.dX16, X.grad.numpy())
        assert np.array_equal(r.dW1, w1.grad.numpy() * s) and np.array_equal(r.dW2, w2.grad.numpy() * s)
        assert np.array_equal(r.dW3, w3.grad.numpy()[:C] * s) and not w3.grad[C:].any()
        assert np.array_equal(r.dabs, X.grad.abs().sum(0).numpy())
        assert r.dW1.any() and r.dW2.any() and r.dW3.any() and r.dX.any()
    assert n_zero > 1000, "the integer data must hit pre-activations of exactly 0"


def test_restatement_sigmoid_branch():
    """Formats 0 and 1: dOut is G sigmoid'(out) rounded once to f16; format 2 hands G through."""
    rng = np.random.default_rng(0)
    w1, w2, w3 = (R.f16(rng.uniform(-0.45, 0.45, s)) for s in ((64, 32), (64, 64), (32, 64)))
    w3[9:] = 0
    X, G = R.f16(rng.normal(0, 1, (50, 32))), R.f16(rng.normal(0, 1, (50, 9)))
    r1, r2 = (R.mlp_backward_f64(w1, w2, w3, X, G, 9, f, 1.0) for f in (1, 2))
    assert np.array_equal(r2.dOut, G) and np.array_equal(r1.out, r2.out)
    s = 1 / (1 + np.exp(-r1.out))
    exact = G * s * (1 - s)
    assert (np.abs(r1.dOut - exact) <= np.abs(exact) * R.F16_U + 2.0 ** -25).all() and np.array_equal(r1.dOut, R.f16(r1.dOut))
    r0 = R.mlp_backward_f64(w1, w2, w3, X, G, 9, 0, 1.0)
    assert np.array_equal(r0.dW2, r1.dW2)


def test_packers_round_trip():
    rng = np.random.default_rng(1)
    dense = rng.integers(0, 65536, (2, 768, 32)).astype(np.uint16)
    planes = R.pack_features(dense)
    assert planes.shape == (2, 3, 16, 256, 2) and np.array_equal(R.unpack_features(planes), dense)
    for typ, slot, lvl, j in ((0, 0, 0, 0), (1, 255, 15, 1), (0, 256, 3, 0), (1, 700, 9, 1)):
        assert planes[typ, slot // 256, lvl, slot % 256, j] == dense[typ, slot, 2 * lvl + j]
    lay = R.Layout(2, inner_solid=True, **SMALL)
    seg = np.concatenate([[0], np.cumsum([5, 0, 3, 2, 4, 1, 0, 6])])
    active = [x for x in range(lay.n_tex) if lay.channels(x) and seg[x // 8 * 4 + x % 4 + 1] > seg[x // 8 * 4 + x % 4]]
    per = {x: rng.integers(1, 30000, (R.rows_slice(lay, seg, x)[1], R.Layout.own_quads(x)[1] * 4)).astype(np.uint16)
           for x in active}
    flat = R.pack_rows(lay, seg, per, SENT16)
    for x in active:
        assert np.array_equal(R.unpack_rows(lay, seg, flat, x), per[x])
    # the layout in words: slot i of segment (shell, d) starts at quad row_base + i ROW_QUADS(d); colour
    # coefficient c at element c, alpha coefficient c at element 4 ALPHA_QUAD(d) + c
    x = R.MAX_DEG * 3 + 3                                  # shell 1, alpha, degree 3
    assert flat[(lay.row_base[4 + 3] + 2 * 8 + 6) * 4 + 3] == per[x][2, 3]
    x = 3                                                  # shell 0, colour, degree 3
    assert flat[(lay.row_base[3] + 1 * 8) * 4 + 20] == per[x][1, 20]
    written = sum(p.size for p in per.values())
    assert (flat == SENT16).sum() == flat.size - written      # nothing else is touched (no value equals the fill)
    assert not any(4 <= x < 8 for x in active), "shell 0 of a solid inner mesh has no alpha texture"


@pytest.mark.parametrize("name", sorted(CASES))
def test_assert_exact_accepts(name):
    case, res = _case(name)
    R.assert_exact(case, res)
    if name.startswith("long"):
        (x,) = case.textures()
        a, b = case.slots(x)
        assert (b - a) % 32 == 1 and ((b - a + 31) // 32 + _pc_run_cost()) // MI355X_CUS >= 10


def test_assert_exact_rejects():
    """Too large in two ways: features of 11 significant bits under dense weights, and an accumulation target
    far above the gradient's quantum."""
    lay = R.Layout(1, **SMALL)
    case = _make_case(lay, [257, 129, 127, 33], 1, dens=(1.0, 1.0, 1.0))
    for x in case.X:
        case.X[x] = case.X[x] * 1023.0 + 1.0
    with pytest.raises(R.NotExact):
        R.assert_exact(case)
    case, res = _case("widths_a")
    R.assert_exact(case, res)
    big = R.Case(case.layout, case.seg, case.weights, case.X, case.G, case.prefill.copy(), case.grad_scale)
    big.prefill[0, 5] = 2.0 ** 22
    with pytest.raises(R.NotExact, match="weight gradient"):
        R.assert_exact(big, res)


# ---------------------------------------------------------------- GPU, leg A

def _n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _leg_a(name):
    case, res = _case(name, _n_cus())
    R.assert_exact(case, res)
    ins, exp = _buffers(case, res)
    bank, got = _run(case, ins)
    _assert_outputs(case, got, exp)
    return case, res, ins, exp, bank, got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["widths_a", "edges_b", "edges_c"])
def test_exact_every_width_and_tile_edge(name):
    """K = 1, all eight textures: every reachable width instance with its own asymmetric weights, segment
    lengths 1 ... 257, an empty segment; accumulation into a non-zero weights.grad; all sentinels."""
    case, res, ins, exp, bank, got = _leg_a(name)
    assert exp["touched"].any() and (~exp["touched"] & (ins["wgrad"].view(np.uint32) != SENT32)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["long_deg0", "long_deg3"])
def test_exact_three_trips_and_split_texture(name):
    """One texture over every workgroup, three trips each (_long_layout): the narrowest and the widest instance.
    Hundreds of workgroups flush partial sums of the same weight rows; exactness makes their order irrelevant."""
    _leg_a(name)


@pytest.mark.gpu
def test_exact_shared_models():
    """K = 2, one colour and one alpha model: both shells' sums land in shell 0's rows, shell 1's keep their
    sentinel bits, dfeat_abs_sum stays per logical texture."""
    case, res, ins, exp, bank, got = _leg_a("shared")
    assert exp["touched"][:8].any() and not exp["touched"][8:].any() and exp["dabs"][8:].any()


@pytest.mark.gpu
def test_exact_independent_shells():
    """K = 3: every shell's textures receive their own slots' contributions only."""
    _leg_a("independent")


@pytest.mark.gpu
def test_exact_inner_solid():
    """Shell 0 has no alpha texture: its alpha quads of grad_rows and the alpha planes over its slots keep their bits."""
    case, res, ins, exp, bank, got = _leg_a("inner_solid")
    a, b = case.seg[0], case.seg[4]
    assert (got["features"][1, a:b] == SENT16).all()


@pytest.mark.gpu
def test_rows_consumed_and_launch_deterministic():
    """The second launch on the now cleared rows adds nothing to weights.grad; a fresh run of the same case
    gives the same bits."""
    case, res, ins, exp, bank, got = _leg_a("widths_a")
    bank.backward_mlp(case.grad_scale)
    again = _read(bank)
    assert np.array_equal(again["wgrad"].view(np.uint32), got["wgrad"].view(np.uint32))
    assert np.array_equal(again["rows"], got["rows"])
    assert not again["dabs"].any()
    _, fresh = _run(case, ins)
    for key in ("features", "rows", "wgrad", "dabs"):
        assert np.array_equal(fresh[key].view(np.uint8), got[key].view(np.uint8)), key


@pytest.mark.gpu
def test_exact_with_one_infinite_gradient():
    """+inf in one gradient element of one slot (colour, degree 3, channel 17: the second k-step): that slot's
    dF, that texture's weight gradients and dfeat_abs_sum are non-finite exactly where the restatement's are
    and bit-equal elsewhere; every other slot and texture equals the run without the inf."""
    base, base_res = _case("widths_a", _n_cus())
    x, slot_in_seg, ch = 3, 5, 17
    G = dict(base.G)
    G[x] = base.G[x].copy()
    G[x][slot_in_seg, ch] = np.inf
    case = R.Case(base.layout, base.seg, base.weights, base.X, G, base.prefill, base.grad_scale)
    res = dict(base_res)
    C = case.layout.channels(x)
    res[x] = R.mlp_backward_f64(*R.unpack_weights(case.weights[x]), case.X[x], G[x][:, :C], C, 2, 1.0 / case.grad_scale)
    ins, exp = _buffers(case, res)
    _, got = _run(case, ins)
    _, got0 = _run(base, _buffers(base, base_res)[0])
    a = case.slots(x)[0] + slot_in_seg

    def nonfinite(key, buf):                     # non-finite values that are no sentinels
        if key == "features":
            return ~np.isfinite(buf.view(np.float16)) & (buf != SENT16)
        return ~np.isfinite(buf) & (buf.view(np.uint32) != SENT32)

    for key in ("features", "wgrad", "dabs"):
        bad_ref, bad_got = nonfinite(key, exp[key]), nonfinite(key, got[key])
        assert bad_ref.any()
        assert np.array_equal(bad_got, bad_ref), (key, np.argwhere(bad_got != bad_ref)[:8].tolist())
        g, e = got[key].copy(), exp[key].copy()
        g[bad_ref], e[bad_ref] = 0, 0
        _assert_bits(case, key, g, e, raw=~exp["touched"] if key == "wgrad" else None)
    _assert_bits(case, "rows", got["rows"], exp["rows"])
    # what the inf may reach: slot `a` of the colour planes, texture x's weight gradients and its dabs
    bad = nonfinite("features", exp["features"])
    assert bad[0, a].any() and not np.delete(bad, a, axis=1).any() and not bad[1].any()
    same = np.ones_like(bad)
    same[0, a] = False
    assert np.array_equal(got["features"][same], got0["features"][same])
    others = [t for t in range(case.layout.n_tex) if t != x]
    assert np.array_equal(got["wgrad"][others].view(np.uint32), got0["wgrad"][others].view(np.uint32))
    assert np.array_equal(got["dabs"][others].view(np.uint32), got0["dabs"][others].view(np.uint32))
    assert np.array_equal(got["rows"], got0["rows"])


# ---------------------------------------------------------------- GPU, leg B

# Measured on the MI355X against the float64 restatement (both row formats, the maximum of the two runs below):
#   weight gradients, max |got - ref| / (A 2^-11), A = the restatement's sum |terms| of that element
MEASURED_DW = {"dW1": 0.0343, "dW2": 1.6570, "dW3": 0.0382}
#   dF, largest distance from the reference in f16 ulps of the reference (reached where dX all but cancels: an
#   ulp of the reference is then far below the rounding of the terms), the same error as a multiple of A 2^-11, and
#   the largest relative error of dfeat_abs_sum
MEASURED_DF_ULPS, MEASURED_DF_OF_A, MEASURED_DABS_REL = 836.0, 1.8456, 3.502e-6
DF_SHARE_OVER_1ULP_CAP = 0.01          # a cap (module docstring), not a measurement
LEG_B_SEG = {0: [1000, 129, 997, 33], 1: [33, 1003, 129, 1000]}


@pytest.mark.gpu
@pytest.mark.parametrize("row_format", [0, 1])
def test_rounding_against_float64(row_format):
    """dOut = G sigmoid'(out) and ordinary rounding: weights U(-0.45, 0.45), features from bank.encode() of
    random tables (the recipe of test_nt_mlp._bank), gradient rows N(0, 1) grad_scale / n rounded to f16;
    K = 1, all degrees, segments of about 1000 slots and the ragged 33 and 129."""
    lay = R.Layout(1, 512, textures_res=(64, 64, 32, 32))
    seg_len = LEG_B_SEG[row_format]
    seg = np.concatenate([[0], np.cumsum(seg_len)])
    g = torch.Generator().manual_seed(20 + row_format)
    rng = np.random.default_rng(30 + row_format)
    shape = R.Case(lay, seg, None, {}, {}, None, GRAD_SCALE, row_format)
    bank = _new_bank(shape)
    with torch.no_grad():
        bank.tables.copy_(torch.rand(bank.tables.shape, generator=g) * 2 - 1)
        w = (torch.rand(bank.weights.shape, generator=g) * 2 - 1) * 0.45
        bank.weights.copy_(w.cuda() * (bank.weights != 0))
        bank.refresh_half_params()
        bank.seg_start.copy_(torch.tensor(seg, dtype=torch.int32))
        bank.slot_xy.copy_(torch.rand(bank.slot_xy.shape, generator=g))
        bank.features.view(torch.int16).fill_(int(np.uint16(SENT16).view(np.int16)))
    bank.encode()
    torch.cuda.synchronize()
    f_in = R.unpack_features(bank.features.view(torch.int16).cpu().numpy().view(np.uint16))
    assert (f_in[:, seg[-1]:] == SENT16).all()
    weights = bank.weights_h.cpu().double().numpy()
    X, G = {}, {}
    prefill = np.full((lay.n_tex, R.WEIGHTS_PER_TEX), SENT32, np.uint32)
    for x in range(lay.n_tex):
        C, (_, typ, deg) = lay.channels(x), R.Layout.split(x)
        n = seg_len[deg]
        prefill[x, :R.W3_OFF + C * 64] = 0
        X[x] = f_in[typ, seg[deg]:seg[deg + 1]].view(np.float16).astype(np.float64)
        assert np.isfinite(X[x]).all() and X[x].any()
        G[x] = np.zeros((n, R.Layout.own_quads(x)[1] * 4))
        G[x][:, :C] = R.f16(rng.normal(0, 1, (n, C)) * GRAD_SCALE / n)
    case = R.Case(lay, seg, weights, X, G, prefill.view(np.float32), GRAD_SCALE, row_format)
    res = R.restate_case(case)
    ins, exp = _buffers(case, res)
    with torch.no_grad():
        bank.grad_rows.view(torch.int16).copy_(torch.from_numpy(ins["rows"].view(np.int16)))
        bank.weights.grad = torch.from_numpy(ins["wgrad"].copy()).cuda()
    bank.backward_mlp(case.grad_scale)
    got = _read(bank)

    # what must keep its bits, as in leg A
    _assert_bits(case, "rows", got["rows"], exp["rows"])
    assert np.array_equal(got["features"][:, seg[-1]:], f_in[:, seg[-1]:])
    outside = ins["wgrad"].view(np.uint32) == SENT32
    assert np.array_equal(got["wgrad"].view(np.uint32)[outside], ins["wgrad"].view(np.uint32)[outside])

    dw = {k: 0.0 for k in MEASURED_DW}
    ulps, over1, n_df, dabs_rel, df_of_a, worst = 0.0, 0, 0, 0.0, 0.0, None
    hist = np.zeros(4, np.int64)
    for x in case.textures():
        C, r, typ = lay.channels(x), res[x], R.Layout.split(x)[1]
        a, b = case.slots(x)
        for name, off in (("dW1", R.W1_OFF), ("dW2", R.W2_OFF), ("dW3", R.W3_OFF)):
            ref, A = getattr(r, name).ravel(), r.A[name].ravel()
            gw = got["wgrad"][x, off:off + ref.size].astype(np.float64)
            assert not gw[A == 0].any()
            dw[name] = max(dw[name], float((np.abs(gw - ref)[A > 0] / (A[A > 0] * R.F16_U)).max()))
        gf = got["features"][typ, a:b].view(np.float16)
        ref16 = r.dX16.astype(np.float16)
        d = np.abs(gf.astype(np.float64) - r.dX16) / np.spacing(np.abs(ref16)).astype(np.float64)
        e_a = np.abs(gf.astype(np.float64) - r.dX16) / (r.A["dX"] * R.F16_U)
        if d.max() > ulps:
            i = np.unravel_index(np.argmax(d), d.shape)
            worst = (x, float(r.dX[i]), float(r.A["dX"][i]), float(e_a[i]))
        df_of_a = max(df_of_a, float(e_a.max()))
        ulps, over1, n_df = max(ulps, float(d.max())), over1 + int((d > 1).sum()), n_df + d.size
        hist += np.array([(d == 0).sum(), ((d > 0) & (d <= 1)).sum(), ((d > 1) & (d <= 2)).sum(), (d > 2).sum()])
        dabs_rel = max(dabs_rel, float((np.abs(got["dabs"][x] - r.dabs) / r.dabs).max()))
    print("leg B row_format %d: " % row_format + ", ".join("%s %.4f" % kv for kv in sorted(dw.items())) +
          " of A 2^-11; dF max %.2f ulp, share over 1 ulp %.5f, 0 / <=1 / <=2 / >2 ulp: %s of %d; dabs rel %.3e; "
          "dF max %.4f of A 2^-11; worst ulp distance at texture %d: ref %.3e, A %.3e, error %.4f of A 2^-11"
          % ((ulps, over1 / n_df, hist.tolist(), n_df, dabs_rel, df_of_a) + worst))
    assert over1 / n_df <= DF_SHARE_OVER_1ULP_CAP
    for name, m in MEASURED_DW.items():
        assert dw[name] <= 2 * m, (name, dw[name])
    assert ulps <= 2 * MEASURED_DF_ULPS and df_of_a <= 2 * MEASURED_DF_OF_A and dabs_rel <= 2 * MEASURED_DABS_REL
