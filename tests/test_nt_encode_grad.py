"""The neural-texture hash grid's table gradient (csrc/nt_encode.hip: vsa_nt_encode_bwd, _range, _phased)
against a float64 sum, in isolation: the test writes everything the kernel reads — slot_xy, seg_start, dF
(the `features` planes) and dfeat_abs_sum (bank._dfsum) — on a NeuralTextureBank and runs only the encode
backward.  No mark / compact, MLP or shade kernel runs (except in the last test, which checks the producer
of dfeat_abs_sum).

THE REFERENCE is nt_encode_grad_restated.table_grad_f64.  For each (shell, degree) segment, each of its two
textures, each level and feature: the fp32 corner weights and indices of oracle/tcnn_like._grid_cells (what
cell_ref / cell_indices restate), dF converted from half to float64 exactly, the products and sums in
float64.  Per table float, indexed by the parameter texture: S = sum w g, A = sum |w g|, n = the number of
contributions with g != 0.  The expected output is p + S / grad_scale, p the value the float held before.
Non-finite dF is excluded: the fixed point has no representation for it and the restatement refuses it.

THE BOUND follows the arithmetic of enc_bwd_piece; no figure in it is fitted to what the kernel returns.
u = 2^-24, p' = p grad_scale (the held value in the units of dF).
  nt_encode.hip:293-305  total = fl(dfsum * 1.001f) = m 2^e with m in [0.5, 1) (frexpf); S = 2^(30 - e) and
                         2^(e - 30) are powers of two.  q = 2^(e - 30) is the quantum.  e comes from the dfsum
                         the kernel is GIVEN, not from the true sum.
  :396-397               gv = dF * S in one v_fma_mix_f32: a half times a power of two, exact.
  :405                   fl(w gv), one fp32 product per contribution: together                    u A
  :406-407               v_cvt_rpi rounds each contribution to the nearest integer:               (n / 2) q
  :415-441, :466-478     integer adds (registers, LDS atomics, the `copies` planes): exact, since
                         sum |g| 2^(30 - e) + n / 2 < 2^31 (asserted in the restatement and, for the real
                         producer, in the last test).  The integers of a float are together at most
                         A' = A + (n / 2) q.
  :496-498, :510         (float)vi and its product with S_inv = 2^(e - 30) fl(1 / grad_scale) round
                         once each:                                                                2 u A'
  :787 (host)            fl(1 / grad_scale) when grad_scale is no power of two:                    u A'
  :510                   P float adds into the output, each rounding a running value of at most
                         |p'| + A':                                                                P u (A' + |p'|)
In total, divided by grad_scale:

    [(n / 2) q + u A + (2 + P) u A' + P u |p'|] / grad_scale     (+ u A' / grad_scale for fl(1 / grad_scale))

P: the work split (nt_for_each_piece, ENC_UNIT) cuts a segment at multiples of 256 slots only, so one walk
of a segment makes at most ceil(length / 256) flushes, and a flush adds to a float only if one of its own
contributions is nonzero: P = min(n, units), summed over the logical textures that share the parameter
texture and over the launches made.  Every launch here walks every segment once, the shell-by-shell and the
phased ones too.  A stored plane (:496-498) makes no add at all and is covered by P = 1; whether a plane of
several units is stored or cut depends on the grid, so the test takes its units.  With shared models the K
logical textures have K quanta: (n / 2) q is summed per contribution (H in the restatement).
A float with n = 0 has bound 0 and must keep its bits, also in a pre-filled buffer.

The CPU tests show that the bound is right and that it has teeth: a numpy emulation of the arithmetic above
stays within it, and three wrong variants (truncation, a dropped corner, a plane copy left out of the flush)
exceed it on the same inputs.

BRANCHES.  K = 3, textures_res = (256, 128, 64, 32), two geometries:
  default  levels 0-5 dense, both features per pass, copies 32, 16, 8, 4, 2, 1; levels 6-15 hashed
  g100     base 100, growth 1.3: level 0 dense with 10 000 entries (both features, copies 1), levels 1, 2 dense
           with 16 904 and 28 568 entries (ONE feature per pass: the path the default geometry never takes),
           levels 3-15 hashed
  enc_bwd_piece<HASHED, NF, MERGE>   reached by (geometry: level, degree)
    <false, 2, true>    default: levels 0-5, every degree;  g100: level 0, every degree
    <false, 1, true>    g100: levels 1, 2 at degree 0 (scale 129, 168 < 256)
    <false, 1, false>   g100: levels 1, 2 at degrees 1-3
    <true, 1, true>     default: level 6 (scale 181.25) at degree 0;  g100: level 3 (218.7) at degree 0
    <true, 1, false>    every other hashed (level, degree)
  copies > 1            default: levels 0-4
  store                 grads_zeroed=True: every uncut segment (all but the 6001-slot one are one or a few units)
  atomic, P > 1         the 6001-slot segment (24 units, cut by a launch of one workgroup per CU), the 905-slot
                        one; the launch repeated; reserve_cus=200 (56 workgroups: other cuts)
  shared                shared_rgb and shared_alpha: three writers per plane, never stored
  range                 shells=(s, s + 1) for s = 0, 1, 2
  phased                vsa_nt_encode_bwd_phased with phases [2, 3], reserve_cus 0 and 200
  early return          a texture whose dF (and dfsum) is zero;  NF = 2 with one scale zero: one (texture,
                        level 0) whose feature 1 is all zero
  cell column -1        the apron texels left of a texture (x = -0.5 / R) lie in column 0xffffffff once a level is
                        finer than the texture (scale > R).  The both-feature dense levels run the MERGE code at any
                        scale: default levels 4, 5 at R = 64 and levels 2-5 at R = 32 (the merge bookkeeping once
                        took that column for "no cell yet" and dropped those texels' contributions: 408 floats of
                        the first case below); the hashed levels reach the same column without MERGE
Segment lengths 1, 257, 9, 33, 6001, 129, 905, 0, 8, 256, 7, 255: the starts take every residue mod 8, so
the 8-slot lane stretches straddle the textures' segments; every slot of slot_xy and dF past the last
segment holds NaN (the guarded over-reads of :339-355 must not reach the result).
"""
import functools

import numpy as np
import pytest
import torch

import nt_encode_grad_restated as R
from oracle.tcnn_like import GridGeometry

K = 3
TEX_RES = (256, 128, 64, 32)
MAX_RAYS = 1024
SEG_LEN = (1, 257, 9, 33, 6001, 129, 905, 0, 8, 256, 7, 255)
RANDOM_SD, ONE_CELL_SD = 6, 11            # the segment in random order, the one inside a single grid cell
ZERO_TEX = (1, 1)                         # (segment, type) whose dF is all zero: the early return
HALF_ZERO = (4, 0, 0)                     # (segment, type, level) whose feature 1 is all zero
GRIDS = {"default": {}, "g100": dict(base_resolution=100, per_level_scale=1.3)}


@functools.lru_cache(maxsize=None)
def _geom(name):
    return GridGeometry(**GRIDS[name])


def _capacity():
    cap = K * sum(min(4 * MAX_RAYS, (r + 2) ** 2) for r in TEX_RES)
    return (cap + 255) // 256 * 256 + 256          # NeuralTextureBank's slot_capacity


def _slots():
    """seg [13] and slot_xy [capacity, 2]: texel centres in texel order, one segment in random order, one
    that alternates between two neighbouring texels in runs of three; NaN past the last segment."""
    rng = np.random.default_rng(11)
    seg = np.concatenate([[0], np.cumsum(SEG_LEN)])
    xy = np.full((_capacity(), 2), np.nan, np.float32)
    for sd, n in enumerate(SEG_LEN):
        res = TEX_RES[sd % R.MAX_DEG]
        T = (res + 2) ** 2
        if sd == ONE_CELL_SD:
            t0 = (res // 2) * (res + 2) + res // 3 + 1
            t = t0 + (np.arange(n) // 3) % 2
        else:
            t = rng.choice(T, n, replace=False)
            if n > 1000:                            # the four corners of the apron among them
                t[:4] = [0, res + 1, T - res - 2, T - 1]
                t = np.unique(t)
                t = np.concatenate([t, rng.choice(np.setdiff1d(np.arange(T), t), n - t.size, replace=False)])
            t = rng.permutation(t) if sd == RANDOM_SD else np.sort(t)
        xy[seg[sd]:seg[sd + 1]] = R.texel_centres(res, t)
    return seg, xy


@functools.lru_cache(maxsize=None)
def _frame(shared):
    seg, xy = _slots()
    return R.Frame(K, seg, xy, TEX_RES, shared, shared)


@functools.lru_cache(maxsize=None)
def _gradient(kind):
    """dF [2, 16, capacity, 2] float16, NaN past the last segment."""
    rng = np.random.default_rng({"normal": 21, "dynamic": 22}[kind])
    seg, _ = _slots()
    dF = np.full((2, 16, _capacity(), 2), np.nan, np.float16)
    make = R.gradient_normal if kind == "normal" else R.gradient_dynamic_range
    for sd, n in enumerate(SEG_LEN):
        for typ in range(2):
            dF[typ, :, seg[sd]:seg[sd + 1]] = make(rng, n)
    sd, typ = ZERO_TEX
    dF[typ, :, seg[sd]:seg[sd + 1]] = 0
    sd, typ, level = HALF_ZERO
    dF[typ, level, seg[sd]:seg[sd + 1], 1] = 0
    assert np.abs(dF[typ, level, seg[sd]:seg[sd + 1], 0]).max() > 0
    dF.setflags(write=False)
    return dF


class _Case:
    """The float64 reference of one (geometry, dF, shared models, factor on dfsum), computed once."""

    def __init__(self, geom_name, kind, shared=False, dfsum_factor=1.0):
        self.geom_name, self.geom, self.shared = geom_name, _geom(geom_name), shared
        self.frame, self.dF = _frame(shared), _gradient(kind)
        self.dfsum = R.abs_sum_rounded_up(self.dF, self.frame) * np.float32(dfsum_factor)
        S, A, n, H, P = R.table_grad_f64(self.geom, self.frame, self.dF, self.dfsum)
        self.shape, self.t = S.shape, n > 0               # kept: the floats with a contribution, in C order
        self.where = np.argwhere(self.t)
        self.S, self.A, self.n, self.H, self.P = (v[self.t] for v in (S, A, n, H, P))


@functools.lru_cache(maxsize=3)
def _case(*key):
    return _Case(*key)


def _check(label, case, got, grad_scale, prefill=None, launches=1):
    p = np.zeros(case.shape, np.float32) if prefill is None else prefill
    t = case.t
    bound = R.bound(case.A, case.H, case.P, p[t], grad_scale, launches)
    want = p[t].astype(np.float64) + launches * case.S / grad_scale
    err = np.abs(got[t].astype(np.float64) - want)
    assert (bound > 0).all()                             # (a float with n = 0 has bound 0: the bit comparison below)
    ratio = err / bound
    w = int(np.argmax(ratio))
    scale = np.abs(case.S).max() / grad_scale
    print("%s %s: %d floats with contributions, worst error / bound = %.5f at %s (error %.3g, bound %.3g, n %d, P %d); "
          "bound / largest gradient %.2g .. %.2g" % (
              case.geom_name, label, int(t.sum()), ratio[w], tuple(case.where[w]), err[w], bound[w], case.n[w],
              case.P[w], bound.min() / scale, bound.max() / scale))
    assert np.isfinite(got).all(), "%s: %d non-finite floats" % (label, int((~np.isfinite(got)).sum()))
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d table floats beyond the bound, worst %.4g x at %s" % (
        label, int(bad.sum()), ratio[w], tuple(case.where[w]))
    assert np.array_equal(got.view(np.uint32)[~t], p.view(np.uint32)[~t]), \
        "%s: a float without a contribution changed" % label
    return ratio[w]


# ---- CPU: the bound against an emulation of the kernel's arithmetic, and the geometry's branches

def _emulation_frame():
    """One shell: 6000 slots of the R = 256 texture and 900 of the R = 32 one, in texel order."""
    rng = np.random.default_rng(3)
    seg = [0, 6000, 6000, 6000, 6900]
    xy = np.concatenate([R.texel_centres(256, np.sort(rng.choice(258 ** 2, 6000, replace=False))),
                         R.texel_centres(32, np.sort(rng.choice(34 ** 2, 900, replace=False)))])
    frame = R.Frame(1, seg, xy, TEX_RES)
    dF = np.zeros((2, 16, 6900, 2), np.float16)            # type 0: normal, type 1: the dynamic range
    for a, b in ((0, 6000), (6000, 6900)):
        dF[0, :, a:b] = R.gradient_normal(rng, b - a)
        dF[1, :, a:b] = R.gradient_dynamic_range(rng, b - a)
    return frame, dF


@functools.lru_cache(maxsize=None)
def _emulation_case():
    frame, dF = _emulation_frame()
    geom = _geom("default")
    dfsum = R.abs_sum_rounded_up(dF, frame)
    S, A, n, H, P = R.table_grad_f64(geom, frame, dF, dfsum)
    return frame, dF, geom, dfsum, S, A, n, H, np.minimum(P, 1)      # the emulation flushes a segment once


@pytest.mark.parametrize("grad_scale", [4096.0, 2500.0])
def test_emulated_arithmetic_holds_the_bound(grad_scale):
    frame, dF, geom, dfsum, S, A, n, H, P = _emulation_case()
    got = R.emulate(geom, frame, dF, dfsum, grad_scale)
    zero = np.zeros(S.shape, np.float32)
    bound = R.bound(A, H, P, zero, grad_scale)
    err = np.abs(got.astype(np.float64) - S / grad_scale)
    t = n > 0
    assert t.sum() > 100000 and (got[~t] == 0).all()
    scale = np.abs(S).max(axis=(1, 2), keepdims=True) / grad_scale
    rel = (bound / np.where(scale > 0, scale, 1.0))[t]
    print("grad_scale %g: worst error / bound = %.5f, bound / the texture's largest gradient %.2g .. %.2g"
          % (grad_scale, (err[t] / bound[t]).max(), rel.min(), rel.max()))
    assert (err[t] <= bound[t]).all()
    assert (err[t] / bound[t]).max() > 0.9          # ... and tight: some float comes close to it


@pytest.mark.parametrize("mutant", ["truncate", "drop_corner", "drop_copy"])
def test_wrong_arithmetic_exceeds_the_bound(mutant):
    frame, dF, geom, dfsum, S, A, n, H, P = _emulation_case()
    got = R.emulate(geom, frame, dF, dfsum, 4096.0, mutant)
    bound = R.bound(A, H, P, np.zeros(S.shape, np.float32), 4096.0)
    err = np.abs(got.astype(np.float64) - S / 4096.0)
    beyond = err > bound
    print("%s: %d floats beyond the bound, worst %.3g x" % (mutant, beyond.sum(), (err[beyond] / bound[beyond]).max()))
    assert beyond.any()


def test_geometries_reach_every_level_class():
    from volsurfs_amd.neural_textures import grid_geometry
    scale, res, size, _ = grid_geometry(**GRIDS["g100"])
    g = _geom("g100")
    assert (scale, res, size) == (g.scale, g.res, g.size)
    cls = R.level_classes(g)
    assert size[:3] == [10000, 16904, 28568]
    assert cls[0] == (False, 2, 1) and cls[1] == cls[2] == (False, 1, 1)
    assert all(c == (True, 1, 1) for c in cls[3:]) and all(s == 32768 for s in size[3:])
    # one-feature dense and hashed levels: both MERGE instances at these resolutions
    for l in (1, 2, 3):
        assert R.merges(g, l, 256) and not R.merges(g, l, 128)
    assert not any(R.merges(g, l, 256) for l in range(4, 16))
    scale, res, size, _ = grid_geometry()
    g = _geom("default")
    assert (scale, res, size) == (g.scale, g.res, g.size)
    cls = R.level_classes(g)
    assert cls[:6] == [(False, 2, c) for c in (32, 16, 8, 4, 2, 1)]
    assert all(c == (True, 1, 1) for c in cls[6:]) and all(s == 32768 for s in size[6:])
    assert R.merges(g, 6, 256) and not R.merges(g, 6, 128) and not R.merges(g, 7, 256)


def test_segment_starts_take_every_residue():
    seg, xy = _slots()
    assert {int(s) % 8 for s in seg[:-1]} == set(range(8))
    assert {0, 1, 7, 8, 9, 255, 256, 257} <= set(SEG_LEN) and max(SEG_LEN) > 6000
    assert seg[-1] + 8 <= _capacity() and np.isnan(xy[seg[-1]:]).all() and np.isfinite(xy[:seg[-1]]).all()
    assert np.isnan(_gradient("normal")[:, :, seg[-1]:].astype(np.float32)).all()
    one = xy[seg[ONE_CELL_SD]:seg[ONE_CELL_SD + 1]]            # one cell of the coarsest level
    assert len(np.unique(np.floor(one * np.float32(_geom("default").scale[0]) + np.float32(0.5)), axis=0)) == 1


def test_frame_has_texels_left_of_a_texture_at_dense_levels_finer_than_it():
    """Column -1 under the merge code (see `cell column -1` above): present in the frame, with nonzero dF."""
    seg, xy = _slots()
    geom, dF = _geom("default"), _gradient("normal")
    cls = R.level_classes(geom)
    found = 0
    for sd in range(K * R.MAX_DEG):
        a, b = seg[sd], seg[sd + 1]
        for l in range(16):
            col = np.floor(xy[a:b, 0] * np.float32(geom.scale[l]) + np.float32(0.5))
            found += int(((col < 0) & (dF[0, l, a:b, 0] != 0)).sum()) if cls[l][1] == 2 else 0
    assert found >= 20


# ---- GPU

@functools.lru_cache(maxsize=2)
def _bank(geom_name, shared):
    from volsurfs_amd.neural_textures import NeuralTextureBank
    bank = NeuralTextureBank(K, MAX_RAYS, textures_res=TEX_RES, grid=GRIDS[geom_name] or None,
                             shared_rgb=shared, shared_alpha=shared)
    assert bank.slot_capacity == _capacity() and bank.n_entries == _geom(geom_name).offset[-1]
    for x in range(bank.n_tex):
        assert bank.param_tex(x) == (x % 8 if shared else x) and bank.tex_channels(x) > 0
    return bank


def _load(bank, case):
    seg, cap = case.frame.seg, bank.slot_capacity
    bank.seg_start.copy_(torch.tensor(seg, dtype=torch.int32))
    bank.slot_xy.copy_(torch.from_numpy(case.frame.xy))
    planes = torch.tensor(case.dF).view(2, 16, cap // 256, 256, 2).permute(0, 2, 1, 3, 4)
    bank.features.copy_(planes)                          # [type][slot >> 8][level][slot & 255][feature]
    bank._dfsum = torch.from_numpy(case.dfsum).cuda()


def _launch(bank, kind, grad_scale, prefill=None, grads_zeroed=False):
    """One launch schedule into a buffer that holds `prefill` (zeros when None); the gradient on the CPU."""
    from volsurfs_amd.parallel import StepSignals
    shape = tuple(bank.tables.shape)
    bank.tables.grad = torch.zeros(shape, device="cuda") if prefill is None else torch.from_numpy(prefill).cuda()
    if kind in ("one", "twice"):
        for _ in range(2 if kind == "twice" else 1):
            bank.backward_encode(grad_scale, grads_zeroed=grads_zeroed)
    elif kind == "by_shell":
        for s in range(K):
            bank.backward_encode(grad_scale, shells=(s, s + 1), grads_zeroed=grads_zeroed)
    else:
        sg = StepSignals(K, "cuda", [K] if bank.shared_rgb else [2, 3], 0, reserve_cus=int(kind[len("phased"):]))
        sg.signal_weights()
        bank.backward_encode_phased(grad_scale, sg, grads_zeroed=grads_zeroed)
    torch.cuda.synchronize()
    return bank.tables.grad.cpu().numpy()


def _prefill(case, grad_scale):
    g = np.random.default_rng(31)
    return (g.standard_normal(case.shape) * (np.abs(case.S).max() / grad_scale)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["normal", "dynamic"])
@pytest.mark.parametrize("geom_name", ["default", "g100"])
def test_every_launch_schedule_holds_the_bound(geom_name, kind):
    """Stores, atomics on a zero and on a pre-filled buffer, the launch repeated, shell by shell, phased with
    the whole chip and with 200 compute units reserved: each against the same reference."""
    case = _case(geom_name, kind)
    bank = _bank(geom_name, False)
    _load(bank, case)
    gs = 4096.0
    stored = _launch(bank, "one", gs, grads_zeroed=True)
    _check("stored", case, stored, gs)
    atomic = _launch(bank, "one", gs)
    _check("atomic", case, atomic, gs)
    one = case.P == 1                                    # one add of one integer sum: the same float either way
    assert one.sum() > 10000
    assert np.array_equal(stored[case.t][one].view(np.uint32), atomic[case.t][one].view(np.uint32))
    prefill = _prefill(case, gs)
    _check("prefilled", case, _launch(bank, "one", gs, prefill), gs, prefill)
    _check("twice", case, _launch(bank, "twice", gs), gs, launches=2)
    _check("by shell", case, _launch(bank, "by_shell", gs), gs)
    _check("by shell, stored", case, _launch(bank, "by_shell", gs, grads_zeroed=True), gs)
    _check("phased", case, _launch(bank, "phased0", gs), gs)
    _check("phased, stored", case, _launch(bank, "phased0", gs, grads_zeroed=True), gs)
    _check("phased, 200 CUs reserved", case, _launch(bank, "phased200", gs, prefill), gs, prefill)


@pytest.mark.gpu
@pytest.mark.parametrize("geom_name", ["default", "g100"])
def test_shared_models_hold_the_bound(geom_name):
    """shared_rgb and shared_alpha: the three shells' textures add into shell 0's planes (P and the quanta
    summed over the shells); grads_zeroed must not turn those flushes into stores."""
    case = _case(geom_name, "dynamic", True)
    assert not case.t[8:].any() and case.t[:8].any(axis=(1, 2)).all()
    bank = _bank(geom_name, True)
    _load(bank, case)
    gs = 4096.0
    _check("shared", case, _launch(bank, "one", gs), gs)
    _check("shared, grads_zeroed", case, _launch(bank, "one", gs, grads_zeroed=True), gs)
    prefill = _prefill(case, gs)
    _check("shared, phased, prefilled", case, _launch(bank, "phased0", gs, prefill), gs, prefill)


@pytest.mark.gpu
def test_grad_scale_that_is_no_power_of_two():
    case = _case("default", "normal")
    bank = _bank("default", False)
    _load(bank, case)
    prefill = _prefill(case, 2500.0)
    _check("grad_scale 2500", case, _launch(bank, "one", 2500.0, grads_zeroed=True), 2500.0)
    _check("grad_scale 2500, prefilled", case, _launch(bank, "one", 2500.0, prefill), 2500.0, prefill)


@pytest.mark.gpu
def test_bound_follows_the_dfsum_given():
    """dfeat_abs_sum eight times the true sum: the quantum is 2^3 times larger, and so is that term of the bound."""
    case, base = _case("default", "normal", False, 8.0), _case("default", "normal")
    assert np.array_equal(case.H, 8 * base.H) and np.array_equal(case.S, base.S)
    bank = _bank("default", False)
    _load(bank, case)
    _check("dfsum x 8, stored", case, _launch(bank, "one", 4096.0, grads_zeroed=True), 4096.0)
    _check("dfsum x 8, atomic", case, _launch(bank, "one", 4096.0), 4096.0)


@pytest.mark.gpu
def test_mlp_backward_hands_over_a_usable_abs_sum():
    """The producer's side: after backward_shade and backward_mlp on a real frame, for every active (texture,
    level, feature), with dF as stored in bank.features:
      * the fixed point cannot overflow: sum |dF| 2^(30 - e) + n / 2 < 2^31, e from fl(dfsum * 1.001f) as the
        kernel takes it, n = 4 corners x the nonzero slots;
      * dfsum is the sum of |dF| up to the roundings nt_mlp.hip makes.  With T = the float64 sum of |dF|:
          :681      |dx| is summed in fp32 BEFORE dx is rounded to half: 2^-11 per normal element, 2^-25
                    absolute per element whose half is subnormal or zero (count z)
          :681      a lane adds one value per four 32-slot tiles of its run: at most ceil(tiles / 4) adds
          :754      32 lanes' partial sums: 31 adds
          :755      one float atomic per pair and run: at most 4 min(tiles, workgroups) adds
        every add rounds a partial sum of nonnegative terms at u = 2^-24, so with d the number of adds an
        element can pass through and D = T (1 + 2^-10) + z 2^-25 >= the sum of |dx|:
          |dfsum - T| <= (2^-11 + d u) D + z 2^-25."""
    from test_nt_shade import _scene
    Kp, N = 2, 2500
    bank, face_uvs, hit_slot, hit_uv, tris, rays_d = _scene(Kp, N, 3)
    tex_uv = bank.mark_and_compact(hit_slot, hit_uv, face_uvs)
    bank.encode()
    bank.mlp()
    g = torch.Generator().manual_seed(0)
    g_rgb = (torch.randn(N, Kp, 3, generator=g) / N).cuda()
    g_alpha = (torch.randn(N, Kp, generator=g) / N).cuda()
    bank.backward_shade(hit_slot, tex_uv, rays_d, tris, g_rgb, g_alpha, float(N))
    bank.backward_mlp(float(N))
    torch.cuda.synchronize()
    wgs = torch.cuda.get_device_properties(0).multi_processor_count
    dF = bank.features_level_major().cpu().numpy()                     # [type, level, slot, 2]
    dfsum = bank._dfsum.cpu().numpy()
    seg = bank.seg_start.cpu().tolist()
    worst_rel, worst_fill, checked = 0.0, 0.0, 0
    for s in range(Kp):
        for d in range(bank.D):
            a, b = seg[s * 4 + d], seg[s * 4 + d + 1]
            assert b > a
            tiles = (b - a + 31) // 32
            depth = (tiles + 3) // 4 + 31 + 4 * min(tiles, wgs)
            for typ in range(2):
                x = bank.tex_index(s, typ, d)
                if not bank.tex_channels(x):
                    continue
                for l in range(16):
                    for f in range(2):
                        v = np.abs(dF[typ, l, a:b, f].astype(np.float64))
                        assert np.isfinite(v).all()
                        T, given = v.sum(), float(dfsum[x, 2 * l + f])
                        z = int((v < 2.0 ** -14).sum())
                        D = T * (1 + 2.0 ** -10) + z * 2.0 ** -25
                        tol = (2.0 ** -11 + depth * R.U) * D + z * 2.0 ** -25
                        assert abs(given - T) <= tol, (x, l, f, given, T, tol)
                        if T == 0:
                            continue
                        e = R.quantum_exponent(dfsum[x, 2 * l + f])
                        assert e is not None, (x, l, f)
                        fill = (T * 2.0 ** (30 - e) + 2 * int((v != 0).sum())) / 2.0 ** 31
                        assert fill < 1, (x, l, f, fill)
                        worst_rel, worst_fill, checked = max(worst_rel, abs(given - T) / T), max(worst_fill, fill), checked + 1
    print("%d (texture, level, feature): worst |dfsum - sum|dF|| / sum|dF| = %.3g, worst fixed-point fill %.4f of 2^31"
          % (checked, worst_rel, worst_fill))
    assert checked > 400
