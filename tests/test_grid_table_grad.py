"""The fp32 hash grid's three table-gradient paths (csrc/grid_encode.hip) against a float64 sum.

    atomic  vsa_grid_encode_bwd_ld          one float atomicAdd per contribution
    sliced  vsa_grid_encode_bwd_sliced_ld   LDS slices of 2^13 entries, 64-bit fixed point, one partial
                                            sum per sample chunk, joined by float atomicAdds
    binned  vsa_grid_encode_bwd_binned_ld   contributions binned by slice, then accumulated in 64-bit
                                            fixed point, one partial sum per 2^18 records of a bin

All three are called through the C ABI at EVERY size (no Python size threshold), at the smallest shapes
that reach every branch.  The reference is grid_table_grad_restated.table_grad_f64: the fp32 corner
weights and indices of oracle/tcnn_like.grid_forward_f32, the products and sums in float64.  Per table
float it yields the sum S, A = sum |w g| and n = the number of nonzero contributions.

THE BOUND is a rounding bound derived from the arithmetic each path performs; no figure in it is fitted
to what the kernels return.  u = 2^-24 (fp32 round to nearest), p = the value the float held before.

  atomic:  out = fl(...fl(fl(p + fl(w g_1)) + fl(w g_2))...).  One product rounding per contribution,
           together u A; n float adds, each rounding a running value of at most |p| + A:
               (n + 1) u A  +  n u |p|

  sliced / binned:
      q = 2^(E + cb - 62) is the fixed-point quantum: 2^(E-1) <= max finite |g| < 2^E over the 2 L gradient
      columns (frexp), cb = ceil(log2(B 2^D)) the binned path's count bits and an upper bound of the
      sliced path's (which counts the samples of one chunk only).
        * every contribution is rounded to the nearest quantum                      (n / 2) q
        * its fp32 product w g before that                                           u A
        * a partial sum (an exact integer) is scaled back in double and rounded to
          float: the partial sums together are at most A' = A + (n / 2) q            u A'
          (the int64 -> double conversion before that rounds at 2^-53: a further
          step that the code shows)                                                  2^-53 A'
        * P float atomicAdds of the partial sums into the output, each rounding a
          running value of at most |p| + A'                                          P u (A' + |p|)
               (n / 2) q  +  (2 + P) u A'  +  P u |p|  +  2^-53 A'
      P = min(n, sample chunks of the sliced launch) or min(n, ceil(records in the entry's bin / 2^18)),
      from the rules in the host code: chunks = max(1, ceil(6 CUs / (slices * L))) with slices =
      ceil(largest level / 2^13); a bin is shared out in quanta of 2^18 records.

  With p = 0 these are the bounds (n + 1) u A and (n / 2) q + (2 + P) u A up to the second-order terms
  spelled out above.  For a pre-filled buffer the term is K u |p| with K the float adds into the output (n
  or P), not a single u |p + S|: every one of those adds rounds a running value that contains p.  For K = 1
  it is no larger than u |p + S| plus the terms already present.
  A float without a contribution (n = 0) has bound 0: it must keep its bits.
  A float touched by a non-finite gradient (S non-finite) must be non-finite, all others finite and
  within the bound.

Geometries (D, L, log2 table size, base resolution, growth):
  d3   (3, 13, 18, 16, 2)    dense 16^3 (4096 entries: one ragged slice) and 32^3 (four slices), hashed 2^18
                             levels (all 32 slices), level 12 at resolution 65 536 with the wrapped uint32
                             stride that the oracle restates
  d2   (2, 16, 15, 16, 1.5)  dense levels of 256 .. 14 888 entries (two slices, the last ragged), four slices
  s64  (3, 3, 19, 64, 2)     2^19 entries = 64 slices: sliced only, binned must refuse
  b17  (3, 4, 18, 17, 2)     base 17: dense 17^3 -> 4920 entries and 34^3 -> 39 304 (five slices, the last
                             ragged), the sizes base 16 does not produce
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import grid_table_grad_restated as R
from oracle.tcnn_like import GridGeometryND, grid_forward_f32

U = 2.0 ** -24
GEOMS = {"d3": (3, 13, 18, 16, 2.0), "d2": (2, 16, 15, 16, 1.5), "s64": (3, 3, 19, 64, 2.0),
         "b17": (3, 4, 18, 17, 2.0)}
PATHS = ("atomic", "sliced", "binned")
BIN_QUANTUM = 1 << 18


@functools.lru_cache(maxsize=None)
def _geom(name):
    return GridGeometryND(*GEOMS[name])


def _positions(kind, B, D, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    if kind == "uniform":                       # with rows of exact 0.0 and 1.0
        x = torch.rand(B, D, generator=g)
        if B >= 3:
            x[B // 3] = 0.0
            x[2 * B // 3] = 1.0
    elif kind == "point":                       # every sample in one place: the worst collision count
        x = torch.tensor([0.3711, 0.6172, 0.2043][:D]).repeat(B, 1)
    else:                                       # "rays": 64 consecutive samples per segment inside one coarse cell
        seg = (B + 63) // 64
        o = torch.rand(seg, D, generator=g) * 0.9 + 0.05
        d = torch.nn.functional.normalize(torch.randn(seg, D, generator=g), dim=-1) * (1.0 / 64)
        t = (torch.arange(64, dtype=torch.float32) / 64)[None, :, None]
        x = (o[:, None] + t * d[:, None]).reshape(-1, D)[:B].clamp(0.0, 1.0)
    return x.contiguous()


def _gradient(kind, B, L, seed=0):
    g = torch.Generator().manual_seed(200 + seed)
    go = torch.randn(B, 2 * L, generator=g)
    if kind == "randn":                         # every 7th row zero: rows the kernels skip
        go[6::7] = 0
    elif kind == "zero":
        go.zero_()
    elif kind == "single":
        v = go[B // 2, L + 1].item()
        go.zero_()
        go[B // 2, L + 1] = v
    elif kind == "one_level":
        keep = go[:, 2:4].clone()
        go.zero_()
        go[:, 2:4] = keep
    elif kind == "dynamic_range":
        go = R.dynamic_range_gradient(B, 2 * L, seed)
    else:
        raise ValueError(kind)
    return go


class _Case:
    """Inputs and the float64 reference of one (geometry, B, positions, gradient), computed once."""

    def __init__(self, geom_name, B, pos, grad, padded=False, nonfinite=False):
        self.geom_name, self.geom, self.B = geom_name, _geom(geom_name), B
        D, L = self.geom.n_dims, self.geom.n_levels
        self.x = _positions(pos, B, D)
        go = _gradient(grad, B, L)
        self.marks = []
        if nonfinite:                           # one +inf and one NaN element, different samples, levels and features
            self.marks = [(B // 4, 2 * 1 + 0, float("inf")), (B // 2 + 1, 2 * (L - 1) + 1, float("nan"))]
            for r, c, v in self.marks:
                go[r, c] = v
        self.stride = 2 * L
        if padded:                              # rows of 2 L + D floats padded to a multiple of 4; the padding is never read
            self.stride = (2 * L + D + 3) // 4 * 4
            buf = torch.full((B, self.stride), float("nan"))
            buf[:, :2 * L] = go
            go = buf
        self.g = go.contiguous()
        self.S, self.A, self.n = R.table_grad_f64(self.geom, self.x, self.g)
        self.E = R.grad_exponent(self.g, 2 * L)
        self.records = R.bin_records(self.geom, self.x, self.g)

    def partial_sums(self, path, nr_cus):
        """P per table float [n_entries, 2]: the float adds into the output."""
        geom = self.geom
        if path == "atomic":
            return self.n
        if path == "sliced":     # host code: sample chunks = enough workgroups for six per CU
            slices = (max(geom.size) + (1 << R.SLICE_LOG2) - 1) >> R.SLICE_LOG2
            chunks = max(1, -(-6 * nr_cus // (slices * geom.n_levels)))
            return np.minimum(self.n, chunks)
        # binned: a bin is shared out in quanta of 2^18 records
        return np.minimum(self.n, R.per_entry(geom, -(-self.records // BIN_QUANTUM)))

    def bound(self, path, nr_cus, prefill):
        p = np.abs(prefill)
        P = self.partial_sums(path, nr_cus).astype(np.float64)
        n = self.n.astype(np.float64)
        with np.errstate(invalid="ignore"):
            if path == "atomic":
                return (n + 1) * U * self.A + n * U * p
            if self.E is None:
                return np.zeros_like(self.A)
            q = 2.0 ** (self.E + R.count_bits(self.B << self.geom.n_dims) - 62)
            a1 = self.A + 0.5 * n * q
            return 0.5 * n * q + (2 + P) * U * a1 + P * U * p + 2.0 ** -53 * a1


@functools.lru_cache(maxsize=3)                # (a reference of the largest geometry takes ~150 MB)
def _case(*key):
    return _Case(*key)


def _plan(geom_name):
    from volsurfs_amd.encodings import grid_plan
    plan, n_entries = grid_plan(*GEOMS[geom_name])
    assert n_entries == _geom(geom_name).offset[-1]
    return plan


def _raw(name, *args):
    """A C-ABI entry point's status (volsurfs_amd._lib.call raises on a non-zero one)."""
    from volsurfs_amd import _lib
    fn = getattr(_lib.lib(), name)
    return fn(*[_lib._conv(a, fn.argtypes is not None) for a in args])


def _run(path, case, prefill=None, x=None, g=None):
    """The table gradient of one path [n_entries, 2] on the CPU, added to `prefill` (zeros when None)."""
    from volsurfs_amd import _lib
    plan = _plan(case.geom_name)
    x = (case.x if x is None else x).cuda()
    g = (case.g if g is None else g).cuda()
    B, L = x.shape[0], case.geom.n_levels
    out = torch.zeros(case.geom.offset[-1], 2) if prefill is None else torch.from_numpy(prefill).clone()
    out = out.cuda()
    st = _lib.stream_ptr()
    if path == "atomic":
        _lib.call("vsa_grid_encode_bwd_ld", ctypes.byref(plan), x, g, g.shape[1], B, out, st)
    elif path == "sliced":
        ws = torch.empty(2 * B * L + 32, device="cuda")          # [L][B] float2 + 32 words
        _lib.call("vsa_grid_encode_bwd_sliced_ld", ctypes.byref(plan), x, g, g.shape[1], B, out, ws, st)
    else:
        n = ctypes.c_longlong()
        _lib.call("vsa_grid_encode_bwd_binned_workspace", ctypes.byref(plan), B, ctypes.byref(n))
        ws = torch.empty(n.value, device="cuda")
        _lib.call("vsa_grid_encode_bwd_binned_ld", ctypes.byref(plan), x, g, g.shape[1], B, out, ws, st)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _nr_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _check(path, case, got, prefill=None):
    p = np.zeros_like(case.S, dtype=np.float32) if prefill is None else prefill
    bound = case.bound(path, _nr_cus(), p.astype(np.float64))
    finite = np.isfinite(case.S)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - (p.astype(np.float64) + case.S))
        ratio = np.where(finite & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%s %s B=%d: %d floats with contributions, worst error / bound = %.3g at %s (error %.3g, bound %.3g, n %d)"
          % (case.geom_name, path, case.B, int((case.n > 0).sum()), ratio[worst], worst, err[worst], bound[worst],
             case.n[worst]))
    # floats a non-finite gradient touches are non-finite, and only those
    assert np.array_equal(np.isfinite(got), finite), \
        "%s: %d floats non-finite, %d expected" % (path, int((~np.isfinite(got)).sum()), int((~finite).sum()))
    bad = finite & ~(err <= bound)
    assert not bad.any(), "%s: %d table floats beyond the bound, worst %.3g x at %s" % (
        path, int(bad.sum()), ratio[worst], worst)
    # a float without a contribution keeps its bits
    untouched = case.n == 0
    assert np.array_equal(got[untouched].view(np.uint32), p[untouched].view(np.uint32)), path


# ---- CPU: the reference and the emulated conversions

def test_restated_table_gradient_equals_float64_autograd():
    """The helper's sum is the gradient torch autograd forms for the oracle forward run on a float64
    table, to float64 rounding (n + 1 roundings of at most 2^-53 A on each side)."""
    for name, B in (("b17", 700), ("d2", 500)):
        geom = _geom(name)
        x = _positions("uniform", B, geom.n_dims)
        go = _gradient("randn", B, geom.n_levels)
        table = torch.zeros(geom.offset[-1], 2, dtype=torch.float64, requires_grad=True)
        out = grid_forward_f32(geom, table, x)
        assert out.dtype == torch.float64
        out.backward(go.double())
        S, A, n = R.table_grad_f64(geom, x, go)
        assert (n > 0).sum() > 1000 and np.abs(S).max() > 0
        err = np.abs(table.grad.numpy() - S)
        assert (err <= 2 * (n + 1) * 2.0 ** -53 * A).all()


def test_conversion_emulation_values():
    """The signed split rounds small negative values (spacing 256 above 2^31, saturation at 2^32); the
    magnitude split is exact for both signs."""
    v = np.array([-5, -100, -200, -1000, -12345, 5, 100, 12345, 2.0 ** 40, -2.0 ** 40, -2.0 ** 31 - 256, 0], np.float32)
    assert R.fixed62_signed_split(v).tolist() == [-1, -1, -256, -1024, -12288, 5, 100, 12345, 1 << 40, -(1 << 40),
                                                  -(1 << 31) - 256, 0]
    r = np.random.default_rng(0)
    w = (r.standard_normal(200000) * np.exp2(r.integers(0, 61, 200000))).astype(np.float32)
    assert np.array_equal(R.fixed62_magnitude_split(w), np.rint(w.astype(np.float64)).astype(np.int64))


def test_dynamic_range_gradient_separates_the_two_conversions():
    """B = 4096 on the first geometry, one gradient of 1.0 among +-[1, 2) 2^-16 .. 2^-34: q = 2^-46.  With
    the signed split the emulated fixed-point sums break the bound; with the magnitude split they hold it."""
    case = _case("d3", 4096, "uniform", "dynamic_range")
    cb = R.count_bits(4096 << 3)
    assert case.E == 1 and cb == 15
    bound = case.bound("binned", 256, np.zeros_like(case.S))       # one partial sum per float
    assert (case.partial_sums("binned", 256) <= 1).all()
    new = R.table_grad_fixed_point(case.geom, case.x, case.g, R.fixed62_magnitude_split, cb)
    old = R.table_grad_fixed_point(case.geom, case.x, case.g, R.fixed62_signed_split, cb)
    err_new, err_old = np.abs(new - case.S), np.abs(old - case.S)
    assert (err_new <= bound).all()
    beyond = err_old > bound
    print("signed split: %d of %d floats beyond the bound, worst %.3g x" % (
        beyond.sum(), (case.n > 0).sum(), (err_old[beyond] / bound[beyond]).max()))
    assert beyond.any()


# ---- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 64, 65, 1000, 8193])
@pytest.mark.parametrize("pos", ["uniform", "point", "rays"])
@pytest.mark.parametrize("geom_name", ["d3", "d2", "b17"])
def test_three_paths_hold_the_bound(geom_name, pos, B):
    """One lane / one wave / the transposer's ragged 64-row tile / several workgroups / the sliced kernel's
    8192-sample trip plus one; B below the sliced chunk count leaves chunks empty."""
    case = _case(geom_name, B, pos, "randn")
    for path in PATHS:
        _check(path, case, _run(path, case))


@pytest.mark.gpu
@pytest.mark.parametrize("grad", ["zero", "single", "one_level", "dynamic_range"])
@pytest.mark.parametrize("geom_name", ["d3", "d2"])
def test_gradient_patterns(geom_name, grad):
    """All zero (the pre-filled buffer keeps its bits), one nonzero element, one level only, and the
    dynamic-range gradient at B = 4096 that separates an exact fixed-point conversion from one that rounds
    small negative contributions."""
    case = _case(geom_name, 4096 if grad == "dynamic_range" else 1000, "uniform", grad)
    g = np.random.default_rng(5)
    prefill = g.standard_normal(case.S.shape).astype(np.float32) if grad == "zero" else None
    for path in PATHS:
        _check(path, case, _run(path, case, prefill), prefill)


@pytest.mark.gpu
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("geom_name,B,pos", [("d3", 1000, "uniform"), ("d2", 65, "rays"), ("b17", 8193, "point")])
def test_row_stride_and_accumulation_into_a_prefilled_buffer(geom_name, B, pos, padded):
    """g_stride = 2 L and 2 L + D padded to a multiple of 4 with NaN in the padding; the result is added to
    what the gradient buffer held."""
    case = _case(geom_name, B, pos, "randn", padded)
    assert case.g.shape[1] == (2 * case.geom.n_levels if not padded else {"d3": 32, "d2": 36, "b17": 12}[geom_name])
    prefill = np.random.default_rng(6).standard_normal(case.S.shape).astype(np.float32)
    for path in PATHS:
        _check(path, case, _run(path, case, prefill), prefill)


@pytest.mark.gpu
def test_one_bin_beyond_a_quantum_of_records():
    """40 000 samples at one point: the one bin of the coarsest level holds all 274 288 records
    of that level, more than 2^18: the accumulation of such a bin is split over blockIdx.z and joined by float adds."""
    case = _case("d3", 40000, "point", "randn")
    assert case.records.max() > BIN_QUANTUM
    assert case.partial_sums("binned", _nr_cus()).max() == 2
    for path in PATHS:
        _check(path, case, _run(path, case))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [65, 8193])
def test_sixty_four_slices_sliced_only(B, monkeypatch):
    """2^19 entries per level: the sliced path is right, the binned entry point (32 slices at most) refuses
    before it launches anything, and encodings._GridEncode with both thresholds at 1 takes the sliced path."""
    from volsurfs_amd import _lib, encodings as E
    case = _case("s64", B, "uniform", "randn")
    _check("atomic", case, _run("atomic", case))
    _check("sliced", case, _run("sliced", case))
    plan = _plan("s64")
    n = ctypes.c_longlong()
    _lib.call("vsa_grid_encode_bwd_binned_workspace", ctypes.byref(plan), B, ctypes.byref(n))
    ws = torch.empty(n.value, device="cuda")
    out = torch.zeros(case.geom.offset[-1], 2, device="cuda")
    x, g = case.x.cuda(), case.g.cuda()
    rc = _raw("vsa_grid_encode_bwd_binned_ld", ctypes.byref(plan), x, g, g.shape[1], B, out, ws, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -2                              # VSA_ERR_UNSUPPORTED
    assert not out.any()
    # through the autograd function
    D, L, log2, base, growth = GEOMS["s64"]
    enc = E.HashGrid(D, {"otype": "Grid", "type": "Hash", "n_levels": L, "n_features_per_level": 2,
                         "log2_hashmap_size": log2, "base_resolution": base, "per_level_scale": growth})
    called, call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), call(name, *a))[1])
    monkeypatch.setattr(E, "SLICED_BWD_MIN_POINTS", 1)
    monkeypatch.setattr(E, "BINNED_BWD_MIN_POINTS", 1)
    enc(x).backward(g)
    torch.cuda.synchronize()
    assert "vsa_grid_encode_bwd_sliced_ld" in called
    assert not [c for c in called if "binned" in c or c == "vsa_grid_encode_bwd_ld"]
    _check("sliced", case, enc.params.grad.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("geom_name", ["d3", "d2"])
def test_binned_path_does_not_depend_on_the_order_of_the_samples(geom_name):
    """Every bin within one quantum of 2^18 records: one integer sum per table float, so two runs and a run
    with the samples permuted agree bit for bit.  (No such claim for the sliced path: float adds join its chunks.)"""
    case = _case(geom_name, 8193, "uniform", "randn")
    assert case.records.max() <= BIN_QUANTUM
    a = _run("binned", case)
    b = _run("binned", case)
    perm = torch.randperm(case.B, generator=torch.Generator().manual_seed(9))
    c = _run("binned", case, x=case.x[perm].contiguous(), g=case.g[perm].contiguous())
    _check("binned", case, a)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("geom_name,B", [("d3", 1000), ("d2", 8193)])
def test_non_finite_gradients_reach_exactly_the_entries_they_touch(geom_name, B):
    """One +inf and one NaN element: on every path the table floats those two samples' corners touch on
    that level and feature are non-finite, as the float64 reference marks them, and no others."""
    case = _case(geom_name, B, "uniform", "randn", False, True)
    marked = ~np.isfinite(case.S)
    D = case.geom.n_dims
    assert 2 <= marked.sum() <= 2 << D
    assert marked[:, 0].any() and marked[:, 1].any()
    for path in PATHS:
        _check(path, case, _run(path, case))
