"""The row terms of the hash-grid encode backward (csrc/nt_enc_common.h: cell_row, cell_col, cell_col_indices,
enc_row_break; csrc/nt_encode.hip: enc_bwd_piece; switch: vsa_nt_encode_row_terms).

THE RULE.  A lane of the backward walks 8 consecutive slots from the segment's aligned start.  What the cell
arithmetic derives from y alone — py = y * scale + 0.5, fract(py), 1 - fract(py), floor(py), and the row's hash products
cy * PRIME_Y, (cy + 1) * PRIME_Y (hashed) or its offset cy * res (dense) — is made from the lane's first slot and again
wherever some lane of the wave holds a y whose bits differ from the previous slot's.  The column part (x) is per slot.
Every operation is the one the whole-cell helpers perform on the same operands, so nothing may change.  (The forward
was built the same way over its 4-slot runs, gained nothing and kept its per-slot form; the switch's `forward`
argument is accepted and must leave the features alone — the frame still breaks rows at every position of a 4-slot run.)

CPU   a numpy restatement of the split helpers gives, for every texel of the test textures, at every level of the three
      geometries, the float32 bits and the indices of the whole-cell restatement (oracle/tcnn_like._grid_cells, which
      nt_encode_grad_restated uses); texels of one row have bit-equal y; the frame below puts a row break at every
      position of a lane's run in both kernels.
GPU   forward: the features with the switch on are those with it off and the oracle's, bit for bit.  Backward: with the
      switch on the table gradients hold the float64 bound of test_nt_encode_grad (its harness), and every plane that
      both runs flush by stores carries the same bits (the sums are integers); planes that go through float atomics
      are held to the bound only.

THE FRAME.  K = 2, textures_res = (64, 32, 16, 8): 8 (shell, degree) segments in texel raster order.  The marked rows
of a texture hold 1, 2, 3, 4, 5, 7, 8, 9 texels in turn (and every 13th row is marked whole), so that consecutive slots
cross a row's end at every position u of a 4-slot and of an 8-slot run and some runs hold several breaks; every fourth
row starts at the apron texel left of the texture (x = -0.5 / R, cell column -1 at levels finer than the texture);
shell 1's coarsest segment has 3 slots (shorter than one run); shell 0's slots are no multiple of 8, so shell 1's
segments start inside a run.  Past the last segment slot_xy and dF hold NaN.
Geometries: default (levels 0-5 dense with both features per pass, 6-15 hashed and finer than every texture), h10
(log2_hashmap_size 10: levels 2, 3 hashed AND coarser than the 64-texel texture — the forward's REUSE and the
backward's MERGE instances on hashed levels — and finer than the others), g100 (levels 1, 2 dense with one feature per
pass).  The sibling walk on and off, 16 workgroups (cuts at 256 slots) and one per compute unit; a shell without alpha.
"""
import functools
import types

import numpy as np
import pytest
import torch

import nt_encode_grad_restated as R
import test_nt_encode_grad as T
import test_nt_encode_siblings as S
from oracle import tcnn_like
from oracle.tcnn_like import GridGeometry, PRIME_Y

K = 2
TEX_RES = (64, 32, 16, 8)
MAX_RAYS = 1024
ROW_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9)
SHORT_SD = 7                       # (shell 1, degree 3): 3 slots
GRIDS = {"default": {}, "h10": dict(log2_hashmap_size=10), "g100": dict(base_resolution=100, per_level_scale=1.3)}
M32 = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _geom(name):
    return GridGeometry(**GRIDS[name])


def _capacity():
    cap = K * sum(min(4 * MAX_RAYS, (r + 2) ** 2) for r in TEX_RES)
    return (cap + 255) // 256 * 256 + 256


def _texels(sd):
    """Marked texels of segment sd in raster order (indices into the (R + 2)^2 extended grid)."""
    res = TEX_RES[sd % R.MAX_DEG]
    W = res + 2
    if sd == SHORT_SD:
        return np.array([3 * W + 4, 3 * W + 5, 4 * W + 1])
    out = []
    for row in range(W):
        if row % 13 == 12:
            cols = np.arange(W)
        else:
            c = ROW_COUNTS[(row + sd) % len(ROW_COUNTS)]
            c0 = 0 if row % 4 == 0 else (row * 5 + sd) % (W - c + 1)
            cols = c0 + np.arange(c)
        out.append(row * W + cols)
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def _slots():
    tex = [_texels(sd) for sd in range(K * R.MAX_DEG)]
    seg = np.concatenate([[0], np.cumsum([len(t) for t in tex])])
    xy = np.full((_capacity(), 2), np.nan, np.float32)
    for sd, t in enumerate(tex):
        xy[seg[sd]:seg[sd + 1]] = R.texel_centres(TEX_RES[sd % R.MAX_DEG], t)
    xy.setflags(write=False)
    return seg, xy


# ---- the split helpers restated (csrc/nt_enc_common.h), fp32 operation by operation

def cell_row(geom, l, y):
    py = y * np.float32(geom.scale[l]) + np.float32(0.5)
    cyf = np.floor(py)
    fy = py - cyf                                   # v_fract_f32: the subtraction is exact
    gy = np.float32(1.0) - fy
    cy = cyf.astype(np.int64) & M32
    if R.level_hashed(geom.res[l], geom.size[l]):
        return cy, fy, gy, (cy * PRIME_Y) & M32, (((cy + 1) & M32) * PRIME_Y) & M32
    return cy, fy, gy, (cy * geom.res[l]) & M32, None


def cell_col(geom, l, x, row):
    cy, fy, gy, h0, h1 = row
    px = x * np.float32(geom.scale[l]) + np.float32(0.5)
    cxf = np.floor(px)
    fx = px - cxf
    gx = np.float32(1.0) - fx
    cx = cxf.astype(np.int64) & M32
    w = np.stack([gx * gy, fx * gy, gx * fy, fx * fy])
    size, res = geom.size[l], geom.res[l]
    if h1 is not None:
        mask = size - 1
        idx = np.stack([(cx ^ h0) & mask, (((cx + 1) & M32) ^ h0) & mask, (cx ^ h1) & mask, (((cx + 1) & M32) ^ h1) & mask])
    else:
        r0 = (cx + h0) & M32
        idx = np.stack([r0, (r0 + 1) & M32, (r0 + res) & M32, (r0 + res + 1) & M32])
        wrap = (idx[3] >= size) | (idx[0] > idx[3])
        idx = np.where(wrap[None, :], idx % size, idx)
    return idx, w


# ---- CPU

@pytest.mark.parametrize("geom_name", list(GRIDS))
def test_split_helpers_give_the_whole_cells_bits(geom_name):
    geom = _geom(geom_name)
    checked = 0
    for res in TEX_RES:
        W = res + 2
        xy = R.texel_centres(res, np.arange(W * W))
        y_rows = xy[:, 1].reshape(W, W).view(np.uint32)
        assert (y_rows == y_rows[:, :1]).all(), "texels of one row: one y, bit for bit"
        assert len(np.unique(y_rows[:, 0])) == W
        for l in range(geom.n_levels):
            want_idx, want_w = tcnn_like._grid_cells(geom, l, torch.from_numpy(xy))
            # the row part from ONE texel of each row, used for the whole row
            first = np.repeat(xy[::W, 1], W)
            idx, w = cell_col(geom, l, xy[:, 0], cell_row(geom, l, first))
            assert w.dtype == np.float32 and want_w.dtype == torch.float32
            assert np.array_equal(w.view(np.uint32), want_w.numpy().view(np.uint32)), (res, l)
            assert np.array_equal(idx, want_idx.numpy()), (res, l)
            checked += idx.size
    assert checked > 16 * 4 * 66 * 66


def test_frame_breaks_rows_at_every_position_of_a_run():
    seg, xy = _slots()
    assert seg[-1] + 8 <= _capacity() and np.isnan(xy[seg[-1]:]).all() and np.isfinite(xy[:seg[-1]]).all()
    assert seg[R.MAX_DEG] % 8 != 0 and seg[R.MAX_DEG] % 4 != 0          # shell 1 starts inside a run
    assert seg[SHORT_SD + 1] - seg[SHORT_SD] == 3
    ybits = xy[:, 1].view(np.uint32)
    for unroll in (4, 8):
        where, several = set(), 0
        for sd in range(K * R.MAX_DEG):
            a, b = int(seg[sd]), int(seg[sd + 1])
            for s0 in range(a & ~(unroll - 1), b, unroll):
                us = [u for u in range(1, unroll) if a < s0 + u < b and s0 + u - 1 >= a
                      and ybits[s0 + u] != ybits[s0 + u - 1]]
                where |= set(us)
                several += len(us) > 1
        assert where == set(range(1, unroll)) and several > 10, (unroll, where, several)
    # a marked apron texel left of every texture, and a row of one texel
    for sd in range(K * R.MAX_DEG):
        if sd != SHORT_SD:
            assert (xy[seg[sd]:seg[sd + 1], 0] < 0).sum() >= 2
    # the level classes the docstring names
    cls = R.level_classes(_geom("h10"))
    assert [c[0] for c in cls[:4]] == [False, False, True, True]
    assert R.merges(_geom("h10"), 2, 64) and R.merges(_geom("h10"), 3, 64) and not R.merges(_geom("h10"), 4, 64)
    assert not R.merges(_geom("h10"), 2, 32)
    cls = R.level_classes(_geom("g100"))
    assert cls[1][:2] == (False, 1) and cls[2][:2] == (False, 1)
    d = _geom("default")
    assert any(R.merges(d, l, 64) for l in range(6)) and any(not R.merges(d, l, 8) for l in range(6))


def test_switch_refuses_what_it_does_not_know():
    from volsurfs_amd import _lib
    from volsurfs_amd.neural_textures import NeuralTextureBank
    assert "vsa_nt_encode_row_terms" in _lib.declared_prototypes()
    for bad in ((-1, 0), (2, 0), (0, -1), (1, 2)):
        with pytest.raises(_lib.VolsurfsHipError):
            NeuralTextureBank.encode_row_terms(*bad)
    for f in (0, 1):
        for b in (0, 1):
            NeuralTextureBank.encode_row_terms(f, b)
    NeuralTextureBank.encode_row_terms(S._define("NT_ENC_ROW_TERMS_FWD"), S._define("NT_ENC_ROW_TERMS_BWD"))


# ---- GPU

@pytest.fixture
def switches():
    """vsa_nt_encode_row_terms and vsa_nt_encode_config for the test; the library's defaults again afterwards."""
    from volsurfs_amd.neural_textures import NeuralTextureBank

    def set_(row, siblings, grid):
        NeuralTextureBank.encode_row_terms(row, row)
        NeuralTextureBank.encode_config(siblings, grid)
    yield set_
    NeuralTextureBank.encode_row_terms(S._define("NT_ENC_ROW_TERMS_FWD"), S._define("NT_ENC_ROW_TERMS_BWD"))
    NeuralTextureBank.encode_config(S._define("NT_ENC_SIBLING_GROUPS"), 0)


@functools.lru_cache(maxsize=None)
def _bank(geom_name, inner_solid):
    from volsurfs_amd.neural_textures import NeuralTextureBank
    bank = NeuralTextureBank(K, MAX_RAYS, textures_res=TEX_RES, grid=GRIDS[geom_name] or None,
                             inner_solid=inner_solid)
    assert bank.slot_capacity == _capacity() and bank.n_entries == _geom(geom_name).offset[-1]
    seg, xy = _slots()
    bank.seg_start.copy_(torch.tensor(seg, dtype=torch.int32))
    bank.slot_xy.copy_(torch.from_numpy(xy.copy()))
    g = torch.Generator().manual_seed(5)
    bank.tables_h.copy_(torch.randn(bank.tables_h.shape, generator=g).half())
    return bank


def _features(bank):
    seg, xy = _slots()
    bank.seg_start.copy_(torch.tensor(seg, dtype=torch.int32))
    bank.slot_xy.copy_(torch.from_numpy(xy.copy()))
    bank.features.fill_(-7.0)                      # what the launch does not write keeps this
    bank.encode()
    torch.cuda.synchronize()
    return bank.features.cpu().numpy().view(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("inner_solid", [False, True], ids=["alpha", "shell0_no_alpha"])
@pytest.mark.parametrize("geom_name", list(GRIDS))
def test_forward_features_keep_their_bits(switches, geom_name, inner_solid):
    bank, geom = _bank(geom_name, inner_solid), _geom(geom_name)
    seg, xy = _slots()
    switches(0, 0, 0)
    want = _features(bank)
    lm = bank.features_level_major().cpu()
    checked = 0
    for sd in range(K * R.MAX_DEG):                # the oracle, once
        a, b = int(seg[sd]), int(seg[sd + 1])
        s, d = divmod(sd, R.MAX_DEG)
        for typ in range(2):
            x = bank.tex_index(s, typ, d)
            if not bank.tex_channels(x):
                continue
            ref = tcnn_like.hashgrid_forward(geom, bank.tables_h[x].cpu().float(), torch.from_numpy(xy[a:b].copy()))
            got = lm[typ, :, a:b].permute(1, 0, 2).reshape(-1, 32)
            assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (sd, typ)
            checked += 1
    assert checked == (12 if inner_solid else 16)
    assert (lm[1, :, :seg[R.MAX_DEG]] == -7).all() == inner_solid
    for siblings in (0, 1):
        for grid in (16, 0):
            switches(0, siblings, grid)
            off = _features(bank)
            switches(1, siblings, grid)
            on = _features(bank)
            assert np.array_equal(off, want), "switch off, siblings %d, grid %d" % (siblings, grid)
            assert np.array_equal(on, want), "switch on, siblings %d, grid %d: %d feature halves differ" % (
                siblings, grid, int((on != want).sum()))


class _Case:
    """The float64 reference of one geometry on the frame above (the fields test_nt_encode_grad._check reads)."""

    def __init__(self, geom_name):
        seg, xy = _slots()
        self.geom_name, self.geom = geom_name, _geom(geom_name)
        self.frame = R.Frame(K, seg, xy, TEX_RES)
        rng = np.random.default_rng(41)
        dF = np.full((2, 16, _capacity(), 2), np.nan, np.float16)
        for sd in range(K * R.MAX_DEG):
            n = int(seg[sd + 1] - seg[sd])
            for typ in range(2):
                dF[typ, :, seg[sd]:seg[sd + 1]] = R.gradient_dynamic_range(rng, n) if sd == 1 else R.gradient_normal(rng, n)
        self.dF = dF
        self.dfsum = R.abs_sum_rounded_up(dF, self.frame)
        Sm, A, n, H, P = R.table_grad_f64(self.geom, self.frame, dF, self.dfsum)
        self.shape, self.t = Sm.shape, n > 0
        self.where = np.argwhere(self.t)
        self.S, self.A, self.n, self.H, self.P = (v[self.t] for v in (Sm, A, n, H, P))


@functools.lru_cache(maxsize=None)
def _case(geom_name):
    return _Case(geom_name)


def _whole_planes(geom, cars, grid, siblings):
    """{(texture, level, feature)} one piece of the backward launch covers whole: what it stores under grads_zeroed
    (test_nt_encode_siblings._whole_planes at this file's texture resolutions)."""
    cls = R.level_classes(geom)
    whole = set()
    dense = [(l, None) if cls[l][1] == 2 else (l, f) for l in range(geom.n_levels) if not cls[l][0]
             for f in range(1 if cls[l][1] == 2 else 2)]
    for _, (l, f), typ, c, first, last in S.plain_pieces(grid, dense, cars, S._define("NT_ENC_OVH_BD"), lambda pl, d: 16):
        if (first, last) == (c.begin, c.end):
            whole |= {(c.tex(typ), l, ff) for ff in ((0, 1) if f is None else (f,))}
    levels = S._hashed_levels(geom)
    w = S._weight(geom, TEX_RES, 14)
    ovh = S._define("NT_ENC_OVH_BH")
    if siblings and S.grid_ok(grid, 4):
        for _, _, _, l, typ, f, c, first, last in S.sibling_pieces(grid, 4, cars, levels, ovh, w):
            if (first, last) == (c.begin, c.end):
                whole.add((c.tex(typ), l, f))
    else:
        planes = [(l, f) for l in levels for f in range(2)]
        for _, (l, f), typ, c, first, last in S.plain_pieces(grid, planes, cars, ovh, lambda pl, d: w(pl[0], d)):
            if (first, last) == (c.begin, c.end):
                whole.add((c.tex(typ), l, f))
    return whole


@pytest.mark.gpu
@pytest.mark.parametrize("inner_solid", [False, True], ids=["alpha", "shell0_no_alpha"])
@pytest.mark.parametrize("geom_name", list(GRIDS))
def test_backward_holds_the_bound_and_stored_planes_keep_their_bits(switches, geom_name, inner_solid):
    case = _case(geom_name)
    geom = case.geom
    bank = _bank(geom_name, inner_solid)
    T._load(bank, case)
    ref = S._without_alpha_of_shell0(case) if inner_solid else case
    seg, _ = _slots()
    cars = S.carriers(seg, (0,) if inner_solid else ())
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    gs = 4096.0
    one = np.zeros(case.shape, bool)
    one[tuple(ref.where[ref.P == 1].T)] = True             # one add of one integer sum: the same float in any run
    prefill = T._prefill(case, gs)
    for siblings in (0, 1):
        for grid in (16, 32, 0):
            n_wg = grid or cus
            switches(0, siblings, grid)
            off = T._launch(bank, "one", gs, grads_zeroed=True)
            T._check("switch off, siblings %d, grid %d, stored" % (siblings, grid), ref, off, gs)
            switches(1, siblings, grid)
            on = T._launch(bank, "one", gs, grads_zeroed=True)
            T._check("switch on, siblings %d, grid %d, stored" % (siblings, grid), ref, on, gs)
            stored = _whole_planes(geom, cars, n_wg, bool(siblings))     # the same walk, the same cuts, on and off
            same = (S._mask(geom, case.shape, stored) | one) & ref.t
            assert len(stored) > 50 and same.sum() > 2000
            diff = on.view(np.uint32)[same] != off.view(np.uint32)[same]
            print("siblings %d, grid %d: %d planes stored in both runs, %d floats compared" % (
                siblings, n_wg, len(stored), int(same.sum())))
            assert not diff.any(), "siblings %d, grid %d: %d floats of planes both runs store differ" % (
                siblings, grid, int(diff.sum()))
            T._check("switch on, siblings %d, grid %d, atomics on a pre-filled buffer" % (siblings, grid), ref,
                     T._launch(bank, "one", gs, prefill), gs, prefill)
    if not inner_solid:                                      # the range and phased entry points share the piece
        switches(1, 0, 0)
        by_shell = np.zeros(case.shape, np.float32)
        bank.tables.grad = torch.zeros(tuple(bank.tables.shape), device="cuda")
        for s in range(K):
            bank.backward_encode(gs, shells=(s, s + 1), grads_zeroed=False)
        torch.cuda.synchronize()
        by_shell = bank.tables.grad.cpu().numpy()
        T._check("switch on, shell by shell", ref, by_shell, gs)
        from volsurfs_amd.parallel import StepSignals
        sg = StepSignals(K, "cuda", [1, 2], 0, reserve_cus=0)
        sg.signal_weights()
        bank.tables.grad = torch.zeros(tuple(bank.tables.shape), device="cuda")
        bank.backward_encode_phased(gs, sg, grads_zeroed=False)
        torch.cuda.synchronize()
        T._check("switch on, phased", ref, bank.tables.grad.cpu().numpy(), gs)
