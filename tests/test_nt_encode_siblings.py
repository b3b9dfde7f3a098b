"""The sibling-group walk of the hash-grid encode kernels (csrc/nt_common.h: nt_sibling_stretch, nt_sibling_share,
nt_for_each_sibling_piece; csrc/nt_encode.hip; switch: vsa_nt_encode_config).

THE RULE restated here, from the header.  Carriers are the (shell, degree) with a non-empty segment and at least one
active texture, in texture order (the colour texture's lane carries, the alpha texture's where there is no colour
texture).  The axis is level-major; on a level a carrier takes ovh * 16 of spacing and then units * w, units =
ceil(length / 256), w = max(1, wt * n_sib / G), wt the plain walk's unit weight, n_sib = types * (G / 2).  For a grid
that is a multiple of 8 G, block b has r = b % 8G, group = (b // 8G) * 8 + r % 8, member = r // 8, and the group's
stretch is [total * group // n_groups, total * (group + 1) // n_groups), n_groups = grid / G.  A unit belongs to the
stretch that holds its start.  Of the stretch's units [ua, ub) of a carrier, member m takes sibling m % n_sib (type =
sibling % types, feature = sibling // types) and, of the r = G / n_sib members of that sibling, share j = m // n_sib:
units [ua + n j // r, ua + n (j + 1) // r), n = ub - ua.

CPU: that rule visits every (sibling plane, carrier, unit) exactly once and hands the members of a group identical
ranges where all siblings exist; a grid of 20 is refused.  GPU: the forward's features are those of the plain walk bit
for bit; the backward holds the float64 bound of test_nt_encode_grad through that file's harness, and every plane that
both walks flush by stores (found by restating both walks' cuts) carries the same bits.  Cut planes go through float
atomics in both walks and are held to the bound only.
"""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import nt_encode_grad_restated as R
import test_nt_encode_grad as T

UNIT = R.UNIT
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "volsurfs_amd", "csrc", "nt_encode.hip")


@functools.lru_cache(maxsize=None)
def _define(name):
    with open(_SRC) as f:
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, f.read()).group(1))


# ---- the rule

def grid_ok(grid, G):
    return grid > 0 and grid % (8 * G) == 0


def stretch(block, grid, G, total):
    r, n_groups = block % (8 * G), grid // G
    group, member = block // (8 * G) * 8 + r % 8, r // 8
    return group, member, total * group // n_groups, total * (group + 1) // n_groups


def share(member, G, n_sib, ua, ub):
    r, j, n = G // n_sib, member // n_sib, ub - ua
    return member % n_sib, ua + n * j // r, ua + n * (j + 1) // r


class Carrier:
    def __init__(self, sd, begin, end, typs):
        self.sd, self.begin, self.end, self.types = sd, int(begin), int(end), tuple(typs)
        self.shell, self.deg = divmod(sd, R.MAX_DEG)
        self.units = (self.end - self.begin + UNIT - 1) // UNIT

    def tex(self, typ):
        return (self.shell * 2 + typ) * R.MAX_DEG + self.deg


def carriers(seg, no_alpha_shells=()):
    out = []
    for sd in range(len(seg) - 1):
        typs = (0,) if sd // R.MAX_DEG in no_alpha_shells else (0, 1)
        if seg[sd + 1] > seg[sd]:
            out.append(Carrier(sd, seg[sd], seg[sd + 1], typs))
    return out


def _units_in(lo, hi, t0, units, w):
    """Units of a texture whose units start at t0 (weight w each) that start inside [lo, hi)."""
    span = units * w
    if t0 >= hi:
        return 0, 0
    a, b = max(lo - t0, 0), min(hi - t0, span)
    if b <= a:
        return 0, 0
    return -(-a // w), -(-b // w)


def sibling_pieces(grid, G, cars, levels, ovh, weight):
    """[(block, group, member, level, type, feature, carrier, first, last)] of the sibling walk."""
    NF = G // 2

    def uw(l, c):
        return max(1, weight(l, c.deg) * len(c.types) * NF // G)
    total = sum(ovh * 16 + c.units * uw(l, c) for l in levels for c in cars)
    out = []
    for block in range(grid):
        group, member, lo, hi = stretch(block, grid, G, total)
        c0 = 0
        for l in levels:
            for c in cars:
                t0, w = c0 + ovh * 16, uw(l, c)
                c0 = t0 + c.units * w
                ua, ub = _units_in(lo, hi, t0, c.units, w)
                if ub <= ua:
                    continue
                sib, ma, mb = share(member, G, len(c.types) * NF, ua, ub)
                if mb <= ma:
                    continue
                out.append((block, group, member, l, c.types[sib % len(c.types)], sib // len(c.types), c,
                            c.begin + ma * UNIT, min(c.begin + mb * UNIT, c.end)))
    return out


def plain_pieces(grid, planes, cars, ovh, weight):
    """[(block, plane, type, carrier, first, last)] of nt_for_each_piece (one texture per piece, equal shares):
    plane-major, within a plane the textures in index order."""
    texs = sorted(((c.tex(t), t, c) for c in cars for t in c.types), key=lambda x: x[0])
    total = sum(ovh * 16 + c.units * weight(pl, c.deg) for pl in planes for _, _, c in texs)
    out = []
    for block in range(grid):
        lo, hi = total * block // grid, total * (block + 1) // grid
        c0 = 0
        for pl in planes:
            for _, typ, c in texs:
                t0, w = c0 + ovh * 16, weight(pl, c.deg)
                c0 = t0 + c.units * w
                ua, ub = _units_in(lo, hi, t0, c.units, w)
                if ub > ua:
                    out.append((block, pl, typ, c, c.begin + ua * UNIT, min(c.begin + ub * UNIT, c.end)))
    return out


def _hashed_levels(geom):
    return [l for l in range(geom.n_levels) if R.level_classes(geom)[l][0]]


def _weight(geom, tex_res, lo_w):
    """The unit weights of nt_encode.hip: 16 where cells are coarser than texels, else 15 (forward) / 14 (backward)."""
    return lambda l, deg: 16 if np.float32(geom.scale[l]) < np.float32(tex_res[deg]) else lo_w


# ---- CPU

BIG_SEG = (70001, 40000, 20003, 9000, 120000, 65536, 0, 5000, 1, 300, 33000, 77)
SETS = {"small": (T.SEG_LEN, ()), "small, shell 0 without alpha": (T.SEG_LEN, (0,)),
        "large, shell 1 without alpha": (BIG_SEG, (1,))}


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("mult", [8, 16, 0])
@pytest.mark.parametrize("G", [2, 4])
def test_split_visits_every_unit_once(G, mult, name):
    grid = mult * G if mult else 256
    assert grid_ok(grid, G)
    lens, no_alpha = SETS[name]
    assert {0, 1} <= set(lens) and any(n % UNIT for n in lens if n > UNIT)
    seg = np.concatenate([[0], np.cumsum(lens)])
    cars = carriers(seg, no_alpha)
    geom = T._geom("default")
    levels = _hashed_levels(geom)
    ovh = _define("NT_ENC_OVH_FH" if G == 2 else "NT_ENC_OVH_BH")
    pieces = sibling_pieces(grid, G, cars, levels, ovh, _weight(geom, T.TEX_RES, 15 if G == 2 else 14))
    seen = {(l, t, f, c.sd): np.zeros(c.units, np.int64) for l in levels for c in cars for t in c.types
            for f in range(G // 2)}
    by_group = {}
    for block, group, member, l, typ, feat, c, first, last in pieces:
        assert (group, member) == stretch(block, grid, G, 1)[:2] and 0 <= member < G and 0 <= group < grid // G
        assert c.begin <= first < last <= c.end and (first - c.begin) % UNIT == 0
        assert last == c.end or (last - c.begin) % UNIT == 0
        seen[(l, typ, feat, c.sd)][(first - c.begin) // UNIT:(last - c.begin + UNIT - 1) // UNIT] += 1
        by_group.setdefault((group, l, c.sd), []).append((member, typ, feat, first, last))
    for key, n in seen.items():
        assert (n == 1).all(), (key, n)
    # every (group, member) is one block; the members of a group sit on one XCD (id % 8) within 8 G consecutive ids
    ids = {}
    for b in range(grid):
        g, m = stretch(b, grid, G, 1)[:2]
        ids.setdefault(g, {})[m] = b
    assert len(ids) == grid // G
    for g, mem in ids.items():
        assert sorted(mem) == list(range(G)) and len({b % 8 for b in mem.values()}) == 1
        assert len({b // (8 * G) for b in mem.values()}) == 1
    full = 0
    for (group, l, sd), got in by_group.items():
        c = next(c for c in cars if c.sd == sd)
        if len(c.types) == 2:      # all siblings exist: one range, every member on its own plane
            assert len({(first, last) for _, _, _, first, last in got}) == 1, (group, l, sd, got)
            assert sorted((m, t, f) for m, t, f, _, _ in got) == [(m, m & 1, m >> 1) for m in range(G)]
            full += 1
        else:                      # the members share the carrier's range
            assert len(got) <= G and len({m for m, *_ in got}) == len(got)
    assert full > 0


def test_other_grids_take_the_plain_walk():
    assert not grid_ok(20, 2) and not grid_ok(20, 4) and not grid_ok(16, 4) and not grid_ok(0, 2)
    assert grid_ok(16, 2) and grid_ok(32, 4) and grid_ok(256, 2) and grid_ok(256, 4)


def test_config_refuses_what_it_does_not_know():
    from volsurfs_amd import _lib
    from volsurfs_amd.neural_textures import NeuralTextureBank
    assert "vsa_nt_encode_config" in _lib.declared_prototypes()
    for bad in ((-1, 0), (4, 0), (0, -1), (1, 4097)):
        with pytest.raises(_lib.VolsurfsHipError):
            NeuralTextureBank.encode_config(*bad)
    for mode in (0, 1, 2, 3, _define("NT_ENC_SIBLING_GROUPS")):
        NeuralTextureBank.encode_config(mode, 0)


# ---- GPU

@pytest.fixture
def config():
    """vsa_nt_encode_config for the test; the library's default again afterwards."""
    from volsurfs_amd.neural_textures import NeuralTextureBank

    def set_(siblings, grid=0):
        NeuralTextureBank.encode_config(siblings, grid)
    yield set_
    NeuralTextureBank.encode_config(_define("NT_ENC_SIBLING_GROUPS"), 0)


@functools.lru_cache(maxsize=None)
def _own_bank(geom_name, inner_solid):
    from volsurfs_amd.neural_textures import NeuralTextureBank
    bank = NeuralTextureBank(T.K, T.MAX_RAYS, textures_res=T.TEX_RES, grid=T.GRIDS[geom_name] or None,
                             inner_solid=inner_solid)
    assert bank.slot_capacity == T._capacity()
    seg, xy = T._slots()
    bank.seg_start.copy_(torch.tensor(seg, dtype=torch.int32))
    bank.slot_xy.copy_(torch.from_numpy(xy))
    g = torch.Generator().manual_seed(5)
    bank.tables_h.copy_(torch.randn(bank.tables_h.shape, generator=g).half())
    return bank


def _features(bank):
    bank.features.fill_(-7.0)                      # what the launch does not write keeps this
    bank.encode()
    torch.cuda.synchronize()
    return bank.features.cpu().numpy().view(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("inner_solid", [False, True], ids=["alpha", "shell0_no_alpha"])
@pytest.mark.parametrize("geom_name", ["default", "g100"])
def test_forward_features_are_the_plain_walks(config, geom_name, inner_solid):
    bank = _own_bank(geom_name, inner_solid)
    config(0, 0)
    want = _features(bank)
    lm = bank.features_level_major().cpu().numpy()
    seg, _ = T._slots()
    assert np.isfinite(lm[0, :, :seg[-1]].astype(np.float32)).all() and (lm[0, :, :seg[-1]] != -7).any()
    assert (lm[1, :, :seg[R.MAX_DEG]] == -7).all() == inner_solid          # shell 0's alpha planes: not written
    for grid in (16, 32, 0, 20):                                          # (20: the fallback)
        config(1, grid)
        got = _features(bank)
        assert np.array_equal(got, want), "grid %d: %d feature halves differ" % (grid, int((got != want).sum()))
        config(0, grid)
        assert np.array_equal(_features(bank), want), "plain walk, grid %d" % grid


def _whole_planes(geom, cars, grid, siblings):
    """{(texture, level, feature)}: the planes one piece of the backward launch covers whole — what it stores under
    grads_zeroed.  Dense planes by the plain walk, hashed ones by the walk the launch takes."""
    cls = R.level_classes(geom)
    whole = set()
    dense = [(l, None) if cls[l][1] == 2 else (l, f) for l in range(geom.n_levels) if not cls[l][0]
             for f in range(1 if cls[l][1] == 2 else 2)]
    for _, (l, f), typ, c, first, last in plain_pieces(grid, dense, cars, _define("NT_ENC_OVH_BD"), lambda pl, d: 16):
        if (first, last) == (c.begin, c.end):
            whole |= {(c.tex(typ), l, ff) for ff in ((0, 1) if f is None else (f,))}
    levels = _hashed_levels(geom)
    w = _weight(geom, T.TEX_RES, 14)
    ovh = _define("NT_ENC_OVH_BH")
    if siblings and grid_ok(grid, 4):
        for _, _, _, l, typ, f, c, first, last in sibling_pieces(grid, 4, cars, levels, ovh, w):
            if (first, last) == (c.begin, c.end):
                whole.add((c.tex(typ), l, f))
    else:
        planes = [(l, f) for l in levels for f in range(2)]
        for _, (l, f), typ, c, first, last in plain_pieces(grid, planes, cars, ovh, lambda pl, d: w(pl[0], d)):
            if (first, last) == (c.begin, c.end):
                whole.add((c.tex(typ), l, f))
    return whole


def _mask(geom, shape, planes):
    m = np.zeros(shape, bool)
    for tex, l, f in planes:
        m[tex, geom.offset[l]:geom.offset[l + 1], f] = True
    return m


def _without_alpha_of_shell0(case):
    """The reference of a bank whose shell 0 has no alpha model: those textures get no gradient at all."""
    keep = ~np.isin(case.where[:, 0], [R.MAX_DEG + d for d in range(R.MAX_DEG)])   # textures 4 .. 7
    t = case.t.copy()
    t[R.MAX_DEG:2 * R.MAX_DEG] = False
    return types.SimpleNamespace(geom_name=case.geom_name + ", shell 0 without alpha", shape=case.shape, t=t,
                                 where=case.where[keep], S=case.S[keep], A=case.A[keep], n=case.n[keep],
                                 H=case.H[keep], P=case.P[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("inner_solid", [False, True], ids=["alpha", "shell0_no_alpha"])
@pytest.mark.parametrize("geom_name", ["default", "g100"])
def test_backward_holds_the_bound_and_stored_planes_keep_their_bits(config, geom_name, inner_solid):
    case = T._case(geom_name, "normal")
    geom = case.geom
    bank = _own_bank(geom_name, True) if inner_solid else T._bank(geom_name, False)
    T._load(bank, case)
    ref = _without_alpha_of_shell0(case) if inner_solid else case
    seg, _ = T._slots()
    cars = carriers(seg, (0,) if inner_solid else ())
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    gs = 4096.0
    one = np.zeros(case.shape, bool)
    one[tuple(ref.where[ref.P == 1].T)] = True             # one add of one integer sum: the same float in any walk
    prefill = T._prefill(case, gs)
    for grid in (16, 32, 0, 20):                            # (16 and 20: the backward's fallback)
        n_wg = grid or cus
        config(0, grid)
        plain = T._launch(bank, "one", gs, grads_zeroed=True)
        T._check("plain walk, grid %d, stored" % grid, ref, plain, gs)
        config(1, grid)
        got = T._launch(bank, "one", gs, grads_zeroed=True)
        T._check("siblings, grid %d, stored" % grid, ref, got, gs)
        both = _whole_planes(geom, cars, n_wg, False) & _whole_planes(geom, cars, n_wg, True)
        same = (_mask(geom, case.shape, both) | one) & ref.t
        assert len(both) > 100 and same.sum() > 10000
        diff = got.view(np.uint32)[same] != plain.view(np.uint32)[same]
        print("grid %d: %d planes stored by both walks, %d floats compared" % (n_wg, len(both), int(same.sum())))
        assert not diff.any(), "grid %d: %d floats of planes both walks store differ" % (grid, int(diff.sum()))
        if not grid_ok(n_wg, 4):                            # the same walk: the same cuts
            assert _whole_planes(geom, cars, n_wg, True) == _whole_planes(geom, cars, n_wg, False)
        T._check("siblings, grid %d, atomics on a pre-filled buffer" % grid, ref,
                 T._launch(bank, "one", gs, prefill), gs, prefill)
