"""UV atlases on the GPU (csrc/atlas.hip, volsurfs_amd/atlas.py).

`restate` below is the numpy restatement of the rules in include/volsurfs_hip.h: the same fp32 / fp64 operations in the
same order, the same joins, chart numbering, pack bisection, UV formula, rasterization and splits, so the kernels are
held to it bit for bit.  Atlas validity (UVs in [0, 1], no flipped face, at least half of every face's area kept, no
texel covered twice, charts 2 * padding texels apart), an fp64 triangle-overlap check, the pack error, the files and
the path into neural-texture training are checked on top."""
import os

import numpy as np
import pytest
import torch

from volsurfs_amd import atlas
from volsurfs_amd._lib import VolsurfsHipError
from volsurfs_amd.mesh import icosphere

from uv_raster_restated import raster

AX_U = np.array([1, 2, 2, 0, 0, 1])
AX_V = np.array([2, 1, 0, 2, 1, 0])
DEPTH_CAP = 24
MAX_ROUNDS = 100


# ------------------------------------------------------------------------------------------------- restatement

def _argmax6(x, y, z):
    return np.argmax(np.stack([x, -x, y, -y, z, -z], 1), 1)        # first maximum: ties to the earlier direction


def _labels(P, F):
    p0, p1, p2 = P[F[:, 0]], P[F[:, 1]], P[F[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    nv = np.zeros((len(P), 3), np.float32)
    np.add.at(nv, F.reshape(-1), np.repeat(n, 3, axis=0))          # per vertex in ascending face order, fp32
    s = (nv[F[:, 0]] + nv[F[:, 1]]) + nv[F[:, 2]]
    cand = _argmax6(s[:, 0], s[:, 1], s[:, 2])
    comp = n[np.arange(len(F)), cand >> 1].astype(np.float64)
    dn = np.where(cand & 1, -comp, comp)
    n64 = n.astype(np.float64)
    nn = (n64[:, 0] * n64[:, 0] + n64[:, 1] * n64[:, 1]) + n64[:, 2] * n64[:, 2]
    lab = np.where((dn >= 0) & (4.0 * (dn * dn) >= nn), cand, _argmax6(n[:, 0], n[:, 1], n[:, 2]))
    lab[(n == 0).all(1)] = 0
    return lab


def _join_pairs(F, lab):
    V = int(F.max()) + 1
    a, b = F, np.roll(F, -1, axis=1)
    key = (np.minimum(a, b) * V + np.maximum(a, b)).reshape(-1)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    _, first, cnt = np.unique(ks, return_index=True, return_counts=True)
    first = first[cnt == 2]
    s0, s1 = order[first], order[first + 1]
    f0, f1 = s0 // 3, s1 // 3
    ok = (F[f0, s0 % 3] == F[f1, (s1 % 3 + 1) % 3]) & (lab[f0] == lab[f1])
    return f0[ok], f1[ok]


def _components(n, f0, f1):
    """Minimum index of every element's component."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = coo_matrix((np.ones(len(f0)), (f0, f1)), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    root = np.full(comp.max() + 1, n)
    np.minimum.at(root, comp, np.arange(n))
    return root[comp]


def _ord(x):
    b = np.asarray(x, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _unord(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _boxes(P, F, lab, cidx, C):
    fi = np.repeat(np.arange(len(F)), 3)
    v = F.reshape(-1)
    ku = _ord(P[v, AX_U[lab[fi]]])
    kv = _ord(P[v, AX_V[lab[fi]]])
    box = np.zeros((C, 4), np.uint32)
    box[:, 0] = box[:, 2] = 0xFFFFFFFF
    c = cidx[fi]
    np.minimum.at(box[:, 0], c, ku)
    np.maximum.at(box[:, 1], c, ku)
    np.minimum.at(box[:, 2], c, kv)
    np.maximum.at(box[:, 3], c, kv)
    return _unord(box)


def _sides(e, s, R, p):
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.ceil(e * np.float32(s))
        ok = t <= np.float32(R)
        return np.where(ok, np.where(ok, t, 0).astype(np.int64) + 2 * p, R + 1)


def _walk(W, H, R):
    """Next-fit shelves over sorted rectangles: (fit, [(start, y)], prefix)."""
    pre = np.concatenate([[0], np.cumsum(W)])
    i, y, out, C = 0, 0, [], len(W)
    while i < C:
        j = int(np.searchsorted(pre, pre[i] + R, side="right")) - 1
        if j == i:
            return False, out, pre
        out.append((i, y))
        y += int(H[i])
        if y > R:
            return False, out, pre
        i = j
    return True, out, pre


def _pack(ew, eh, R, p):
    """(s, offsets [C, 2]) by the header's bisection, or a VolsurfsHipError when nothing fits."""
    C = len(ew)
    ids = np.arange(C)

    def step(bits):
        s = np.array([bits], np.uint32).view(np.float32)[0]
        W, H = _sides(ew, s, R, p), _sides(eh, s, R, p)
        order = np.lexsort((ids, -W, -H))
        fit, sh, pre = _walk(W[order], H[order], R)
        return fit, order, sh, pre, s

    if p > 0:
        per = R // (2 * p)
        if per == 0 or -(-C // per) * 2 * p > R:
            raise VolsurfsHipError(atlas.full_message(C, R, p, atlas.min_resolution(C, p)))
    lo, hi = 0, 0x7F800000
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if step(mid)[0]:
            lo = mid
        else:
            hi = mid
    fit, order, sh, pre, s = step(lo)
    assert fit
    starts = np.array([a for a, _ in sh])
    ys = np.array([b for _, b in sh])
    k = np.arange(C)
    shelf = np.searchsorted(starts, k, side="right") - 1
    off = np.zeros((C, 2), np.int64)
    off[order, 0] = pre[k] - pre[starts[shelf]]
    off[order, 1] = ys[shelf]
    return s, off


def _emit(P, F, lab, cidx, box, off, s, R, p):
    c = cidx
    umin, umax, vmin, vmax = (box[c, k] for k in range(4))
    rot = (vmax - vmin) > (umax - umin)
    ox = (off[c, 0] + p).astype(np.float32)
    oy = (off[c, 1] + p).astype(np.float32)
    s, r = np.float32(s), np.float32(R)
    uv = np.zeros((len(F), 3, 2), np.float32)
    for k in range(3):
        u = P[F[:, k], AX_U[lab]]
        w = P[F[:, k], AX_V[lab]]
        lx = np.where(rot, vmax - w, u - umin)
        ly = np.where(rot, u - umin, w - vmin)
        uv[:, k, 0] = (lx * s + ox) / r
        uv[:, k, 1] = (ly * s + oy) / r
    return uv


def restate(P, F, R=1024, p=4, return_labels=False):
    """(faces_uvs [F, 3, 2] f32, chart [F] i32, stats) of the rules in include/volsurfs_hip.h."""
    P = np.asarray(P, np.float32)
    F = np.asarray(F, np.int64)
    nf = len(F)
    lab = _labels(P, F)
    f0, f1 = _join_pairs(F, lab)
    code = np.ones(nf, np.int64)
    splits = 0
    while True:
        act = (code[f0] == code[f1]) & (code[f0] != 0)
        root = _components(nf, f0[act], f1[act])
        _, cidx = np.unique(root, return_inverse=True)
        C = int(cidx.max()) + 1
        box = _boxes(P, F, lab, cidx, C)
        w, h = box[:, 1] - box[:, 0], box[:, 3] - box[:, 2]
        rot = h > w
        s, off = _pack(np.where(rot, h, w), np.where(rot, w, h), R, p)
        uv = _emit(P, F, lab, cidx, box, off, s, R, p)
        _, count, pf, pt = raster(uv, R)
        flag = np.zeros(C, bool)
        flag[cidx[pf[count.reshape(-1)[pt] >= 2]]] = True
        if not flag.any():
            st = {"charts": C, "split_rounds": splits, "scale": float(s), "covered": int((count > 0).sum())}
            out = (uv, cidx.astype(np.int32), st)
            return out + (lab,) if return_labels else out
        if splits + 1 >= MAX_ROUNDS:
            raise VolsurfsHipError("vsa_atlas: no end after MAX_ROUNDS rounds")
        sel = flag[cidx] & (code != 0)
        if not sel.any():
            raise VolsurfsHipError("vsa_atlas: a split that changes nothing")
        cap = sel & (code >= 1 << DEPTH_CAP)
        code[cap] = 0
        sel &= ~cap
        c = cidx[sel]
        along_u = (box[c, 1] - box[c, 0]) >= (box[c, 3] - box[c, 2])
        ax = np.where(along_u, AX_U[lab[sel]], AX_V[lab[sel]])
        lo = np.where(along_u, box[c, 0], box[c, 2]).astype(np.float64)
        hi = np.where(along_u, box[c, 1], box[c, 3]).astype(np.float64)
        cs = [P[F[sel, k], ax].astype(np.float64) for k in range(3)]
        side = ((cs[0] + cs[1]) + cs[2]) > 1.5 * (lo + hi)
        code[sel] = 2 * code[sel] + side
        splits += 1


# ------------------------------------------------------------------------------------------------ meshes

def _helix_ramp(turns=2.0, nt=96, nw=4, r0=0.2, r1=0.5, pitch=0.1):
    """A ribbon winding `turns` times around z, normals up: its +z projection overlaps itself."""
    t = np.linspace(0.0, 2 * np.pi * turns, nt + 1)
    r = np.linspace(r0, r1, nw + 1)
    T, Rr = np.meshgrid(t, r, indexing="ij")
    P = np.stack([Rr * np.cos(T), Rr * np.sin(T), pitch * T / (2 * np.pi)], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda i, j: i * (nw + 1) + j
    F = []
    for i in range(nt):
        for j in range(nw):
            F += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    F = np.array(F, np.int32)
    n = np.cross(P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]])
    if n[:, 2].mean() < 0:
        F = F[:, ::-1].copy()
    return P, F


def _torus():
    from tests.test_simplify import _torus_mesh
    return _torus_mesh()


def _open_mc():
    from tests.test_simplify import _open_mesh
    return _open_mesh()


MESHES = {
    "ico3": lambda: icosphere(3, 0.5),
    "torus": _torus,
    "open_mc": _open_mc,
    "helix": _helix_ramp,
}


def _check_atlas(P, F, uv, chart, lab, st, R, p):
    """The atlas validity rules of the issue on a restated or computed atlas."""
    P64 = np.asarray(P, np.float64)
    F = np.asarray(F, np.int64)
    assert uv.shape == (len(F), 3, 2) and (uv >= 0).all() and (uv <= 1).all()
    u = uv.astype(np.float64)
    area_uv = 0.5 * ((u[:, 1, 0] - u[:, 0, 0]) * (u[:, 2, 1] - u[:, 0, 1])
                     - (u[:, 1, 1] - u[:, 0, 1]) * (u[:, 2, 0] - u[:, 0, 0]))
    # exact projections have area >= 0; fp32 UVs move each corner by at most one rounding (2^-24)
    perim = np.linalg.norm(u[:, 1] - u[:, 0], axis=1) + np.linalg.norm(u[:, 2] - u[:, 1], axis=1) + \
        np.linalg.norm(u[:, 0] - u[:, 2], axis=1)
    assert (area_uv >= -4.0 * 2.0 ** -24 * perim).all(), "a face flips in UV"
    n = np.cross(P64[F[:, 1]] - P64[F[:, 0]], P64[F[:, 2]] - P64[F[:, 0]])
    nl = np.linalg.norm(n, axis=1)
    d = np.where(lab & 1, -1.0, 1.0) * n[np.arange(len(F)), lab >> 1]
    big = nl > 0
    assert (d[big] >= (0.5 - 1e-6) * nl[big]).all(), "a face keeps less than half its area in projection"
    # the UV scale agrees with the projection: uv area = projected area * (s / R)^2 on faces of reasonable size
    k = nl > 1e-3 * nl.max()
    ratio = area_uv[k] / (0.5 * d[k] * (st["scale"] / R) ** 2)
    assert np.allclose(ratio, 1.0, atol=1e-2), ratio.min()
    fid, count, _, _ = raster(uv, R)
    assert count.max() <= 1, "a texel is covered twice"
    assert int((count > 0).sum()) == st["covered"]
    cm = np.where(fid >= 0, np.asarray(chart)[np.maximum(fid, 0)], -1)
    g = 2 * p
    pad = np.full((R + 2 * g, R + 2 * g), -1, np.int64)
    pad[g:g + R, g:g + R] = cm
    for di in range(-g, g + 1):          # dilating each chart's coverage by 2p texels reaches no other chart
        for dj in range(-g, g + 1):
            sh = pad[g + dj:g + dj + R, g + di:g + di + R]
            assert not ((cm >= 0) & (sh >= 0) & (sh != cm)).any(), "two charts closer than 2p texels"
    assert st["charts"] == int(np.asarray(chart).max()) + 1


def _tri_overlap_fp64(uv, chart):
    """Pairs of faces of one chart whose UV triangles' interiors overlap (separating axes in fp64)."""
    u = uv.astype(np.float64)
    bad = 0
    for c in np.unique(chart):
        t = u[chart == c]                                  # [n, 3, 2]
        e = np.roll(t, -1, axis=1) - t
        axes = np.stack([-e[:, :, 1], e[:, :, 0]], -1)     # [n, 3, 2] edge normals
        proj_a = np.einsum("nkd,mjd->nmkj", axes, t)       # axes of n onto triangles m
        proj_b = np.einsum("nkd,njd->nkj", axes, t)        # axes of n onto n
        lo_a, hi_a = proj_a.min(3), proj_a.max(3)
        lo_b, hi_b = proj_b.min(2)[:, None, :], proj_b.max(2)[:, None, :]
        sep1 = ((np.minimum(hi_a, hi_b) - np.maximum(lo_a, lo_b)) <= 1e-12).any(2)   # [n, m] by n's axes
        ov = ~(sep1 | sep1.T)
        np.fill_diagonal(ov, False)
        bad += int(ov.sum()) // 2
    return bad


# ------------------------------------------------------------------------------------------------ no GPU needed

@pytest.mark.parametrize("name", list(MESHES))
def test_restatement_is_a_valid_atlas(name):
    P, F = MESHES[name]()
    R, p = 512, 4
    uv, chart, st, lab = restate(P, F, R, p, return_labels=True)
    _check_atlas(P, F, uv, chart, lab, st, R, p)
    print(f"{name}: F {len(F)}, charts {st['charts']}, split rounds {st['split_rounds']}, "
          f"utilization {st['covered'] / R ** 2:.3f}")
    if name == "helix":
        assert st["split_rounds"] >= 1, "the helical ramp must take the split path"
    if name in ("ico3", "torus"):
        assert st["split_rounds"] == 0


@pytest.mark.parametrize("name", ["ico3", "torus"])
def test_no_interior_overlap_fp64(name):
    P, F = MESHES[name]()
    uv, chart, _ = restate(P, F, 256, 2)
    assert _tri_overlap_fp64(uv, chart) == 0


def _soup(n):
    """n disjoint triangles: n single-face charts."""
    rng = np.random.default_rng(0)
    base = rng.uniform(-1, 1, (n, 1, 3)).astype(np.float32)
    tri = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0]], np.float32)
    return (base + tri).reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def test_pack_error_names_charts_and_resolution():
    P, F = _soup(500)
    with pytest.raises(VolsurfsHipError, match=r"500 charts do not fit a 32 x 32 atlas .* is 184$"):
        restate(P, F, 32, 4)
    assert atlas.min_resolution(500, 4) == 184
    restate(P, F, 184, 4)                      # fits there


# ------------------------------------------------------------------------------------------------------- GPU

def _gpu(P, F, R, p):
    from volsurfs_amd.mesh import TensorMesh
    m = TensorMesh(torch.from_numpy(np.asarray(P, np.float32)), torch.from_numpy(np.asarray(F, np.int32)), None,
                   device="cuda")
    return atlas.compute_atlas(m, R, p, return_stats=True, return_charts=True)


def _simplified(kind):
    from tests.test_isosurface import _h, _lobed_fn
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.simplify import simplify_mesh
    n = 96
    if kind == "sphere":
        fn = lambda q: torch.linalg.vector_norm(q, dim=-1)[:, None] - 0.5
    else:
        fn = _lobed_fn
    mc = iso.marching_cubes(iso.sample_grid(fn, n), [0.0], [-1.0] * 3, [_h(n)] * 3)[0]
    m = simplify_mesh(mc, 0.1)
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy()


GPU_MESHES = dict(MESHES, sphere_simplified=lambda: _simplified("sphere"),
                  lobed_simplified=lambda: _simplified("lobed"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_MESHES))
@pytest.mark.parametrize("R,p", [(256, 2), (1024, 4)])
def test_exact_vs_restatement(name, R, p):
    P, F = GPU_MESHES[name]()
    uv, chart, st, lab = restate(P, F, R, p, return_labels=True)
    m, gst, gchart = _gpu(P, F, R, p)
    again, _, _ = _gpu(P, F, R, p)
    assert torch.equal(m.faces_uvs.cpu().view(torch.int32), torch.from_numpy(uv).view(torch.int32))
    assert torch.equal(gchart.cpu(), torch.from_numpy(chart))
    assert {k: gst[k] for k in st} == st
    assert torch.equal(m.faces_uvs, again.faces_uvs)
    assert m.has_uvs and np.array_equal(m.faces.cpu().numpy(), np.asarray(F, np.int32))
    assert torch.equal(m.vertices.cpu(), torch.from_numpy(np.asarray(P, np.float32)))
    _check_atlas(P, F, uv, chart, lab, st, R, p)
    print(f"{name} R={R} p={p}: F {len(F)}, charts {st['charts']}, split rounds {st['split_rounds']}, "
          f"utilization {gst['utilization']:.3f}")


@pytest.mark.gpu
def test_large_shell_is_deterministic_and_exact():
    """A lobed n = 512 shell simplified to 0.1 (about 60k faces in about a hundred charts, so deep union-find trees,
    and a split round): the same bits on every call, and the restatement's.  test_scale_n1000_five_levels checks the
    same on noisy shells of thousands of charts and up to 17 split rounds, call against call."""
    from tests.test_isosurface import _h, _lobed_fn
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.simplify import simplify_mesh
    n = 512
    mc = iso.marching_cubes(iso.sample_grid(_lobed_fn, n), [0.0], [-1.0] * 3, [_h(n)] * 3)[0]
    m = simplify_mesh(mc, 0.1)
    del mc
    runs = [atlas.compute_atlas(m, 1024, 4, return_stats=True, return_charts=True) for _ in range(3)]
    for a, st, ch in runs[1:]:
        assert torch.equal(a.faces_uvs.view(torch.int32), runs[0][0].faces_uvs.view(torch.int32))
        assert torch.equal(ch, runs[0][2]) and st == runs[0][1]
    P, F = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
    uv, chart, st = restate(P, F, 1024, 4)
    a, gst, gchart = runs[0]
    print(f"lobed n=512 @0.1: F {len(F)}, charts {st['charts']}, split rounds {st['split_rounds']}, "
          f"utilization {gst['utilization']:.3f}")
    assert len(F) > 50000 and st["split_rounds"] >= 1
    assert torch.equal(a.faces_uvs.cpu().view(torch.int32), torch.from_numpy(uv).view(torch.int32))
    assert torch.equal(gchart.cpu(), torch.from_numpy(chart)) and {k: gst[k] for k in st} == st


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ico3", "helix", "lobed_simplified"])
def test_rasterize_vs_restatement(name):
    P, F = GPU_MESHES[name]()
    R = 512
    uv, _, _ = restate(P, F, R, 4)
    # the atlas itself, and a perturbed copy whose faces overlap and flip
    rng = np.random.default_rng(3)
    wild = np.clip(uv + rng.normal(0, 0.02, uv.shape).astype(np.float32), 0, 1).astype(np.float32)
    for q in (uv, wild):
        fid, count, _, _ = raster(q, R)
        gid, gcount = atlas.rasterize_atlas(torch.from_numpy(q).cuda(), R)
        assert torch.equal(gid.cpu(), torch.from_numpy(fid)) and torch.equal(gcount.cpu(), torch.from_numpy(count))
    assert count.max() >= 2


@pytest.mark.gpu
def test_workspace_is_linear():
    # a GPU test: the query includes rocPRIM's temporary-storage size, and rocPRIM's size queries need a device
    a, b = atlas.workspace_bytes(1000, 2000, 256), atlas.workspace_bytes(100000, 200000, 256)
    r = 4 * 256 * 256
    assert a > r and b > r
    assert (b - r) < 101 * (a - r)
    assert atlas.workspace_bytes(1000, 2000, 1024) - a == 4 * (1024 ** 2 - 256 ** 2)


@pytest.mark.gpu
def test_pack_error_on_gpu():
    P, F = _soup(500)
    with pytest.raises(VolsurfsHipError, match=r"500 charts do not fit a 32 x 32 atlas .* is 184$"):
        _gpu(P, F, 32, 4)


@pytest.mark.gpu
def test_empty_and_invalid_inputs():
    from volsurfs_amd.mesh import TensorMesh
    V, F = icosphere(1, 0.5)
    good = TensorMesh(V, F, None, device="cuda")
    for R, p in ((4, 0), (20000, 4), (64, 32), (64, -1)):
        with pytest.raises(ValueError):
            atlas.compute_atlas(good, R, p)
    with pytest.raises(ValueError):
        atlas.compute_atlas(TensorMesh(V, F, None, device="cpu"), 256, 4)
    bad = V.copy()
    bad[3, 1] = np.nan
    with pytest.raises(VolsurfsHipError):
        atlas.compute_atlas(TensorMesh(bad, F, None, device="cuda"), 256, 4)
    for v in (len(V), -1):
        f = F.copy()
        f[5, 2] = v
        with pytest.raises(VolsurfsHipError):
            atlas.compute_atlas(TensorMesh(V, f, None, device="cuda"), 256, 4)
    f = F.copy()
    f[5, 2] = f[5, 1]
    with pytest.raises(VolsurfsHipError):
        atlas.compute_atlas(TensorMesh(V, f, None, device="cuda"), 256, 4)
    empty, st = atlas.compute_atlas(TensorMesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None,
                                               device="cuda"), 256, 4, return_stats=True)
    assert empty.faces_uvs.shape == (0, 3, 2) and empty.has_uvs and st["charts"] == 0
    with pytest.raises(ValueError):
        atlas.rasterize_atlas(torch.zeros(4, 3, 2), 64)


@pytest.mark.gpu
def test_end_to_end_files_and_neural_texture_training(tmp_path):
    from tests.test_isosurface import _lobed_fn as lobed
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.camera import pinhole_rays
    from volsurfs_amd.mesh import load_obj
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.simplify import simplify_meshes
    from volsurfs_amd.trainer import train_step
    meshes, levels = iso.extract_level_sets(lobed, 96, 5, delta_surfs=0.01)
    raw, simp, uvd = (str(tmp_path / d) for d in ("meshes", "meshes_simplified", "meshes_simplified_uvs"))
    iso.save_level_sets(meshes, levels, raw)
    simplify_meshes(raw, simp, 0.1)
    paths = atlas.compute_meshes_atlas(simp, uvd, 1024, 4)
    stems = [f"{round(lv, 4)}" for lv in levels]
    assert [os.path.basename(x) for x in paths] == [s + ".obj" for s in stems]
    for s, path in zip(stems, paths):
        assert os.path.getsize(os.path.join(uvd, "atlas", s + ".png")) > 0
        from volsurfs_amd.mesh import load_ply
        want = atlas.compute_atlas(load_ply(os.path.join(simp, s + ".ply")), 1024, 4)
        got = load_obj(path)
        assert got.has_uvs and torch.equal(got.faces_uvs, want.faces_uvs) and torch.equal(got.faces, want.faces)
        assert torch.equal(got.vertices, want.vertices)
    m = VolSurfs.from_meshes_path(uvd, str(tmp_path / "ckpt"), using_neural_textures=True, max_rays=4096,
                                  textures_res=(256, 128, 64, 32), nr_warmup_iters=2, lr=2e-3)
    o, d = pinhole_rays(48, 48, focal=60.0, cam_pos=(0.0, 0.0, -1.6))
    gt = torch.rand(48 * 48, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) * 0.2 + 0.4
    loss = m(o, d, gt, iter_nr=0, is_first_iter=True)[0]["loss"]
    loss.backward()
    assert torch.isfinite(loss)
    grads = [q.grad for q in m.parameters() if q.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    m.zero_grad(set_to_none=True)
    m.init_optim()
    m.grad_scale = float(48 * 48)
    losses = []
    for it in range(12):
        l, _ = train_step(m, o, d, gt, None, iter_nr=it, is_first_iter=(it == 0), nr_rays=48 * 48,
                          target_nr_of_training_samples=100000)
        losses.append(l["loss"])
    print("neural-texture training on atlased shells, loss:", [round(x, 5) for x in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[1]


# measured on MI355X: 0.207 s for the five shells, lowest utilization 0.247; the time bound is 2x, the
# utilization floor half the measured value
SCALE_SECONDS_MEASURED = 0.207
SCALE_UTILIZATION_MEASURED = 0.247


@pytest.mark.gpu
def test_scale_n1000_five_levels():
    import time
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.simplify import simplify_mesh
    from tests.test_simplify import _lobed_fn
    meshes, _ = iso.extract_level_sets(_lobed_fn, 1000, 5, delta_surfs=0.0025)
    simp = [simplify_mesh(m, 0.025) for m in meshes]
    del meshes
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [atlas.compute_atlas(m, 1024, 4, return_stats=True) for m in simp]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    util = [st["utilization"] for _, st in out]
    print(f"n=1000 K=5 lobed_noisy @0.025: {sum(m.faces.shape[0] for m in simp)} faces atlased in {dt:.3f} s; "
          f"charts {[st['charts'] for _, st in out]}, split rounds {[st['split_rounds'] for _, st in out]}, "
          f"utilization {[round(u, 3) for u in util]}")
    again = [atlas.compute_atlas(m, 1024, 4, return_stats=True) for m in simp]
    for (a, st), (b, st2) in zip(out, again):
        assert torch.equal(a.faces_uvs.view(torch.int32), b.faces_uvs.view(torch.int32)) and st == st2
    for m, (a, _) in zip(simp, out):
        uv = a.faces_uvs
        assert bool(((uv >= 0) & (uv <= 1)).all())
        _, count = atlas.rasterize_atlas(a, 1024)
        assert int(count.max()) <= 1
    assert dt <= 2 * SCALE_SECONDS_MEASURED
    assert min(util) >= 0.5 * SCALE_UTILIZATION_MEASURED
