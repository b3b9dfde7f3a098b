"""Quadric edge-collapse simplification on the GPU (csrc/simplify.hip, volsurfs_amd/simplify.py).

`restate` below is the numpy restatement of the rules in include/volsurfs_hip.h: the same fp64 operations in the same
order, the same candidate rules, keys, winners, target rule and output order, so the kernels are held to it bit for
bit.  Topology (closed 2-manifolds, Euler characteristic, boundary loops, orientation), the target rule, sphere
geometry, the files, the path into RayTracer and VolSurfs and an n = 1000 run are checked on top."""
import os

import numpy as np
import pytest
import torch

from tests.test_isosurface import _h, _noisy_closed, _signed_volume, _sphere, _topology, restate as mc_restate
from volsurfs_amd import simplify as smp
from volsurfs_amd.mesh import icosphere

DET_REL, BOUNDARY_WEIGHT = 1e-10, 10.0
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------- restatement

def _plane(w, u0, u1, u2, d):
    p = (u0, u1, u2, d)
    return np.stack([w * (p[i] * p[j]) for i in range(4) for j in range(i, 4)], -1)


def _cross(e1, e2):
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                     e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)


def _normal(p0, p1, p2):
    return _cross(p1 - p0, p2 - p0)


def _unit_plane(m, through, w):
    with np.errstate(all="ignore"):
        ln = np.sqrt(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1] + m[:, 2] * m[:, 2])
        u = m / ln[:, None]
        d = -(u[:, 0] * through[:, 0] + u[:, 1] * through[:, 1] + u[:, 2] * through[:, 2])
        q = _plane(w(ln), u[:, 0], u[:, 1], u[:, 2], d)
    q[~(ln > 0)] = 0.0
    return q


def _init_quadrics(P, F):
    V = len(P)
    P64 = P.astype(np.float64)
    p = [P64[F[:, c]] for c in range(3)]
    n = _normal(*p)
    qf = _unit_plane(n, p[0], lambda ln: 0.5 * ln)
    a, b = F, np.roll(F, -1, axis=1)
    key = (np.minimum(a, b) * V + np.maximum(a, b)).reshape(-1)
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    bnd = (cnt[inv] == 1).reshape(-1, 3)
    # records in (face, sub) order: Q_f to its corners, then the penalty of boundary edge c to its two endpoints
    vid, val, order = [], [], []
    nf = len(F)
    for c in range(3):
        vid.append(F[:, c])
        val.append(qf)
        order.append(np.arange(nf) * 8)
    for c in range(3):
        c1 = (c + 1) % 3
        pi, pj = p[c], p[c1]
        e = pj - pi
        qb = _unit_plane(_cross(e, n), pi,
                         lambda ln, e=e: BOUNDARY_WEIGHT * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]))
        sel = bnd[:, c]
        for corner in (c, c1):
            vid.append(F[sel, corner])
            val.append(qb[sel])
            order.append(np.nonzero(sel)[0] * 8 + 1 + c)
    vid, val, order = np.concatenate(vid), np.concatenate(val), np.concatenate(order)
    o = np.argsort(order, kind="stable")
    Q = np.zeros((V, 10))
    np.add.at(Q, vid[o], val[o])
    return Q


def _eval(q, p):
    x, y, z = (p[:, c].astype(np.float64) for c in range(3))
    t0 = q[:, 0] * x + q[:, 1] * y + q[:, 2] * z + q[:, 3]
    t1 = q[:, 1] * x + q[:, 4] * y + q[:, 5] * z + q[:, 6]
    t2 = q[:, 2] * x + q[:, 5] * y + q[:, 7] * z + q[:, 8]
    t3 = q[:, 3] * x + q[:, 6] * y + q[:, 8] * z + q[:, 9]
    return t0 * x + t1 * y + t2 * z + t3


def _place(P, Q, ea, eb, bnd):
    q = Q[ea] + Q[eb]
    pa, pb = P[ea], P[eb]
    A, B, C, D, E, Fq = q[:, 0], q[:, 1], q[:, 2], q[:, 4], q[:, 5], q[:, 7]
    r0, r1, r2 = -q[:, 3], -q[:, 6], -q[:, 8]
    c00, c01, c02 = D * Fq - E * E, C * E - B * Fq, B * E - C * D
    c11, c12, c22 = A * Fq - C * C, B * C - A * E, A * D - B * B
    det = A * c00 + B * c01 + C * c02
    tr = A + D + Fq
    with np.errstate(all="ignore"):
        ps = np.stack([(c00 * r0 + c01 * r1 + c02 * r2) / det, (c01 * r0 + c11 * r1 + c12 * r2) / det,
                       (c02 * r0 + c12 * r1 + c22 * r2) / det], 1).astype(np.float32)
        pm = ((pa.astype(np.float64) + pb.astype(np.float64)) * 0.5).astype(np.float32)
        ca, cb, cm, cs = _eval(q, pa), _eval(q, pb), _eval(q, pm), _eval(q, ps)
    best, p = ca.copy(), pa.copy()
    t = cb < best
    best[t], p[t] = cb[t], pb[t]
    t = cm < best
    best[t], p[t] = cm[t], pm[t]
    solve = det > DET_REL * (tr * tr * tr)
    best[solve], p[solve] = cs[solve], ps[solve]
    ba, bb = bnd[ea], bnd[eb]
    one = ba != bb
    pe = np.where(ba[:, None], pa, pb)
    with np.errstate(all="ignore"):
        ce = _eval(q, pe)
    best[one], p[one] = ce[one], pe[one]
    return p, best


def _ranges(starts, lengths):
    """Concatenated aranges [s, s + l) and the index of the range each element came from."""
    rid = np.repeat(np.arange(len(starts)), lengths)
    off = np.cumsum(lengths) - lengths
    return np.repeat(starts, lengths) + np.arange(lengths.sum()) - np.repeat(off, lengths), rid


def _ring_pairs(F, V, verts):
    """(edge index, face) for every face at verts[e], e in order."""
    flat = F.reshape(-1)
    order = np.argsort(flat, kind="stable")
    vs = flat[order]
    start = np.searchsorted(vs, np.arange(V))
    end = np.searchsorted(vs, np.arange(V), side="right")
    idx, eid = _ranges(start[verts], end[verts] - start[verts])
    return eid, order[idx] // 3


def _candidates(P, F, ea, eb, cnt, bnd, frz, p, cost):
    V, E = len(P), len(ea)
    ok = ~(frz[ea] | frz[eb]) & ~((cnt > 1) & bnd[ea] & bnd[eb])
    ok &= np.isfinite(p).all(1) & ~np.isnan(cost)
    # link condition
    nb = np.concatenate([F[:, [i, j]] for i in range(3) for j in range(3) if i != j], 0)
    nkeys = np.unique(nb[:, 0] * V + nb[:, 1])
    s = np.searchsorted(nkeys, ea * V)
    t = np.searchsorted(nkeys, ea * V + V)
    idx, eid = _ranges(s, t - s)
    x = nkeys[idx] % V
    member = np.isin(eb[eid] * V + x, nkeys) & (x != eb[eid])
    ok &= np.bincount(eid[member], minlength=E) == cnt
    # flips and duplicated faces
    P64 = P.astype(np.float64)
    tri = []
    for side, (m, other) in enumerate(((ea, eb), (eb, ea))):
        eid, f = _ring_pairs(F, V, m)
        c = F[f]
        keep = ~(c == other[eid][:, None]).any(1)
        eid, c = eid[keep], c[keep]
        po = [P64[c[:, k]] for k in range(3)]
        pn = [np.where((c[:, k] == m[eid])[:, None], p[eid].astype(np.float64), po[k]) for k in range(3)]
        nbf, naf = _normal(*po), _normal(*pn)
        dot = nbf[:, 0] * naf[:, 0] + nbf[:, 1] * naf[:, 1] + nbf[:, 2] * naf[:, 2]
        bad = (nbf != 0).any(1) & ~(dot > 0)
        ok &= np.bincount(eid[bad], minlength=E) == 0
        mapped = np.where(c == eb[eid][:, None], ea[eid][:, None], c)
        tri.append(np.unique(np.concatenate([eid[:, None], np.sort(mapped, 1)], 1), axis=0))
    rows, counts = np.unique(np.concatenate(tri, 0), axis=0, return_counts=True)
    ok &= np.bincount(rows[counts > 1, 0], minlength=E) == 0
    return ok


def _key(cost, ok):
    c = np.maximum(cost, 0.0)
    with np.errstate(all="ignore"):
        cf = c.astype(np.float32)
    bits = cf.view(np.uint32).astype(np.uint64) + (cf.astype(np.float64) < c).astype(np.uint64)
    key = (bits << np.uint64(32)) | np.arange(len(c), dtype=np.uint64)
    return np.where(ok, key, NONE)


def restate(P, F, ratio):
    """(V_out [V, 3] f32, F_out [F, 3] i32, stats) of the rules in include/volsurfs_hip.h."""
    P = np.array(P, np.float32)
    F = np.array(F, np.int64)
    V = len(P)
    target = smp.target_faces(len(F), ratio)
    Q = _init_quadrics(P, F)
    rounds = collapses = 0
    stalled = False
    while len(F) > target:
        a, b = F, np.roll(F, -1, axis=1)
        uk, cnt = np.unique((np.minimum(a, b) * V + np.maximum(a, b)).reshape(-1), return_counts=True)
        ea, eb = uk // V, uk % V
        bnd, frz = np.zeros(V, bool), np.zeros(V, bool)
        bnd[ea[cnt == 1]] = bnd[eb[cnt == 1]] = True
        frz[ea[cnt > 2]] = frz[eb[cnt > 2]] = True
        p, cost = _place(P, Q, ea, eb, bnd)
        key = _key(cost, _candidates(P, F, ea, eb, cnt, bnd, frz, p, cost))
        m1 = np.full(V, NONE)
        np.minimum.at(m1, ea, key)
        np.minimum.at(m1, eb, key)
        fm = m1[F].min(1)
        m2 = np.full(V, NONE)
        for c in range(3):
            np.minimum.at(m2, F[:, c], fm)
        win = np.nonzero((key != NONE) & (key == m2[ea]) & (key == m2[eb]))[0]
        if len(win) == 0:
            stalled = True
            break
        need = len(F) - target
        if cnt[win].sum() > need:
            win = win[np.argsort(key[win], kind="stable")]
            pre = np.cumsum(cnt[win]) - cnt[win]
            win = win[pre < need]
        wa, wb = ea[win], eb[win]
        Q[wa] = Q[wa] + Q[wb]
        P[wa] = p[win]
        remap = np.arange(V)
        remap[wb] = wa
        F = remap[F]
        F = F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 2] != F[:, 0])]
        rounds += 1
        collapses += len(win)
    used = np.zeros(V, bool)
    used[F.reshape(-1)] = True
    new = np.cumsum(used) - 1
    st = {"rounds": rounds, "collapses": collapses, "stalled": stalled, "faces_out": len(F), "target": target}
    return P[used], new[F].astype(np.int32), st


# ------------------------------------------------------------------------------------------------ meshes

def _torus_mesh(nu=40, nv=24, R=0.5, r=0.2):
    u, v = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    th, ph = 2 * np.pi * u / nu, 2 * np.pi * v / nv
    P = np.stack([(R + r * np.cos(ph)) * np.cos(th), (R + r * np.cos(ph)) * np.sin(th), r * np.sin(ph)], -1)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    F = []
    for i in range(nu):
        for j in range(nv):
            F += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return P.reshape(-1, 3).astype(np.float32), np.array(F, np.int32)


def _mc_mesh(f, n):
    return mc_restate(f, [0.0], [-1.0] * 3, [_h(n)] * 3)[0]


def _open_mesh():
    """A marching-cubes sphere cut by a box: the faces wholly inside |x| <= 0.3 (filter_inside's rule)."""
    n = 40
    V, F = _mc_mesh(_sphere((n, n, n), 0.5), n)
    keep = (np.abs(V[:, 0]) <= np.float32(0.3))[F].all(1)
    F = F[keep]
    used = np.zeros(len(V), bool)
    used[F.reshape(-1)] = True
    return V[used], (np.cumsum(used) - 1)[F].astype(np.int32)


def _degenerate_mesh():
    """Grid values exactly at the level: zero-area faces; the largest closed piece is kept whole."""
    n = 24
    X = np.linspace(-1, 1, n, dtype=np.float32)
    X, Y, Z = np.meshgrid(X, X, X, indexing="ij")
    f = np.round((np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.6) * 8).astype(np.float32) / 8
    return _mc_mesh(f, n)


MESHES = {
    "ico2": lambda: icosphere(2, 0.5),
    "ico3": lambda: icosphere(3, 0.5),
    "ico4": lambda: icosphere(4, 0.5),
    "torus": _torus_mesh,
    "noisy_mc": lambda: _mc_mesh(_noisy_closed(20, seed=2), 20),
    "open_mc": _open_mesh,
    "degenerate_mc": _degenerate_mesh,
}
CLOSED_EULER = {"ico2": 2, "ico3": 2, "ico4": 2, "torus": 0}


def _boundary_loops(F):
    """Number of boundary loops (connected components of the boundary edges)."""
    F = np.asarray(F, np.int64)
    d = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], 0)
    k = np.sort(d, 1)
    u, c = np.unique(k, axis=0, return_counts=True)
    be = u[c == 1]
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in be:
        parent[find(x)] = find(y)
    return len({find(x) for x in be.reshape(-1)})


def _check_valid(V, F, closed_euler=None, loops=None):
    F = np.asarray(F, np.int64)
    assert ((F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 2] != F[:, 0])).all(), "repeated index in a face"
    assert len(F) == 0 or np.array_equal(np.unique(F), np.arange(len(V))), "unreferenced vertices"
    if closed_euler is not None:
        assert _topology(V, F) == closed_euler
        assert _signed_volume(V, F) > 0
    if loops is not None:
        assert _boundary_loops(F) == loops


# ------------------------------------------------------------------------------------------------ no GPU needed

def test_target_rule_is_pymeshlabs():
    assert smp.target_faces(1000, 0.025) == 25 and smp.target_faces(999, 0.1) == 99 and smp.target_faces(4, 0.01) == 0


@pytest.mark.parametrize("name", ["ico3", "torus", "open_mc", "degenerate_mc"])
def test_restatement_topology_and_target(name):
    V0, F0 = MESHES[name]()
    loops = _boundary_loops(F0)
    for ratio in (0.1, 0.025):
        V, F, st = restate(V0, F0, ratio)
        _check_valid(V, F, CLOSED_EULER.get(name), loops if name == "open_mc" else None)
        if not st["stalled"]:
            assert st["target"] - 2 <= len(F) <= st["target"]


def test_restatement_tetrahedron_stalls():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    v, f, st = restate(V, F, 0.01)
    assert st["stalled"] and st["collapses"] == 0 and np.array_equal(f, F) and np.array_equal(v, V)


@pytest.mark.gpu
def test_workspace_is_linear():
    # a GPU test: the query includes rocPRIM's temporary-storage size, and rocPRIM's size queries need a device
    a, b = smp.workspace_bytes(1000, 2000), smp.workspace_bytes(100000, 200000)
    assert a > 0
    assert b < 101 * a
    assert smp.workspace_bytes(1_250_000, 2_500_000) < 1 << 30


# ------------------------------------------------------------------------------------------------------- GPU

def _gpu(V, F, ratio, **kw):
    from volsurfs_amd.mesh import TensorMesh
    m = TensorMesh(torch.from_numpy(np.asarray(V, np.float32)), torch.from_numpy(np.asarray(F, np.int32)), None,
                   device="cuda")
    return smp.simplify_mesh(m, ratio, return_stats=True, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MESHES))
@pytest.mark.parametrize("ratio", [0.5, 0.1, 0.025])
def test_exact_vs_restatement(name, ratio):
    V0, F0 = MESHES[name]()
    V, F, st = restate(V0, F0, ratio)
    got, gst = _gpu(V0, F0, ratio)
    again, _ = _gpu(V0, F0, ratio)
    assert torch.equal(got.faces.cpu(), torch.from_numpy(F))
    assert torch.equal(got.vertices.cpu().view(torch.int32), torch.from_numpy(V).view(torch.int32))
    assert torch.equal(got.faces, again.faces) and torch.equal(got.vertices, again.vertices)
    assert {k: gst[k] for k in st} == st and gst["faces_in"] == len(F0)
    assert not got.has_uvs and got.faces_uvs.shape == (len(F), 3, 2)
    _check_valid(V, F, CLOSED_EULER.get(name), _boundary_loops(F0) if name == "open_mc" else None)
    if not st["stalled"]:
        assert st["target"] - 2 <= len(F) <= st["target"]


@pytest.mark.gpu
def test_tetrahedron_stalls_and_stays_valid():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    m, st = _gpu(V, F, 0.01)
    assert st["stalled"] and st["faces_out"] == 4 and st["collapses"] == 0
    assert np.array_equal(m.faces.cpu().numpy(), F) and np.array_equal(m.vertices.cpu().numpy(), V)


# measured on MI355X: vertices 0.0872 h, face centroids 0.1126 h; the bound is 2x the larger
SPHERE_ERR_MEASURED_H = 0.1126


@pytest.mark.gpu
def test_geometry_sphere_n256():
    from volsurfs_amd import isosurface as iso
    n, r = 256, 0.5
    h = _h(n)
    grid = iso.sample_grid(lambda p: torch.linalg.vector_norm(p, dim=-1)[:, None] - r, n)
    mc = iso.marching_cubes(grid, [0.0], [-1.0] * 3, [h] * 3)[0]
    m, st = smp.simplify_mesh(mc, 0.025, return_stats=True)
    assert not st["stalled"] and st["target"] - 2 <= st["faces_out"] <= st["target"]
    V = m.vertices.cpu().numpy().astype(np.float64)
    F = m.faces.cpu().numpy().astype(np.int64)
    _check_valid(V, F, 2)
    err_v = np.abs(np.linalg.norm(V, axis=1) - r).max()
    cen = V[F].mean(1)
    err_c = np.abs(np.linalg.norm(cen, axis=1) - r).max()
    print(f"sphere n=256 ratio 0.025: F {st['faces_in']} -> {st['faces_out']} in {st['rounds']} rounds, "
          f"max radial error vertices {err_v / h:.4f} h, centroids {err_c / h:.4f} h")
    bound = 2 * SPHERE_ERR_MEASURED_H * h
    assert err_v <= bound and err_c <= bound
    n_f = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    assert ((n_f * cen).sum(1) > 0).all(), "a face normal points inward"


@pytest.mark.gpu
def test_empty_and_invalid_inputs():
    from volsurfs_amd._lib import VolsurfsHipError
    from volsurfs_amd.mesh import TensorMesh
    V, F = icosphere(1, 0.5)
    good = TensorMesh(V, F, None, device="cuda")
    for r in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            smp.simplify_mesh(good, r)
    with pytest.raises(ValueError):
        smp.simplify_mesh(TensorMesh(V, F, None, device="cpu"), 0.5)
    bad = V.copy()
    bad[3, 1] = np.nan
    with pytest.raises(VolsurfsHipError):
        smp.simplify_mesh(TensorMesh(bad, F, None, device="cuda"), 0.5)
    f = F.copy()
    f[5, 2] = len(V)
    with pytest.raises(VolsurfsHipError):
        smp.simplify_mesh(TensorMesh(V, f, None, device="cuda"), 0.5)
    f = F.copy()
    f[5, 2] = -1
    with pytest.raises(VolsurfsHipError):
        smp.simplify_mesh(TensorMesh(V, f, None, device="cuda"), 0.5)
    empty = smp.simplify_mesh(TensorMesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None,
                                         device="cuda"), 0.5)
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)
    same, st = smp.simplify_mesh(good, 1.0, return_stats=True)
    assert st["rounds"] == 0 and torch.equal(same.faces, good.faces) and torch.equal(same.vertices, good.vertices)


def _lobed_fn(pts):
    rad = torch.linalg.vector_norm(pts, dim=-1)
    phi = torch.atan2(pts[:, 1], pts[:, 0])
    f = rad - 0.45 * (1.0 + 0.25 * torch.sin(4.0 * phi) * torch.cos(3.0 * pts[:, 2]))
    noise = 0.01 * torch.sin(97.0 * pts[:, 0]) * torch.sin(89.0 * pts[:, 1]) * torch.sin(83.0 * pts[:, 2])
    return (f + noise)[:, None]


@pytest.mark.gpu
def test_end_to_end_files_raytracer_and_volsurfs(tmp_path):
    from tests.bvh_builder_cases import assert_same_hits as _assert_same_hits
    from tests.test_isosurface import _lobed_fn as lobed
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.camera import pinhole_rays
    from volsurfs_amd.mesh import load_meshes_indexed_from_path
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.raytrace import RayTracer
    meshes, levels = iso.extract_level_sets(lobed, 96, 5, delta_surfs=0.01)
    raw = str(tmp_path / "meshes")
    out = str(tmp_path / "meshes_simplified")
    iso.save_level_sets(meshes, levels, raw)
    paths = smp.simplify_meshes(raw, out, 0.1)
    assert sorted(os.listdir(out)) == sorted(os.listdir(raw)) and len(paths) == 5
    assert [os.path.basename(p) for p in paths] == [f"{round(lv, 4)}.ply" for lv in levels]
    loaded = load_meshes_indexed_from_path(None, out)
    for m, l in zip(meshes, loaded):                        # inner -> outer
        assert not l.has_uvs
        want = smp.simplify_mesh(m, 0.1)
        assert torch.equal(want.faces, l.faces) and torch.equal(want.vertices, l.vertices)
        assert l.faces.shape[0] <= int(m.faces.shape[0] * 0.1)
    o, d = pinhole_rays(96, 96, focal=120.0, cam_pos=(0.0, 0.0, -1.6))
    host, ploc = RayTracer(loaded), RayTracer(loaded, builder="ploc")
    ref = [x.clone() for x in host.trace_all(o, d)]
    assert (ref[1] >= 0).sum().item() > 1000
    _assert_same_hits(ploc.trace_all(o, d), ref, ploc, host)
    # sphere shells simplified: hit t within h of the analytic ray-sphere t
    n, radii = 128, [0.3, 0.35, 0.4]
    sph = iso.marching_cubes(iso.sample_grid(lambda p: torch.linalg.vector_norm(p, dim=-1)[:, None], n), radii,
                             [-1.0] * 3, [_h(n)] * 3)
    sph = [smp.simplify_mesh(m, 0.1) for m in sph]
    t, slot, _ = RayTracer(sph, builder="ploc").trace_all(o, d)
    oo, dd = o.double(), torch.nn.functional.normalize(d.double(), dim=-1)
    scale = torch.linalg.vector_norm(d.double(), dim=-1)
    for k, r in enumerate(radii):
        b = (oo * dd).sum(-1)
        disc = b * b - ((oo * oo).sum(-1) - r * r)
        hit = (slot[k] >= 0) & (disc > (4 * _h(n)) ** 2)
        t_ref = (-b - disc.clamp(min=0).sqrt()) / scale
        assert hit.sum() > 500
        assert ((t[k].double() - t_ref)[hit].abs() * scale[hit]).max() <= _h(n)
    m = VolSurfs.from_meshes_path(out, str(tmp_path / "ckpt"), using_neural_textures=False, max_rays=4096,
                                  rgb_mlp_layers_dims=(64, 32), bb_sides=1.0, sh_degree=3)
    o2, d2 = pinhole_rays(32, 32, focal=40.0, cam_pos=(0.0, 0.0, -1.6))
    gt = torch.rand(o2.shape[0], 3, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    loss = m(o2, d2, gt, iter_nr=0, is_first_iter=True)[0]["loss"]
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)


@pytest.mark.gpu
def test_scale_n1000_five_levels():
    import time
    from volsurfs_amd import isosurface as iso
    meshes, levels = iso.extract_level_sets(_lobed_fn, 1000, 5, delta_surfs=0.0025)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    total_in = total_out = 0
    for m in meshes:
        nv, nf = m.vertices.shape[0], m.faces.shape[0]
        assert smp.workspace_bytes(nv, nf) < 1 << 30
        s, st = smp.simplify_mesh(m, 0.025, return_stats=True)
        assert not st["stalled"] and st["target"] - 2 <= st["faces_out"] <= st["target"]
        total_in += nf
        total_out += st["faces_out"]
        _check_valid(s.vertices.cpu().numpy(), s.faces.cpu().numpy())
    torch.cuda.synchronize()
    print(f"n=1000 K=5 lobed_noisy: {total_in} -> {total_out} faces in {time.perf_counter() - t0:.3f} s")
    assert total_in > 5_000_000
