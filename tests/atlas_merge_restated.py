"""The numpy restatement of vsa_atlas_merged (include/volsurfs_hip.h): box-projection charts merged into
plane-projected groups, then vsa_atlas's own charts, pack, UVs, raster and splits on the groups' plane coordinates.
The same fp32 / fp64 operations in the same order as the kernels, which are held to it bit for bit.  Everything that is
vsa_atlas's rule unchanged is imported from tests/test_atlas.py."""
import numpy as np

from volsurfs_amd._lib import VolsurfsHipError

from tests.test_atlas import (AX_U, AX_V, DEPTH_CAP, MAX_ROUNDS, _components, _join_pairs, _labels, _ord, _pack,
                              _unord)
from uv_raster_restated import raster


def face_normals(P, F):
    """The label stage's fp32 normals."""
    p0, p1, p2 = P[F[:, 0]], P[F[:, 1]], P[F[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _group_pairs(grp, e0, e1, nf):
    """(a, b, weight) of the adjacent groups a < b, sorted by (a, b)."""
    ga, gb = grp[e0], grp[e1]
    k = ga != gb
    key = np.minimum(ga[k], gb[k]) * nf + np.maximum(ga[k], gb[k])
    key, w = np.unique(key, return_counts=True)
    return key // nf, key % nf, w


def _valid(grp, n64, nn, zero, A, a, b, tt):
    """Rule 3 for every pair: one (face, pair) item per face of both groups, laid out by sorting the faces by group."""
    order = np.argsort(grp, kind="stable")
    gs = grp[order]
    start = np.searchsorted(gs, np.arange(len(grp)), side="left")
    size = np.searchsorted(gs, np.arange(len(grp)), side="right") - start
    D = A[a] + A[b]
    DD = _dot(D, D)
    bad = np.zeros(len(a), bool)
    for g in (a, b):
        cnt = size[g]
        pj = np.repeat(np.arange(len(a)), cnt)
        within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        f = order[start[g][pj] + within]
        c = _dot(n64[f], D[pj])
        ok = zero[f] | ((c > 0) & (c * c >= (tt * nn[f]) * DD[pj]))
        bad |= np.bincount(pj[~ok], minlength=len(a)) > 0
    return ~bad


def merge_groups(P, F, lab, min_cos, merge_rounds):
    """Rules 1-4: (grp [F] (the group's minimum face), merged [F] bool by group id, A [F, 3] f64 by group id, stats)."""
    nf = len(F)
    n = face_normals(P, F)
    n64 = n.astype(np.float64)
    nn = _dot(n64, n64)
    zero = (n == 0).all(1)
    e0, e1 = _join_pairs(F, np.zeros(nf, np.int64))                # the join rule's edge test without the label test
    same = lab[e0] == lab[e1]
    grp = _components(nf, e0[same], e1[same])
    A = np.zeros((nf, 3), np.float64)
    np.add.at(A, grp, n64)                                         # ascending face order, from 0
    merged = np.zeros(nf, bool)
    box_charts = len(np.unique(grp))
    tt = float(min_cos) * float(min_cos)
    rounds = 0
    while True:
        a, b, w = _group_pairs(grp, e0, e1, nf)
        ok = _valid(grp, n64, nn, zero, A, a, b, tt) if len(a) else np.zeros(0, bool)
        a, b, w = a[ok], b[ok], w[ok]
        if rounds == merge_rounds:
            break
        rounds += 1                                                # the round that finds no valid pair counts
        if len(a) == 0:
            break
        src, dst, ww = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])
        o = np.lexsort((dst, -ww, src))                            # per group: largest weight, then the smaller id
        first = np.ones(len(o), bool)
        first[1:] = src[o][1:] != src[o][:-1]
        pick = np.full(nf, -1, np.int64)
        pick[src[o][first]] = dst[o][first]
        m = (pick[a] == b) & (pick[b] == a)
        assert m.any()
        ma, mb = a[m], b[m]
        A[ma] = A[ma] + A[mb]
        merged[ma] = True
        to = np.arange(nf)
        to[mb] = ma
        grp = to[grp]
    st = {"box_charts": box_charts, "groups": len(np.unique(grp)), "merge_rounds": rounds, "valid_pairs_left": len(a)}
    return grp, merged, A, st


def frames(A, ids):
    """Rule 5: (t, b) [n, 3] f64 of the merged groups `ids`."""
    D = A[ids]
    k = np.argmin(np.abs(D), axis=1)                               # first minimum: ties to the earlier
    z = np.zeros(len(D))
    t = np.where((k == 0)[:, None], np.stack([z, -D[:, 2], D[:, 1]], 1),
                 np.where((k == 1)[:, None], np.stack([D[:, 2], z, -D[:, 0]], 1), np.stack([-D[:, 1], D[:, 0], z], 1)))
    b = np.stack([D[:, 1] * t[:, 2] - D[:, 2] * t[:, 1], D[:, 2] * t[:, 0] - D[:, 0] * t[:, 2],
                  D[:, 0] * t[:, 1] - D[:, 1] * t[:, 0]], 1)
    t = t / np.sqrt(_dot(t, t))[:, None]
    b = b / np.sqrt(_dot(b, b))[:, None]
    return t, b


def plane_coords(P, F, lab, grp, merged, A):
    """[F, 3, 2] f32: every corner's plane coordinates, by its face's label (unmerged group) or frame (merged)."""
    pc = np.stack([P[F, AX_U[lab][:, None]], P[F, AX_V[lab][:, None]]], -1).astype(np.float32)
    ids = np.flatnonzero(merged)
    if len(ids):
        t, b = frames(A, ids)
        slot = np.zeros(len(F), np.int64)
        slot[ids] = np.arange(len(ids))
        fm = np.flatnonzero(merged[grp])
        q = P[F[fm]].astype(np.float64)                            # [m, 3, 3]
        tt, bb = t[slot[grp[fm]]][:, None, :], b[slot[grp[fm]]][:, None, :]
        pc[fm] = np.stack([_dot(q, tt), _dot(q, bb)], -1).astype(np.float32)
    return pc


def _boxes_pc(pc, cidx, C):
    c = np.repeat(cidx, 3)
    ku, kv = _ord(pc[:, :, 0].reshape(-1)), _ord(pc[:, :, 1].reshape(-1))
    box = np.zeros((C, 4), np.uint32)
    box[:, 0] = box[:, 2] = 0xFFFFFFFF
    np.minimum.at(box[:, 0], c, ku)
    np.maximum.at(box[:, 1], c, ku)
    np.minimum.at(box[:, 2], c, kv)
    np.maximum.at(box[:, 3], c, kv)
    return _unord(box)


def _emit_pc(pc, cidx, box, off, s, R, p):
    c = cidx
    umin, umax, vmin, vmax = (box[c, k] for k in range(4))
    rot = (vmax - vmin) > (umax - umin)
    ox = (off[c, 0] + p).astype(np.float32)
    oy = (off[c, 1] + p).astype(np.float32)
    s, r = np.float32(s), np.float32(R)
    uv = np.zeros((len(pc), 3, 2), np.float32)
    for k in range(3):
        u, w = pc[:, k, 0], pc[:, k, 1]
        lx = np.where(rot, vmax - w, u - umin)
        ly = np.where(rot, u - umin, w - vmin)
        uv[:, k, 0] = (lx * s + ox) / r
        uv[:, k, 1] = (ly * s + oy) / r
    return uv


def restate_merged(P, F, R=1024, p=4, min_cos=0.5, merge_rounds=64, return_groups=False):
    """(faces_uvs [F, 3, 2] f32, chart [F] i32, stats) of vsa_atlas_merged's rules; with `return_groups` also
    (labels, grp, merged, A)."""
    P = np.asarray(P, np.float32)
    F = np.asarray(F, np.int64)
    nf = len(F)
    lab = _labels(P, F)
    grp, merged, A, mst = merge_groups(P, F, lab, min_cos, merge_rounds)
    pc = plane_coords(P, F, lab, grp, merged, A)
    f0, f1 = _join_pairs(F, np.zeros(nf, np.int64))
    code = np.ones(nf, np.int64)
    splits = 0
    while True:
        act = (grp[f0] == grp[f1]) & (code[f0] == code[f1]) & (code[f0] != 0)
        root = _components(nf, f0[act], f1[act])
        _, cidx = np.unique(root, return_inverse=True)
        C = int(cidx.max()) + 1
        box = _boxes_pc(pc, cidx, C)
        w, h = box[:, 1] - box[:, 0], box[:, 3] - box[:, 2]
        rot = h > w
        s, off = _pack(np.where(rot, h, w), np.where(rot, w, h), R, p)
        uv = _emit_pc(pc, cidx, box, off, s, R, p)
        _, count, pf, pt = raster(uv, R)
        flag = np.zeros(C, bool)
        flag[cidx[pf[count.reshape(-1)[pt] >= 2]]] = True
        if not flag.any():
            st = {"charts": C, "split_rounds": splits, "scale": float(s), "covered": int((count > 0).sum())}
            st.update(mst)
            out = (uv, cidx.astype(np.int32), st)
            return out + ((lab, grp, merged, A),) if return_groups else out
        if splits + 1 >= MAX_ROUNDS:
            raise VolsurfsHipError("vsa_atlas_merged: no end after MAX_ROUNDS rounds")
        sel = flag[cidx] & (code != 0)
        if not sel.any():
            raise VolsurfsHipError("vsa_atlas_merged: a split that changes nothing")
        cap = sel & (code >= 1 << DEPTH_CAP)
        code[cap] = 0
        sel &= ~cap
        c = cidx[sel]
        along_u = (box[c, 1] - box[c, 0]) >= (box[c, 3] - box[c, 2])
        lo = np.where(along_u, box[c, 0], box[c, 2]).astype(np.float64)
        hi = np.where(along_u, box[c, 1], box[c, 3]).astype(np.float64)
        cs = [np.where(along_u, pc[sel, k, 0], pc[sel, k, 1]).astype(np.float64) for k in range(3)]
        side = ((cs[0] + cs[1]) + cs[2]) > 1.5 * (lo + hi)
        code[sel] = 2 * code[sel] + side
        splits += 1
