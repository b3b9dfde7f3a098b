"""Guarded simplification (include/volsurfs_hip.h "Mesh simplification", the `guard` condition) restated in
numpy: `tests.test_simplify.restate`'s loop, part for part, with one more candidate condition -- no face a collapse
would create may cross a face of a guard mesh, by `mesh_intersect_restated.crosses` -- and the stack order of
`simplify.simplify_shells`.  Every comparison of the device with this file is exact equality.

The bounding-box prefilter in front of `crosses` cannot change a verdict: two triangles whose closed boxes are disjoint
have no common point, and a box with a NaN bound belongs to a face that crosses nothing."""
import numpy as np

from tests import mesh_intersect_restated as mir
from tests.test_simplify import NONE, _candidates, _init_quadrics, _key, _place, _ring_pairs
from volsurfs_amd import simplify as smp

REPORT_FIELDS = ("shell", "guards", "faces_in", "faces_out", "target", "rounds", "collapses", "stalled",
                 "guard_rejected", "self_crossings")


def guard_triangles(vertices, faces):
    """[F', 3, 3] float64 of a guard mesh: a face with an index outside the vertex array is no face."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    return v[f[((f >= 0) & (f < len(v))).all(1)]]


def _boxes(T):
    with np.errstate(all="ignore"):
        return T.min(-2), T.max(-2)


def any_cross(T, B, chunk=4096):
    """bool [N]: does triangle T[i] (as A) cross any triangle of B."""
    out = np.zeros(len(T), bool)
    if len(T) == 0 or len(B) == 0:
        return out
    tlo, thi = _boxes(T)
    blo, bhi = _boxes(B)
    for lo in range(0, len(T), chunk):
        with np.errstate(all="ignore"):
            near = ((tlo[lo:lo + chunk, None] <= bhi[None]) & (thi[lo:lo + chunk, None] >= blo[None])).all(-1)
        i, j = np.nonzero(near)
        if len(i):
            hit = mir.crosses(T[lo + i], B[j])
            out[lo + i[hit]] = True
    return out


def guard_ok(P, F, ea, eb, p, ok, guards):
    """bool [E]: the candidates `ok` that pass the guard.  For every face at a or b without both, in its corner order
    with the moved vertex at p: it crosses no face of any guard (triangle arrays of `guard_triangles`)."""
    V = len(P)
    P64 = P.astype(np.float64)
    sel = np.nonzero(ok)[0]
    bad = np.zeros(len(ea), bool)
    for m, other in ((ea, eb), (eb, ea)):
        eid, f = _ring_pairs(F, V, m[sel])
        c = F[f]
        keep = ~(c == other[sel][eid][:, None]).any(1)
        eid, c = eid[keep], c[keep]
        moved = c == m[sel][eid][:, None]
        T = np.where(moved[:, :, None], p[sel][eid].astype(np.float64)[:, None, :], P64[c])
        hit = np.zeros(len(T), bool)
        for B in guards:
            hit |= any_cross(T, B)
        bad[sel[eid[hit]]] = True
    return ok & ~bad


def restate(P, F, ratio, guards=()):
    """(V_out [V, 3] f32, F_out [F, 3] i32, stats) of the rules in include/volsurfs_hip.h with the guard condition;
    `guards`: (vertices, faces) pairs.  stats has `guard_rejected`: the (round, edge) verdicts the guard turned down."""
    guards = [guard_triangles(v, f) for v, f in guards]
    P = np.array(P, np.float32)
    F = np.array(F, np.int64)
    V = len(P)
    target = smp.target_faces(len(F), ratio)
    Q = _init_quadrics(P, F)
    rounds = collapses = rejected = 0
    stalled = False
    while len(F) > target:
        a, b = F, np.roll(F, -1, axis=1)
        uk, cnt = np.unique((np.minimum(a, b) * V + np.maximum(a, b)).reshape(-1), return_counts=True)
        ea, eb = uk // V, uk % V
        bnd, frz = np.zeros(V, bool), np.zeros(V, bool)
        bnd[ea[cnt == 1]] = bnd[eb[cnt == 1]] = True
        frz[ea[cnt > 2]] = frz[eb[cnt > 2]] = True
        p, cost = _place(P, Q, ea, eb, bnd)
        ok = _candidates(P, F, ea, eb, cnt, bnd, frz, p, cost)
        if guards:
            passed = guard_ok(P, F, ea, eb, p, ok, guards)
            rejected += int((ok & ~passed).sum())
            ok = passed
        key = _key(cost, ok)
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
    st = {"rounds": rounds, "collapses": collapses, "stalled": stalled, "faces_out": len(F), "target": target,
          "guard_rejected": rejected}
    return P[used], new[F].astype(np.int32), st


def crossing_pairs(a, b):
    return len(mir.mesh_crossings(a[0], a[1], b[0], b[1])["pairs"])


def stack_order(K, anchor=None):
    """[(shell, guards)] in the order `simplify_shells` takes the shells: guards are ("in", k) = input shell k or
    ("out", k) = the already simplified shell k, lower shell first."""
    anchor = K // 2 if anchor is None else int(anchor)
    order = [(anchor, [("in", k) for k in (anchor - 1, anchor + 1) if 0 <= k < K])]
    for k in range(anchor + 1, K):
        order.append((k, [("out", k - 1)] + ([("in", k + 1)] if k + 1 < K else [])))
    for k in range(anchor - 1, -1, -1):
        order.append((k, ([("in", k - 1)] if k - 1 >= 0 else []) + [("out", k + 1)]))
    return order


def restate_shells(meshes, ratio, anchor=None):
    """(outputs [(V, F)], reports [dict of REPORT_FIELDS], crossings_in, crossings_out) of `simplify_shells`."""
    K = len(meshes)
    out, reports = [None] * K, [None] * K
    for k, names in stack_order(K, anchor):
        guards = [meshes[g] if which == "in" else out[g] for which, g in names]
        v, f, st = restate(meshes[k][0], meshes[k][1], ratio, guards)
        out[k] = (v, f)
        reports[k] = {"shell": k, "guards": tuple(names), "faces_in": len(meshes[k][1]), "faces_out": st["faces_out"],
                      "target": st["target"], "rounds": st["rounds"], "collapses": st["collapses"],
                      "stalled": st["stalled"], "guard_rejected": st["guard_rejected"],
                      "self_crossings": len(mir.self_crossings(v, f)["pairs"])}
    cin = [crossing_pairs(meshes[k], meshes[k + 1]) for k in range(K - 1)]
    cout = [crossing_pairs(out[k], out[k + 1]) for k in range(K - 1)]
    return out, reports, cin, cout


def lobed_stack(amp, gap, K=3, subdiv=2):
    """G1 / G2: K lobed icospheres, inner to outer, float32, NOT rotated: the unit icosphere with each vertex scaled by
    0.40 + gap k + amp sin(3 atan2(y, x)) sin(3 acos(z)) (`shell_untangle_restated.lobed_stack` without its rotation)."""
    from volsurfs_amd.mesh import icosphere
    F32 = np.float32
    v, f = icosphere(subdiv)
    v = (v / np.sqrt((v * v).sum(1, keepdims=True, dtype=F32))).astype(F32)
    out = []
    for k in range(K):
        lobes = np.sin(F32(3.0) * np.arctan2(v[:, 1], v[:, 0])) * np.sin(F32(3.0) * np.arccos(np.clip(v[:, 2], -1, 1)))
        radius = (F32(0.40) + F32(gap) * F32(k)) + F32(amp) * lobes.astype(F32)
        out.append(((v * radius[:, None]).astype(F32), f.copy()))
    return out


G1 = dict(amp=0.06, gap=0.03)
G2 = dict(amp=0.08, gap=0.02)
G_RATIO = 0.25
