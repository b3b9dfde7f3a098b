"""The shell-untangling rule (include/volsurfs_hip.h "Shell untangling") restated in numpy, written from the
rule, on top of tests/mesh_sdf_restated.py (`signed_distance`: r, normal, unsigned and dist are exactly what the rule
needs) and tests/mesh_intersect_restated.py (`mesh_crossings`, `self_crossings`).  The reference has no such stage: the
rule is this library's own and unpinned.  Every comparison of the device with this file is exact equality.

Also the lobed stacks the tests share."""
import numpy as np

import mesh_intersect_restated as X
import mesh_sdf_restated as S

F32 = np.float32
FIELDS = ("shell", "side", "against", "rounds", "moved_vertices", "max_displacement", "max_level", "stuck",
          "crossings_before", "crossings_after", "self_crossings_after", "converged")


def signed_query(points, xv, xf, table, sign="pseudonormal"):
    """`mesh_sdf_restated.signed_distance`; sign="winding": dist negative iff the exact float64 winding number exceeds
    1/2 (the device sums it in float32 with a far field: a property, not a bit-exact yardstick)."""
    q = S.signed_distance(points, xv, xf, table)
    if sign == "winding":
        w = S.winding_number(points, xv, xf)
        q["dist"] = np.where(w > 0.5, -q["unsigned"], q["unsigned"]).astype(F32)
    return q


def project(v, level, xv, xf, table, side, margin, max_level, sign="pseudonormal"):
    """Step 1 for all vertices: (new vertices, moved mask, stuck mask, t)."""
    q = signed_query(v, xv, xf, table, sign)
    dist, ad, r, n = q["dist"], q["unsigned"], q["r"], q["normal"]
    s = F32(side)
    with np.errstate(all="ignore"):
        m = F32(margin) * np.exp2(np.minimum(level, max_level)).astype(F32)
        violated = s * dist < m                                   # (a NaN never is)
        t = s * (F32(1.25) * m) - dist
        g_r = r / ad[:, None]
        g_r = np.where((dist < 0)[:, None], -g_r, g_r)
        length = np.sqrt(S.R.dot3(n[:, 0], n[:, 1], n[:, 2], n[:, 0], n[:, 1], n[:, 2]))
        g_n = n / length[:, None]
        g = np.where((ad > 0)[:, None], g_r, g_n)
        step = t[:, None] * g                                     # a multiply, then an add
        new = v + step
    assert m.dtype == F32 and t.dtype == F32 and g.dtype == F32 and new.dtype == F32
    ok = np.isfinite(g).all(1)
    moved, stuck = violated & ok, violated & ~ok
    return np.where(moved[:, None], new, v), moved, stuck, t


def untangle_pair(mv, mf, xv, xf, side, margin=1e-3, max_rounds=16, max_level=6, sign="pseudonormal"):
    """One moving shell (mv, mf) against one fixed shell (xv, xf): (vertices, report dict without shell / against,
    log of (moved, stuck, max |t|, P) per round)."""
    v0 = np.asarray(mv, F32)
    v, mf = v0.copy(), np.asarray(mf, np.int64)
    xv, xf = np.asarray(xv, F32), np.asarray(xf, np.int64)
    table = S.pseudonormal_table(xv, xf)
    level = np.zeros(v.shape[0], np.int64)
    before = len(X.mesh_crossings(v, mf, xv, xf)["pairs"])
    log, converged = [], False
    for _ in range(max_rounds):
        v, moved, stuck, t = project(v, level, xv, xf, table, side, margin, max_level, sign)
        cr = X.mesh_crossings(v, mf, xv, xf)
        P = len(cr["pairs"])
        log.append((int(moved.sum()), int(stuck.sum()), float(np.abs(t[moved]).max()) if moved.any() else 0.0, P))
        if not moved.any() and P == 0:
            converged = True
            break
        level[np.unique(mf[cr["count_a"] > 0])] += 1              # once per vertex and round
    changed = (v.view(np.int32) != v0.view(np.int32)).any(1)
    d = v.astype(np.float64) - v0.astype(np.float64)
    with np.errstate(all="ignore"):
        disp = np.where(changed, np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]), 0.0)
    report = {"side": side, "rounds": len(log), "moved_vertices": int(changed.sum()),
              "max_displacement": float(disp.max()), "max_level": int(level.max()), "stuck": log[-1][1],
              "crossings_before": before, "crossings_after": log[-1][3],
              "self_crossings_after": len(X.self_crossings(v, mf)["pairs"]), "converged": converged}
    return v, report, log


def untangle_shells(meshes, anchor=None, **kw):
    """The stack: `meshes` a list of (vertices, faces), inner to outer.  (list of vertices, list of K report dicts)."""
    K = len(meshes)
    anchor = K // 2 if anchor is None else anchor
    out = [np.asarray(v, F32).copy() for v, _ in meshes]
    reports = [None] * K
    for k, against, side in ([(k, k - 1, 1) for k in range(anchor + 1, K)] +
                             [(k, k + 1, -1) for k in range(anchor - 1, -1, -1)]):
        out[k], rep, _ = untangle_pair(out[k], meshes[k][1], out[against], meshes[against][1], side, **kw)
        reports[k] = dict(rep, shell=k, against=against)
    reports[anchor] = {"shell": anchor, "side": 0, "against": None, "rounds": 0, "moved_vertices": 0,
                       "max_displacement": 0.0, "max_level": 0, "stuck": 0, "crossings_before": 0, "crossings_after": 0,
                       "self_crossings_after": len(X.self_crossings(out[anchor], meshes[anchor][1])["pairs"]),
                       "converged": True}
    return out, reports


# ---- the stacks the tests share

def lobed_stack(subdiv, K, amp, gap):
    """K lobed icospheres, inner to outer, float32: the unit icosphere rotated about z by 0.35 k, each vertex scaled
    by 0.40 + gap k + amp sin(3 atan2(y, x)) sin(3 acos(z))."""
    from volsurfs_amd.mesh import icosphere
    v, f = icosphere(subdiv)
    v = (v / np.sqrt((v * v).sum(1, keepdims=True, dtype=F32))).astype(F32)
    out = []
    for k in range(K):
        c, s = F32(np.cos(0.35 * k)), F32(np.sin(0.35 * k))
        p = np.stack([c * v[:, 0] - s * v[:, 1], s * v[:, 0] + c * v[:, 1], v[:, 2]], 1).astype(F32)
        lobes = np.sin(F32(3.0) * np.arctan2(p[:, 1], p[:, 0])) * np.sin(F32(3.0) * np.arccos(np.clip(p[:, 2], -1, 1)))
        radius = (F32(0.40) + F32(gap) * F32(k)) + F32(amp) * lobes.astype(F32)
        out.append(((p * radius[:, None]).astype(F32), f.copy()))
    return out


STACK_A = dict(subdiv=2, K=3, amp=0.06, gap=0.03)      # margin 0.005
STACK_B = dict(subdiv=2, K=5, amp=0.08, gap=0.02)      # margin 0.004
MARGIN_A, MARGIN_B = 0.005, 0.004
