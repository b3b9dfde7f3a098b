"""The mesh-smoothing rule (include/volsurfs_hip.h "Mesh smoothing") restated in numpy, written from the rule
and in the device's operation order, on top of tests/mesh_intersect_restated.py (`crosses`: the crossing rule) and
tests/mesh_sdf_restated.py (the sign `nested` asks for).  No torch.  The reference has no such stage: the rule is this
library's own and unpinned.  Every comparison of the device with this file is exact equality: the vertices' bits and
every report field.

Crossings are asked of the pairs whose fp32 bounding boxes overlap (closed) only, as tests/simplify_guarded_restated.py
does: triangles with disjoint boxes are separated by an axis plane and cross nothing, and the device prunes by boxes
that are no tighter (its q16 boxes contain these).  `tests/test_mesh_smooth.py` holds the filtered counts to the brute
force of `mesh_intersect_restated` on the stacks it uses.

Also the meshes the tests share."""
import numpy as np

import mesh_intersect_restated as X
import mesh_sdf_restated as S

F32 = np.float32
FIELDS = ("shell", "guards", "iterations", "moved_vertices", "max_displacement", "boundary_vertices", "stuck",
          "reverted", "guard_rounds", "self_crossings_after")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


# ---- topology

def topology(faces, V):
    """The rings and the boundary flags of `faces` [F, 3] over V vertices: {v, a, b, rank: per corner slot in ring order
    (sorted by vertex, stable: ascending slot within a vertex) the vertex, the next corner's vertex, the one after, and
    the slot's position in its ring; slots [V] = the ring sizes; boundary [V] bool}."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    corners = f.reshape(-1)
    order = np.argsort(corners, kind="stable")
    v = corners[order]
    face, c = order // 3, order % 3
    a, b = f[face, (c + 1) % 3], f[face, (c + 2) % 3]
    slots = np.bincount(v, minlength=V)
    start = np.cumsum(slots) - slots
    rank = np.arange(len(v)) - start[v]
    x, y = corners, f[:, [1, 2, 0]].reshape(-1)                    # the edge of slot 3 f + c: corner c to the next
    lo, hi = np.minimum(x, y), np.maximum(x, y)
    keys, first, count = np.unique(lo << 32 | hi, return_index=True, return_counts=True)
    once = first[count == 1]
    boundary = np.zeros(V, bool)
    boundary[lo[once]] = True
    boundary[hi[once]] = True
    return {"v": v, "a": a, "b": b, "rank": rank, "slots": slots, "boundary": boundary}


def half_step(P, topo, w, fix_boundary=True):
    """(Q, stuck mask) of one half-step with weight w: every vertex reads P."""
    P = np.asarray(P, F32)
    V = len(P)
    slots = topo["slots"]
    free = slots > 0
    if fix_boundary:
        free &= ~topo["boundary"]
    acc = np.zeros((V, 3), F32)
    with np.errstate(all="ignore"):
        for r in range(int(slots.max()) if V else 0):              # slot r of every ring that has one, in ring order
            sel = topo["rank"] == r
            v = topo["v"][sel]
            acc[v] = (acc[v] + P[topo["a"][sel]]) + P[topo["b"][sel]]
        n = (2 * slots).astype(F32)
        cen = acc / n[:, None]
        t = F32(w) * (cen - P)                                      # a multiply, then an add
        new = P + t
    assert acc.dtype == F32 and cen.dtype == F32 and t.dtype == F32 and new.dtype == F32
    ok = np.isfinite(new).all(1)
    stuck = free & ~ok
    return np.where((free & ok)[:, None], new, P), stuck


# ---- crossings

def _tris(v, f):
    """[F', 3, 3] float64 of a mesh, and the ids of its faces: a face with an index outside the vertex array is none."""
    v = np.asarray(v, F32).astype(np.float64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    return v[f[ok]], np.nonzero(ok)[0]


def _near(T, B, lo, chunk):
    with np.errstate(all="ignore"):
        tlo, thi, blo, bhi = T[lo:lo + chunk].min(-2), T[lo:lo + chunk].max(-2), B.min(-2), B.max(-2)
        return np.nonzero(((tlo[:, None] <= bhi[None]) & (thi[:, None] >= blo[None])).all(-1))


def crossing_pairs(va, fa, vb, fb, chunk=1024):
    """The set of (face of a, face of b) that cross, a's face as A."""
    T, ta = _tris(va, fa)
    B, tb = _tris(vb, fb)
    out = set()
    for lo in range(0, len(T), chunk):
        i, j = _near(T, B, lo, chunk)
        hit = X.crosses(T[lo + i], B[j]) if len(i) else np.zeros(0, bool)
        out.update(zip(ta[lo + i[hit]].tolist(), tb[j[hit]].tolist()))
    return out


def self_crossing_count(v, f, chunk=1024):
    """The crossing pairs i < j of one mesh's faces, face i as A."""
    T, _ = _tris(v, f)
    total = 0
    for lo in range(0, len(T), chunk):
        i, j = _near(T, T, lo, chunk)
        keep = lo + i < j
        i, j = i[keep], j[keep]
        if len(i):
            total += int(X.crosses(T[lo + i], T[j]).sum())
    return total


def bad_faces(P, Q, faces, guards):
    """bool [F]: the faces with a vertex whose bits differ between Q and P that cross a face of a guard."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    differs = (_bits(Q) != _bits(P)).any(1)
    live = np.nonzero(differs[f].any(1))[0]
    bad = np.zeros(len(f), bool)
    for gv, gf in guards:
        hit = {a for a, _ in crossing_pairs(Q, f[live], gv, gf)}
        bad[live[sorted(hit)]] = True
    return bad


# ---- the stage

def restate(P, faces, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, guards=()):
    """(vertices, report dict without shell / guards, log of (reverted, guard rounds) per iteration) of `smooth_mesh`;
    `guards`: (vertices, faces) pairs."""
    P0 = np.array(P, F32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    topo = topology(f, len(P0))
    cur, stuck, log = P0, 0, []
    for _ in range(iterations):
        mid, s1 = half_step(cur, topo, lam, fix_boundary)
        new, s2 = half_step(mid, topo, mu, fix_boundary)
        stuck += int(s1.sum()) + int(s2.sum())
        reverted = rounds = 0
        while guards:
            rounds += 1
            back = np.zeros(len(cur), bool)
            back[f[bad_faces(cur, new, f, guards)].reshape(-1)] = True
            back &= (_bits(new) != _bits(cur)).any(1)
            if not back.any():
                break
            new = np.where(back[:, None], cur, new)
            reverted += int(back.sum())
        log.append((reverted, rounds))
        cur = new
    changed = (_bits(cur) != _bits(P0)).any(1)
    d = cur.astype(np.float64) - P0.astype(np.float64)
    with np.errstate(all="ignore"):
        disp = np.where(changed, np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]), 0.0)
    report = {"iterations": iterations, "moved_vertices": int(changed.sum()), "max_displacement": float(disp.max()),
              "boundary_vertices": int(topo["boundary"].sum()), "stuck": stuck,
              "reverted": sum(r for r, _ in log), "guard_rounds": sum(n for _, n in log),
              "self_crossings_after": self_crossing_count(cur, f) if np.isfinite(cur).all() else None}
    return cur, report, log


def stack_order(K, anchor=None):
    """[(shell, guards)] in the order `smooth_shells` takes the shells (`simplify.stack_order`): guards are ("in", k) =
    input shell k or ("out", k) = the already smoothed shell k, lower shell first."""
    anchor = K // 2 if anchor is None else int(anchor)
    order = [(anchor, [("in", k) for k in (anchor - 1, anchor + 1) if 0 <= k < K])]
    for k in range(anchor + 1, K):
        order.append((k, [("out", k - 1)] + ([("in", k + 1)] if k + 1 < K else [])))
    for k in range(anchor - 1, -1, -1):
        order.append((k, ([("in", k - 1)] if k - 1 >= 0 else []) + [("out", k + 1)]))
    return order


def _components_first_vertex(f):
    """One vertex (corner 0 of the lowest face) of every edge-connected component of the faces."""
    f = np.asarray(f, np.int64)
    par = list(range(len(f)))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    seen = {}
    for i, (a, b, c) in enumerate(f.tolist()):
        for e in ((a, b), (b, c), (c, a)):
            e = (min(e), max(e))
            if e in seen:
                x, y = find(seen[e]), find(i)
                par[max(x, y)] = min(x, y)
            else:
                seen[e] = i
    return f[sorted({find(i) for i in range(len(f))}), 0]


def nested(meshes):
    """`mesh_intersect.shells_nested` with the pseudonormal sign: per consecutive pair, no crossing pair and one vertex
    of every component of shell k at a negative signed distance to shell k + 1."""
    out = []
    for (va, fa), (vb, fb) in zip(meshes[:-1], meshes[1:]):
        if crossing_pairs(va, fa, vb, fb):
            out.append(False)
            continue
        d = S.signed_distance(np.asarray(va, F32)[_components_first_vertex(fa)], vb, fb)["dist"]
        out.append(bool((d < 0).all()))
    return out


def restate_shells(meshes, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, anchor=None):
    """(list of vertices, K report dicts, {crossings_in, crossings_out, nested}) of `smooth_shells`."""
    K = len(meshes)
    out, reports = [None] * K, [None] * K
    for k, names in stack_order(K, anchor):
        guards = [meshes[g] if which == "in" else (out[g], meshes[g][1]) for which, g in names]
        out[k], rep, _ = restate(meshes[k][0], meshes[k][1], iterations, lam, mu, fix_boundary, guards)
        reports[k] = dict(rep, shell=k, guards=tuple(names))
    done = [(out[k], meshes[k][1]) for k in range(K)]
    stack = {"crossings_in": [len(crossing_pairs(*meshes[k], *meshes[k + 1])) for k in range(K - 1)],
             "crossings_out": [len(crossing_pairs(*done[k], *done[k + 1])) for k in range(K - 1)],
             "nested": nested(done)}
    return out, reports, stack


# ---- the meshes the tests share

def noisy_sphere():
    """icosphere(3, 0.5) with every vertex scaled by 1 + U(-0.04, 0.04): 642 vertices, 1 280 faces."""
    from volsurfs_amd.mesh import icosphere
    v, f = icosphere(3, 0.5)
    scale = 1.0 + np.random.default_rng(0).uniform(-0.04, 0.04, len(v))
    return (v * scale[:, None]).astype(F32), np.asarray(f, np.int32)


def open_mesh():
    """The noisy sphere without every face that has a vertex with z > 0.35."""
    v, f = noisy_sphere()
    return v, f[~(v[f][:, :, 2] > 0.35).any(1)]


def fan(n=200):
    """One apex over a rim of n vertices: a ring of n slots, longer than a wave; the apex lifted off the rim's plane."""
    t = 2.0 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(t), np.sin(t), 0.05 * np.sin(5.0 * t)], 1)
    v = np.concatenate([[[0.1, -0.05, 0.4]], rim]).astype(F32)
    f = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1).astype(np.int32)
    return v, f


def radius_stats(v):
    r = np.sqrt((np.asarray(v, np.float64) ** 2).sum(1))
    return float(r.mean()), float(r.std())
