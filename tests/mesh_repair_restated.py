"""What tests/test_mesh_repair.py shares: the mesh-repair rules (include/volsurfs_hip.h "Mesh repair") restated
in numpy and scipy's `connected_components`, and the scrambled soups the tests repair.  Written from the rules' text:
float64 with the stated order of operations inside a term; the sums over a component are numpy's, so S and U agree with
the device to rounding while every discrete result (maps, flips, components, counts) is meant to be equal."""
import functools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import mesh_winding_restated as W

F32 = np.float32
NAMES = W.NAMES
CELL_HALF = 1 << 20
DECIDE = 2.0 ** -20


# ---- the inputs

@functools.lru_cache(maxsize=None)
def soup(name):
    """(vertices [3F, 3] f32, faces [F, 3] i32, flipped [F] bool) of `mesh_winding_restated.mesh(name)` un-welded to 3 F
    vertices, the vertices shuffled and each face flipped (corners 1 and 2 swapped) with probability 0.4, all from
    default_rng(11).  Face f of the soup is face f of the mesh."""
    v, f = W.mesh(name)
    nf = f.shape[0]
    rng = np.random.default_rng(11)
    order = rng.permutation(3 * nf)
    flip = rng.random(nf) < 0.4
    corners = v[f.reshape(-1).astype(np.int64)]
    inv = np.empty(3 * nf, np.int64)
    inv[order] = np.arange(3 * nf)
    faces = inv.reshape(nf, 3).astype(np.int32)
    faces[flip] = faces[flip][:, [0, 2, 1]]
    return np.ascontiguousarray(corners[order], F32), np.ascontiguousarray(faces), flip


@functools.lru_cache(maxsize=None)
def mobius(segments=24):
    """A Moebius strip of 2 `segments` faces, wound consistently along the strip (the seam is where it cannot be)."""
    t = 2.0 * np.pi * np.arange(segments) / segments
    radial = np.stack([np.cos(t), np.sin(t), np.zeros_like(t)], 1)
    across = np.cos(t / 2)[:, None] * radial + np.sin(t / 2)[:, None] * np.array([0.0, 0.0, 1.0])
    v = np.empty((2 * segments, 3))
    v[0::2] = 0.3 * radial - 0.08 * across
    v[1::2] = 0.3 * radial + 0.08 * across
    faces = []
    for i in range(segments):
        a0, b0 = 2 * i, 2 * i + 1
        a1, b1 = (2 * i + 2, 2 * i + 3) if i + 1 < segments else (1, 0)       # the half twist: the rims swap
        faces += [[a0, b0, a1], [b0, b1, a1]]
    return v.astype(F32), np.asarray(faces, np.int32)


# ---- grouping

def group_rows(rows):
    """rep [n]: the lowest index whose row equals row i."""
    rows = np.asarray(rows)
    _, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.full(inv.max() + 1, rows.shape[0], np.int64)
    np.minimum.at(first, inv, np.arange(rows.shape[0]))
    return first[inv]


def _lowest_of_component(n, a, b):
    """rep [n]: the lowest node of each connected component of the graph with edges (a[k], b[k])."""
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n))
    _, label = connected_components(g, directed=False)
    first = np.full(label.max() + 1, n, np.int64)
    np.minimum.at(first, label, np.arange(n))
    return first[label]


# ---- weld

def weld_rep(v, tol):
    """rep [V]: the lowest vertex of each vertex's cluster."""
    v = np.asarray(v, F32)
    n = v.shape[0]
    nan = np.isnan(v).any(1)
    if tol == 0.0:
        bits = v.view(np.uint32).copy()
        bits[bits == 0x80000000] = 0
        rep = group_rows(bits)
        rep[nan] = np.arange(n)[nan]
        return rep
    p = v.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        cell = np.floor(p / np.float64(tol))
    out = ~nan & ((cell < -CELL_HALF) | (cell >= CELL_HALF)).any(1)
    if out.any():
        raise ValueError(f"tol = {tol}: a cell index leaves +-2^20")
    tol2 = np.float64(tol) * np.float64(tol)
    a, b = [], []
    for lo in range(0, n, 512):
        d = p[lo:lo + 512, None, :] - p[None, :, :]
        with np.errstate(invalid="ignore"):
            near = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) <= tol2
        i, j = np.nonzero(near)
        a.append(i + lo)
        b.append(j)
    return _lowest_of_component(n, np.concatenate(a), np.concatenate(b))


def weld(v, f, tol=0.0, drop_degenerate=True, drop_duplicates=True):
    """{vertices, faces, vertex_map, face_map, report} by the rule."""
    v, f = np.asarray(v, F32), np.asarray(f, np.int32)
    rep = weld_rep(v, tol)
    is_rep = rep == np.arange(v.shape[0])
    new = np.cumsum(is_rep) - is_rep
    vmap = new[rep].astype(np.int32)
    nf = vmap[f.astype(np.int64)]
    degenerate = (nf[:, 0] == nf[:, 1]) | (nf[:, 1] == nf[:, 2]) | (nf[:, 2] == nf[:, 0])
    gone = degenerate if drop_degenerate else np.zeros(f.shape[0], bool)
    dup = np.zeros(f.shape[0], bool)
    if drop_duplicates:
        dup = ~gone & (group_rows(np.sort(nf, axis=1)) != np.arange(f.shape[0]))
    keep = ~gone & ~dup
    fmap = np.where(keep, np.cumsum(keep) - keep, -1).astype(np.int32)
    report = {"vertices_in": int(v.shape[0]), "vertices_out": int(is_rep.sum()), "degenerate_dropped": int(gone.sum()),
              "duplicates_dropped": int(dup.sum())}
    return {"vertices": v[is_rep], "faces": np.ascontiguousarray(nf[keep]).astype(np.int32), "vertex_map": vmap,
            "face_map": fmap, "report": report, "keep": keep, "rep": rep}


# ---- orient

def _normals(v, f):
    p = np.asarray(v, F32).astype(np.float64)[np.asarray(f, np.int64)]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    return n, p


def normals(v, f):
    """[F, 3] float64: (v1 - v0) x (v2 - v0)."""
    return _normals(v, f)[0]


def constraints(v, f):
    """(f [M], g [M], par [M]): the pairs of live faces tied by an edge that exactly two live, different faces name;
    par = both traverse it in the same direction."""
    f = np.asarray(f, np.int64)
    nf, nv = f.shape[0], int(np.asarray(v).shape[0])
    n, _ = _normals(v, f)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    live = (length > 0.0) & (length < np.inf)
    a = f.reshape(-1)                                         # slot 3 f + c: from corner c to the next
    b = f[:, [1, 2, 0]].reshape(-1)
    face = np.repeat(np.arange(nf), 3)
    key = np.minimum(a, b) * nv + np.maximum(a, b)
    sel = live[face]
    key, a, face = key[sel], a[sel], face[sel]
    order = np.argsort(key, kind="stable")
    key, a, face = key[order], a[order], face[order]
    _, start, count = np.unique(key, return_index=True, return_counts=True)
    two = start[count == 2]
    fa, fb, par = face[two], face[two + 1], a[two] == a[two + 1]
    ok = fa != fb
    return fa[ok], fb[ok], par[ok].astype(np.int64)


def orient(v, f, outward=True):
    """{faces, flipped, component, report, ratio = {lowest face of an orientable component: |S| / U}} by the rule."""
    v, f = np.asarray(v, F32), np.asarray(f, np.int32)
    nf = f.shape[0]
    fa, fb, par = constraints(v, f)
    root = _lowest_of_component(2 * nf, np.concatenate([2 * fa, 2 * fa + 1]),
                                np.concatenate([2 * fb + par, 2 * fb + 1 - par]))
    component = (root[0::2] >> 1).astype(np.int32)
    rel = (root[0::2] & 1).astype(bool)
    orientable = root[0::2] != root[1::2]
    n, p = _normals(v, f)
    n = 0.5 * n
    with np.errstate(invalid="ignore", over="ignore"):
        area = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ok = area < np.inf
    n[rel] = -n[rel]
    c = ((p[:, 0] + p[:, 1]) + p[:, 2]) / 3.0
    area0 = np.where(ok, area, 0.0)
    ac = np.where(ok[:, None], area[:, None] * c, 0.0)
    sum_a = np.bincount(component, area0, nf)
    sum_ac = np.stack([np.bincount(component, ac[:, k], nf) for k in range(3)], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cbar = np.where(sum_a[:, None] > 0.0, sum_ac / sum_a[:, None], 0.0)
    d = c - cbar[component]
    s = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    q = cbar[component]
    u = area * (((np.abs(c[:, 0]) + np.abs(c[:, 1])) + np.abs(c[:, 2]))
                + ((np.abs(q[:, 0]) + np.abs(q[:, 1])) + np.abs(q[:, 2])))
    S = np.bincount(component, np.where(ok, s, 0.0), nf)
    U = np.bincount(component, np.where(ok, u, 0.0), nf)
    lowest = np.unique(component)
    comp_orientable = orientable[lowest]
    decided = np.zeros(nf, bool)
    decided[lowest] = comp_orientable & (np.abs(S[lowest]) > DECIDE * U[lowest])
    flip_c = decided & ((S < 0.0) if outward else (S > 0.0))
    flipped = orientable & (rel ^ flip_c[component])
    faces = f.copy()
    faces[flipped] = faces[flipped][:, [0, 2, 1]]
    undecided = np.zeros(nf, bool)
    undecided[lowest] = comp_orientable & ~decided[lowest]
    sizes = np.bincount(component, minlength=nf)
    report = {"components": int(lowest.size), "flipped": int(flipped.sum()),
              "unorientable_components": int((~comp_orientable).sum()),
              "undecided_components": int(undecided.sum()), "undecided_faces": int(sizes[undecided].sum())}
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = {int(m): float(abs(S[m]) / U[m]) if U[m] > 0 else 0.0 for m in lowest[comp_orientable]}
    return {"faces": faces, "flipped": flipped, "component": component, "report": report, "ratio": ratio,
            "decided_face": decided[component], "S": S, "U": U}


@functools.lru_cache(maxsize=None)
def welded(name):
    """`weld` of `soup(name)` at tol = 0."""
    v, f, _ = soup(name)
    return weld(v, f)


@functools.lru_cache(maxsize=None)
def oriented(name):
    """`orient` of `welded(name)` (`mobius`: of the strip as built)."""
    if name == "mobius":
        return orient(*mobius())
    w = welded(name)
    return orient(w["vertices"], w["faces"])


def census(v, f):
    """{boundary, non_manifold, inconsistent} of `mesh_winding.edge_census`, restated."""
    f = np.asarray(f, np.int64)
    nf, nv = f.shape[0], int(np.asarray(v).shape[0])
    n, _ = _normals(v, f)
    length = np.sqrt((n * n).sum(1))
    live = (length > 0.0) & (length < np.inf)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    sel = live[np.repeat(np.arange(nf), 3)]
    key, a = (np.minimum(a, b) * nv + np.maximum(a, b))[sel], a[sel]
    order = np.argsort(key, kind="stable")
    key, a = key[order], a[order]
    _, start, count = np.unique(key, return_index=True, return_counts=True)
    two = start[count == 2]
    return {"boundary": int((count == 1).sum()), "non_manifold": int((count > 2).sum()),
            "inconsistent": int((a[two] == a[two + 1]).sum())}
