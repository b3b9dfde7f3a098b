"""What tests/test_mesh_winding.py shares: the meshes and queries the issue fixes, and the winding-number rule's tree part
(include/volsurfs_hip.h "Mesh winding number") restated in float64 over exported q16 nodes: the moments of
every subtree and the depth-first walk with the order-0 far field.  The exact sum's oracle is
tests/mesh_sdf_restated.py::winding_number.  Written from the rule; float64 throughout, so it agrees with the device to
rounding, not bit for bit."""
import functools

import numpy as np

import mesh_sdf_restated as S

F32 = np.float32
EMPTY = 0x7fffffff
NAMES = ("closed", "capped", "holes", "cube_open", "two_spheres", "lobed")


# ---- the meshes and the queries

def _icosphere(subdiv, radius):
    from volsurfs_amd.mesh import icosphere
    v, f = icosphere(subdiv, radius)
    return np.asarray(v, F32), np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices [V, 3] float32, faces [F, 3] int32) of one of NAMES."""
    if name == "closed":
        return _icosphere(3, 0.34)
    if name == "capped":                                   # the sphere without its cap: one hole, 1 148 faces
        v, f = mesh("closed")
        z = v[f.astype(np.int64)].astype(np.float64).mean(1)[:, 2]
        return v, np.ascontiguousarray(f[~(z >= 0.8 * 0.34)])
    if name == "holes":                                    # every face dropped with probability 0.2
        v, f = mesh("closed")
        drop = np.random.default_rng(5).random(f.shape[0]) < 0.2
        return v, np.ascontiguousarray(f[~drop])
    if name == "cube_open":                                # the cube without one side
        v, f = S.cube(0.25)
        return v, np.ascontiguousarray(f[2:])
    if name == "two_spheres":                              # overlapping: w = 2 in the lens
        v, f = _icosphere(2, 0.25)
        shift = np.array([0.1, 0.0, 0.0], F32)
        return np.concatenate([v - shift, v + shift]).astype(F32), np.concatenate([f, f + v.shape[0]]).astype(np.int32)
    if name == "lobed":
        from volsurfs_amd.mesh import stress_shells
        m = stress_shells(K=1, subdiv=4, device="cpu")[0]
        return m.vertices.numpy().astype(F32), m.faces.numpy().astype(np.int32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def queries(name):
    """[1536, 3] float32: 1 024 uniform points of [-0.5, 0.5]^3, then 512 face centroids (faces drawn with
    replacement) displaced by N(0, 0.004^2) per axis, all from default_rng(0)."""
    v, f = mesh(name)
    rng = np.random.default_rng(0)
    uniform = rng.uniform(-0.5, 0.5, (1024, 3))
    pick = rng.integers(0, f.shape[0], 512)
    centroids = v[f[pick].astype(np.int64)].astype(np.float64).mean(1)
    return np.concatenate([uniform, centroids + rng.normal(0.0, 0.004, (512, 3))]).astype(F32)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """[1536] float64: the brute-force winding number of `queries(name)`."""
    return S.winding_number(queries(name), *mesh(name))


def boundary_edges(faces):
    """The number of undirected edges that one face names."""
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, count = np.unique(e, axis=0, return_counts=True)
    return int((count == 1).sum())


# ---- the tree part of the rule, float64

def _words(qnodes, n):
    w = np.asarray(qnodes).view(np.uint32).reshape(-1, 8)[n, 6:8].astype(np.int64)
    return [int(x) - (1 << 32) if x >= (1 << 31) else int(x) for x in w]


def _leaf(word):
    code = ~word
    return code >> 4, code & 15


def _vertices(tris, slots):
    t = np.asarray(tris, np.float64).reshape(-1, 12)[slots]
    v0, e1, e2 = t[:, 0:3], t[:, 4:7], t[:, 8:11]
    return v0, e1, e2


def subtree_slots(qnodes, word):
    """The triangle slots under a child word, in the walk's order."""
    if word == EMPTY:
        return []
    if word < 0:
        first, cnt = _leaf(word)
        return list(range(first, first + cnt))
    w0, w1 = _words(qnodes, word)
    return subtree_slots(qnodes, w0) + subtree_slots(qnodes, w1)


def _stored(r):
    """r as the table stores it: (1 + 1e-6) r rounded up to float32."""
    x = F32(r * (1.0 + 1e-6))
    return float(np.nextafter(x, F32(np.inf)) if float(x) < r * (1.0 + 1e-6) else x)


def moments(qnodes, tris, roots):
    """{entry: (N [3], p [3], r)} in float64 by the rule: entry 2 n + c for child c of node n, 2 nr_nodes + m for the
    root of mesh m; plus, under the key ("sums", entry), (sum area centroid, sum area)."""
    nn = np.asarray(qnodes).reshape(-1, 8).shape[0]
    out = {}

    def centre(s, a, fallback):
        return s / a if a > 0 else fallback

    def visit(word, entry):
        if word == EMPTY:
            out[entry] = (np.zeros(3), np.zeros(3), 0.0)
            out[("sums", entry)] = (np.zeros(3), 0.0)
            return
        if word < 0:
            first, cnt = _leaf(word)
            v0, e1, e2 = _vertices(tris, np.arange(first, first + cnt))
            n = 0.5 * np.cross(e1, e2)
            area = np.linalg.norm(n, axis=1)
            s, a = (area[:, None] * (v0 + (e1 + e2) / 3.0)).sum(0), float(area.sum())
            p = centre(s, a, v0[0]).astype(F32).astype(np.float64)
            verts = np.concatenate([v0, v0 + e1, v0 + e2])
            out[entry] = (n.sum(0), p, _stored(np.linalg.norm(verts - p, axis=1).max()))
            out[("sums", entry)] = (s, a)
            return
        w = _words(qnodes, word)
        for c in (0, 1):
            visit(w[c], 2 * word + c)
        (n0, p0, r0), (n1, p1, r1) = out[2 * word], out[2 * word + 1]
        (s0, a0), (s1, a1) = out[("sums", 2 * word)], out[("sums", 2 * word + 1)]
        s, a = s0 + s1, a0 + a1
        p = centre(s, a, p0 if w[0] != EMPTY else p1).astype(F32).astype(np.float64)
        r = max([np.linalg.norm(p - pc) + rc for wc, pc, rc in ((w[0], p0, r0), (w[1], p1, r1)) if wc != EMPTY])
        out[entry] = (n0 + n1, p, _stored(r))
        out[("sums", entry)] = (s, a)

    for m, root in enumerate(roots):
        visit(int(root), 2 * nn + m)
    return out


def walk(qnodes, tris, table, root, root_entry, points, beta):
    """w [N] float64 of the walk over a table `moments` made (or the device's, as {entry: (N, p, r)})."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(pts.shape[0])

    def exact(slots, q):
        v0, e1, e2 = _vertices(tris, np.asarray(slots, np.int64))
        a = v0 - q
        b, c = a + e1, a + e2
        la, lb, lc = (np.linalg.norm(x, axis=1) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(1)
        den = la * lb * lc + (a * b).sum(1) * lc + (b * c).sum(1) * la + (c * a).sum(1) * lb
        return float((2.0 * np.arctan2(num, den)).sum())

    def visit(word, entry, q):
        if word == EMPTY:
            return 0.0
        n, p, r = table[entry]
        d = np.asarray(p, np.float64) - q
        L = float(np.sqrt(d @ d))
        with np.errstate(invalid="ignore"):
            far = L > beta * r
        if far:
            return float(d @ np.asarray(n, np.float64)) / L ** 3
        if word < 0:
            first, cnt = _leaf(word)
            return exact(range(first, first + cnt), q)
        w = _words(qnodes, word)
        return visit(w[0], 2 * word, q) + visit(w[1], 2 * word + 1, q)

    for i, q in enumerate(pts):
        out[i] = visit(int(root), root_entry, q) / (4.0 * np.pi)
    return out
