"""The mesh-cleaning rule (include/volsurfs_hip.h "Mesh cleaning") restated in numpy + scipy, written from
the rule and from no library's source: a sparse face graph from the sorted edge keys, components renumbered by their
minimum face, counts and float64 areas by bincount, the threshold, and the three removals.  The yardstick of
tests/test_mesh_clean.py; tested itself, without a GPU, by tests/test_mesh_clean_restated.py."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def edge_keys(faces, nr_verts):
    """[3F] int64 (min * V + max) of the corner pairs (0, 1), (1, 2), (2, 0), face-major, and the face of each."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = f.reshape(-1)
    b = f[:, [1, 2, 0]].reshape(-1)
    return np.minimum(a, b) * int(nr_verts) + np.maximum(a, b), np.repeat(np.arange(f.shape[0]), 3)


def triangle_clusters(faces, nr_verts):
    """(triangle_clusters [F] int32, C): components of "share an undirected edge", numbered by ascending minimum face."""
    F = np.asarray(faces).reshape(-1, 3).shape[0]
    if F == 0:
        return np.zeros(0, np.int32), 0
    key, face = edge_keys(faces, nr_verts)
    order = np.argsort(key, kind="stable")
    key, face = key[order], face[order]
    same = key[1:] == key[:-1]                       # neighbours in a run of equal keys: chaining joins the whole run
    g = coo_matrix((np.ones(int(same.sum()), np.int8), (face[:-1][same], face[1:][same])), shape=(F, F))
    C, label = connected_components(g, directed=False)
    first = np.full(C, F, np.int64)
    np.minimum.at(first, label, np.arange(F))        # the minimum face of every component
    number = np.empty(C, np.int64)
    number[np.argsort(first, kind="stable")] = np.arange(C)
    return number[label].astype(np.int32), int(C)


def face_areas(verts, faces):
    """[F] float64: 0.5 |(p1 - p0) x (p2 - p0)| in float64 from the float32 vertices."""
    p = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e1, e2 = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)


def area_bound(verts, faces, clusters, C):
    """[C] float64: F_c 2^-52 A_c + 8 2^-52 sum_f |e1| |e2|: a float64 sum of F_c positive terms in any order, plus the
    rounding of the cross product per face."""
    p = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e1, e2 = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
    ee = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    n = np.bincount(clusters, minlength=C).astype(np.float64)
    A = np.bincount(clusters, weights=face_areas(verts, faces), minlength=C)
    return n * 2.0 ** -52 * A + 8 * 2.0 ** -52 * np.bincount(clusters, weights=ee, minlength=C)


def cluster_connected_triangles(verts, faces):
    """(triangle_clusters [F] i32, cluster_n_triangles [C] i32, cluster_area [C] f64)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    cl, C = triangle_clusters(faces, verts.shape[0])
    n = np.bincount(cl, minlength=C).astype(np.int32)
    area = np.bincount(cl, weights=face_areas(verts, faces), minlength=C).astype(np.float64)
    return cl, n, area


def threshold(cluster_n_triangles, cluster_to_keep, min_cluster_faces=50):
    """max(the k-th largest count, min_cluster_faces), k = min(cluster_to_keep, C) (the departure from the reference,
    whose np.sort(...)[-cluster_to_keep] raises for C < cluster_to_keep)."""
    if cluster_to_keep < 1:
        raise ValueError("cluster_to_keep must be at least 1")
    n = np.sort(np.asarray(cluster_n_triangles))
    k = min(int(cluster_to_keep), n.shape[0])
    return max(int(n[-k]), int(min_cluster_faces))


def remove_triangles_by_mask(verts, faces, remove):
    """Open3D's meaning: the faces with remove[f] go, the rest keep their order; vertices untouched.  Also returns the
    kept faces' old indices."""
    keep = ~np.asarray(remove, bool)
    return np.asarray(verts), np.asarray(faces).reshape(-1, 3)[keep], np.nonzero(keep)[0]


def remove_unreferenced_vertices(verts, faces):
    """The vertices a face names, in their order with their bits; faces renumbered.  Also returns the kept vertices'
    old indices."""
    verts, faces = np.asarray(verts).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    used = np.zeros(verts.shape[0], bool)
    used[faces.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return verts[used], new[faces].astype(np.int32).reshape(-1, 3), np.nonzero(used)[0]


def remove_degenerate_triangles(verts, faces):
    """The faces that name a vertex twice go, the rest keep their order; vertices untouched.  Also returns the kept
    faces' indices."""
    f = np.asarray(faces).reshape(-1, 3)
    keep = ~((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0]))
    return np.asarray(verts), f[keep], np.nonzero(keep)[0]


def post_process_mesh(verts, faces, cluster_to_keep=1000, min_cluster_faces=50):
    """-> dict(vertices, faces, vertex_index [V_out] (old index of every kept vertex), face_index [F_out] (old index of
    every kept face), clusters, threshold, clusters_kept)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    if faces.shape[0] == 0:
        return {"vertices": verts[:0], "faces": faces, "vertex_index": np.zeros(0, np.int64),
                "face_index": np.zeros(0, np.int64), "clusters": 0, "threshold": 0, "clusters_kept": 0}
    cl, n, _ = cluster_connected_triangles(verts, faces)
    thr = threshold(n, cluster_to_keep, min_cluster_faces)
    v, f, fi = remove_triangles_by_mask(verts, faces, n[cl] < thr)
    v, f, vi = remove_unreferenced_vertices(v, f)
    v, f, keep = remove_degenerate_triangles(v, f)
    return {"vertices": v, "faces": f, "vertex_index": vi, "face_index": fi[keep], "clusters": int(n.shape[0]),
            "threshold": thr, "clusters_kept": int((n >= thr).sum())}


# ---- the shared test meshes

def seven_spheres():
    """Seven icospheres of subdivisions 4, 3, 2, 1, 1, 0, 0 and scales 0.5 .. 0.02 at the origin, sharing no vertex
    index; the 6 920 faces permuted with default_rng(0).  (vertices f32 [V, 3], faces i32 [F, 3])."""
    from volsurfs_amd.mesh import icosphere
    vs, fs, off = [], [], 0
    for sub, scale in zip((4, 3, 2, 1, 1, 0, 0), (0.5, 0.3, 0.1, 0.05, 0.04, 0.02, 0.02)):
        v, f = icosphere(sub, scale)
        vs.append(v)
        fs.append(f + off)
        off += v.shape[0]
    v, f = np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)
    return v, f[np.random.default_rng(0).permutation(f.shape[0])]


def corner_cases():
    """Hand-built adjacency cases: {name: (vertices, faces, expected triangle_clusters)}."""
    rng = np.random.default_rng(1)
    P = lambda n: rng.standard_normal((n, 3)).astype(np.float32)
    cases = {}
    # two fans of three faces around vertex 0 that share nothing but the apex
    cases["two_fans_share_apex"] = (P(9), [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 5, 6], [0, 6, 7], [0, 7, 8]],
                                    [0, 0, 0, 1, 1, 1])
    cases["three_faces_on_one_edge"] = (P(5), [[0, 1, 2], [1, 0, 3], [0, 1, 4]], [0, 0, 0])
    cases["duplicated_face"] = (P(6), [[0, 1, 2], [3, 4, 5], [0, 1, 2]], [0, 1, 0])
    # face 1 = (a, a, b) with a = 1, b = 2 joins face 0 across (1, 2); face 2 is apart
    cases["twice_named_vertex"] = (P(7), [[0, 1, 2], [1, 1, 2], [4, 5, 6]], [0, 0, 1])
    cases["isolated_triangle"] = (P(3), [[0, 1, 2]], [0])
    # vertices 0, 4 and 9 are named by no face; cluster numbers follow the minimum face, not the vertex order
    cases["unreferenced_vertices"] = (P(10), [[7, 8, 6], [1, 2, 3], [3, 2, 5], [6, 8, 5]], [0, 1, 1, 0])
    return {k: (v, np.asarray(f, np.int32), np.asarray(c, np.int32)) for k, (v, f, c) in cases.items()}


def blob_field(n, seed=0, nr_blobs=40, ball_radius=0.55):
    """A float32 grid [n, n, n] on [-1, 1]^3 whose level 0 (inside below) is one ball of radius `ball_radius` and `nr_blobs`
    small balls outside it, radii from 0.2 to 12 voxels of an n = 128 lattice (twice that at n = 256), at least three
    such voxels apart from the ball and from each other.  Returns (grid, origin, spacing, big, centres) with `big` the
    large ball's own grid and `centres` the (centre, radius) of every blob placed."""
    rng = np.random.default_rng(seed)
    ax = np.linspace(-1.0, 1.0, n).astype(np.float32)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    big = (np.sqrt(X * X + Y * Y + Z * Z) - np.float32(ball_radius)).astype(np.float32)
    grid = big.copy()
    voxel = 2.0 / 127
    radii = np.exp(rng.uniform(np.log(0.2 * voxel), np.log(12 * voxel), nr_blobs))
    radii[0] = 0.2 * voxel
    centres = []
    for r in radii:
        for _ in range(1000):
            c = rng.uniform(-0.95 + r, 0.95 - r, 3)
            if np.linalg.norm(c) - r < ball_radius + 3 * voxel:
                continue
            if all(np.linalg.norm(c - c2) > r + r2 + 3 * voxel for c2, r2 in centres):
                break
        else:
            continue
        centres.append((c, r))
        d = np.sqrt((X - np.float32(c[0])) ** 2 + (Y - np.float32(c[1])) ** 2 + (Z - np.float32(c[2])) ** 2)
        np.minimum(grid, (d - np.float32(r)).astype(np.float32), out=grid)
    return grid, [-1.0] * 3, [2.0 / (n - 1)] * 3, big, centres
