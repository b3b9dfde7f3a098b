"""Which faces of two meshes cross, exactly: a triangle-triangle rule in fp64 over a box-overlap walk of the shells' BVHs
(csrc/mesh_cross.hip, csrc/cross_walk.h).  The reference has no such stage: the rule is this library's own
(include/volsurfs_hip.h "Mesh crossings"), restated in tests/mesh_intersect_restated.py and unpinned.  Where
`mesh_sdf.shell_nesting` and `mesh_distance.shell_clearance` sample, these functions decide every pair of faces.

Two faces CROSS when an edge of one passes through the other: its end points lie strictly on opposite sides of the
other's plane and the edge passes inside (or through the border of) the other triangle.  Faces that share a vertex by
equal coordinates have side exactly 0 there: neighbours in a mesh never cross, and a triangle soup gives what its welded
mesh gives.  Coplanar overlap, touching without passing through, duplicate and zero-area faces are not crossings; a
face with a NaN coordinate crosses nothing.

A mesh is given as a cuda `TensorMesh` or as a pair `(RayTracer, mesh_id)` of a tracer with q16 nodes that already
holds it, as in `mesh_distance`.  The mesh whose tree is walked needs a tracer (one is built with `builder="device"`
when a TensorMesh is given); the query mesh needs none, but when it sits in a tracer its faces are taken in that
tracer's leaf order, so that the lanes of a wave hold nearby faces.  The results do not depend on that.

* `mesh_crossings(a, b)` — the crossing pairs (face of a, face of b), the counts per face, optionally the segments.
* `self_crossings(mesh)` — the pairs i < j of one mesh's faces.
* `crossing_stats(a, b)` — the count pass alone.
* `shell_crossings`, `shells_nested`, `check_shells` — the same for the consecutive shells of a stack.
"""
import collections

import torch

from . import _lib
from .mesh import TensorMesh
from .mesh_distance import _resolve
from .raytrace import RayTracer

MAX_PAIRS = 0x7FFFFFFF


def _length(self):
    """The fp64 sum of the segments' lengths (torch): the length of the crossing curve where exactly two edges pierce
    per pair.  Needs `segments=True`."""
    if self.segments is None:
        raise ValueError("length() needs the segments: call with segments=True")
    d = self.segments[:, 1] - self.segments[:, 0]
    return float((d * d).sum(1).sqrt().sum())


class Crossings(collections.namedtuple("Crossings", "pairs count_a count_b segments")):
    """pairs [P, 2] int64 (face of a, face of b) sorted ascending by (face_a, face_b); count_a [Fa] int32 = the faces of
    b each face of a crosses, count_b [Fb] int32 the reverse (both sum to P); segments [P, 2, 3] float64 or None."""
    __slots__ = ()
    length = _length


class SelfCrossings(collections.namedtuple("SelfCrossings", "pairs count segments")):
    """pairs [P, 2] int64 with i < j, sorted ascending; count [F] int32 = the partners of each face (sums to 2 P);
    segments [P, 2, 3] float64 (face i as A) or None."""
    __slots__ = ()
    length = _length


def arrays_of(mesh, device, what):
    """(vertices [V, 3] f32, faces [F, 3] i32) of a TensorMesh, contiguous on `device`."""
    v = mesh.vertices.detach().to(device, torch.float32).contiguous()
    f = mesh.faces.detach().to(device, torch.int32).contiguous()
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or v.shape[0] < 1 or f.shape[0] < 1:
        raise ValueError(f"{what}: expected vertices [V, 3] and faces [F, 3] with V, F >= 1, got {tuple(v.shape)} / "
                         f"{tuple(f.shape)}")
    return v, f


def tree_of(mesh, what):
    """(tracer, mesh_id, vertices, faces) of the mesh whose tree is walked."""
    tracer, mesh_id = _resolve(mesh, what)
    tracer.require_q16(what)
    return (tracer, mesh_id) + arrays_of(tracer._meshes[mesh_id], tracer.device, what)


def _query(mesh, device, what):
    """(vertices, faces, order or None) of the query mesh: a TensorMesh in input order, a tracer's mesh in leaf order."""
    if isinstance(mesh, TensorMesh):
        if not mesh.vertices.is_cuda:
            raise ValueError(f"{what}: the mesh must be on cuda, got {mesh.vertices.device}")
        return arrays_of(mesh, device, what) + (None,)
    tracer, mesh_id = _resolve(mesh, what)
    return arrays_of(tracer._meshes[mesh_id], device, what) + (leaf_order(tracer, mesh_id),)


def leaf_order(tracer, mesh_id):
    """The face ids of the tracer's mesh `mesh_id` in the order of its tree's leaf slots."""
    first, nr = tracer.mesh_tri_offset[mesh_id], tracer.mesh_nr_tris[mesh_id]
    return tracer.slot_face_id[first:first + nr].contiguous()


def cross_passes(tree, query, self_mode, segments, emit, max_depth=None):
    """The two passes.  Returns (pairs or None, count_query, count_tree or None, segments or None, P)."""
    tracer, mesh_id, tv, tf = tree
    qv, qf, order = query
    dev = tracer.device
    qnodes, tris, root, frame, _, depth = tracer.q16_tree_args(mesh_id)
    depth = depth if max_depth is None else int(max_depth)
    Fq, Ft = qf.shape[0], tf.shape[0]
    if order is not None and order.shape[0] != Fq:
        raise _lib.VolsurfsHipError(f"the tracer holds {order.shape[0]} faces of a mesh of {Fq}")
    mesh_args = (qnodes, tris, root[0], frame, depth, tv, tv.shape[0], tf, Ft, qv, qv.shape[0], qf, Fq, order,
                 int(bool(self_mode)))
    nbytes = _lib.workspace_bytes("vsa_mesh_cross_workspace_bytes", Fq, 0, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    count_q = torch.empty(Fq, dtype=torch.int32, device=dev)
    count_t = None if self_mode else torch.empty(Ft, dtype=torch.int32, device=dev)
    offsets = torch.empty(Fq, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    st = _lib.stream_ptr()
    _lib.call("vsa_mesh_cross_count", *mesh_args, count_q, count_t, offsets, total, ws, nbytes, st)
    if not emit:
        return None, count_q, count_t, None, total
    P = int(total.item())                                         # the one blocking read
    if P > MAX_PAIRS:
        raise _lib.VolsurfsHipError(f"{P} crossing pairs: more than {MAX_PAIRS}")
    pairs = torch.empty(P, 2, dtype=torch.int64, device=dev)
    segs = torch.empty(P, 2, 3, dtype=torch.float64, device=dev) if segments else None
    if P > 0:
        nbytes = _lib.workspace_bytes("vsa_mesh_cross_workspace_bytes", Fq, P, int(bool(segments)))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.call("vsa_mesh_cross_emit", *mesh_args, offsets, P, pairs, segs, ws, nbytes, st)
    return pairs, count_q, count_t, segs, P


@torch.no_grad()
def mesh_crossings(a, b, segments=False):
    """`Crossings` of the faces of `a` against the faces of `b` (the tree walked is b's): a count pass, one blocking read
    of the number of pairs, an emit pass, a sort.  The same meshes give the same bytes whatever b's builder."""
    tree = tree_of(b, "mesh_crossings")
    pairs, ca, cb, segs, _ = cross_passes(tree, _query(a, tree[0].device, "mesh_crossings"), False, segments, True)
    return Crossings(pairs, ca, cb, segs)


@torch.no_grad()
def self_crossings(mesh, segments=False):
    """`SelfCrossings` of one mesh: the pairs i < j of its faces that cross, each evaluated with face i as A."""
    tracer, mesh_id, v, f = tree = tree_of(mesh, "self_crossings")
    pairs, count, _, segs, _ = cross_passes(tree, (v, f, leaf_order(tracer, mesh_id)), True, segments, True)
    return SelfCrossings(pairs, count, segs)


def _stats(count_q, count_t, total):
    w = torch.stack([total[0], (count_q > 0).sum(), (count_t > 0).sum()]).cpu().tolist()
    return int(w[0]), int(w[1]), int(w[2])


@torch.no_grad()
def crossing_stats(a, b):
    """(pairs, faces_a, faces_b): the number of crossing pairs, of faces of a that cross b and of faces of b that cross
    a, from the count pass alone: nothing is emitted or sorted."""
    tree = tree_of(b, "crossing_stats")
    _, ca, cb, _, total = cross_passes(tree, _query(a, tree[0].device, "crossing_stats"), False, False, False)
    return _stats(ca, cb, total)


@torch.no_grad()
def shell_crossings(meshes):
    """For each consecutive pair of shells (k, k + 1): {pair, pairs = the crossing face pairs, faces_inner = the faces
    of shell k that cross shell k + 1, faces_outer = the reverse}, from the count pass.  `meshes`: a list of
    TensorMeshes (one tracer is built for all of them) or a RayTracer."""
    tracer = RayTracer.over(meshes)
    out = []
    for k in range(tracer.nr_meshes - 1):
        pairs, inner, outer = crossing_stats((tracer, k), (tracer, k + 1))
        out.append({"pair": (k, k + 1), "pairs": pairs, "faces_inner": inner, "faces_outer": outer})
    return out


@torch.no_grad()
def shells_nested(meshes, sign="pseudonormal"):
    """Is every shell inside the next one?  A list of K - 1 bools, one per consecutive pair (k, k + 1): True iff no
    face of shell k crosses a face of shell k + 1 and one vertex of every edge-connected component of shell k
    (`mesh_clean.cluster_connected_triangles`) has a negative signed distance to shell k + 1
    (`RayTracer.signed_distance(.., sign=sign)`).

    What it proves: for a closed shell k + 1, a connected piece of surface that nowhere passes through it lies on one
    side of it, so one vertex inside puts the whole component inside (its closure: it may touch).  Unlike
    `mesh_sdf.shell_nesting`, no crossing is too small to be seen.  What the rule does not see: shells that touch or
    overlap in a common plane without passing through, a passage exactly through a vertex whose side rounds to 0, and
    the self-crossings of either shell (`self_crossings`); for a shell k + 1 that is not closed the sign is whatever
    `sign` gives and "inside" means no more than that."""
    from .mesh_clean import cluster_connected_triangles
    tracer = RayTracer.over(meshes)
    tracer.sign_rule(sign)
    out = []
    for k in range(tracer.nr_meshes - 1):
        pairs, _, _ = crossing_stats((tracer, k), (tracer, k + 1))
        if pairs:
            out.append(False)
            continue
        v, f = arrays_of(tracer._meshes[k], tracer.device, "shells_nested")
        clusters, sizes, _ = cluster_connected_triangles(TensorMesh(v, f, device=tracer.device))
        first = torch.full((sizes.shape[0],), f.shape[0], dtype=torch.int64, device=tracer.device)
        first.scatter_reduce_(0, clusters.long(), torch.arange(f.shape[0], device=tracer.device), "amin")
        points = v[f[first, 0].long()]
        d = tracer.signed_distance(points, k + 1, sign=sign)["dist"]
        out.append(bool((d < 0).all()))
    return out


@torch.no_grad()
def check_shells(meshes_dir, sign="pseudonormal"):
    """A `meshes*/` directory of `<level>.ply` / `.obj` shells, sorted by level as `VolSurfs.from_meshes_path` sorts
    them: {files, self_crossings = the crossing pairs i < j of each shell, crossings = `shell_crossings`, nested =
    `shells_nested`}."""
    from .mesh import load_meshes_indexed_from_path
    from .shell_stack import self_crossing_count                  # (shell_stack is built on this module)
    meshes, paths = load_meshes_indexed_from_path(None, meshes_dir, return_paths=True)
    tracer = RayTracer(meshes, builder="device")
    selfs = [self_crossing_count(tracer, k) for k in range(tracer.nr_meshes)]
    return {"files": paths, "self_crossings": [int(t) for t in torch.cat(selfs).cpu().tolist()],
            "crossings": shell_crossings(tracer), "nested": shells_nested(tracer, sign=sign)}


_arrays, _tree, _leaf_order, _cross = arrays_of, tree_of, leaf_order, cross_passes           # (tests call these names)

__all__ = ["Crossings", "SelfCrossings", "mesh_crossings", "self_crossings", "crossing_stats", "shell_crossings",
           "shells_nested", "check_shells", "arrays_of", "tree_of", "leaf_order", "cross_passes"]
