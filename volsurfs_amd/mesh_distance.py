"""How far one mesh is from another, on the device: closest-point queries over the shells' BVHs, an area-weighted surface
sampler, and the metrics on top (Chamfer, Hausdorff, precision / recall / F-score, the DTU names, shell clearance, the
simplifier's error).  The reference has no such stage: the rule is this library's own (include/volsurfs_hip.h "Mesh
distance"), restated in tests/mesh_distance_restated.py and unpinned.

A mesh is given as a cuda `TensorMesh` (a tracer is built for it with `builder="device"`, once per call) or as a pair
`(RayTracer, mesh_id)` of a tracer with q16 nodes that already holds it.

* `closest_points` / `closest_positions` — the closest point of a mesh to each query point (`RayTracer.closest`).
* `sample_surface` — n stratified, area-weighted samples of a mesh; a function of (mesh records, n, seed).
* `surface_distance` — the statistics of the distances from n samples of one mesh to another, in one fused launch
  (csrc/mesh_distance.hip): no sample and no distance reaches memory, one blocking read of twelve words.
* `mesh_distance`, `evaluate_mesh`, `shell_clearance`, `simplification_error` — both directions and the usual names.
* `point_cloud_mesh` — a scan as a mesh of zero-area faces, so that ground-truth point clouds take the same walk.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .mesh import TensorMesh
from .raytrace import RayTracer

MAX_THRESHOLDS = 8

DistanceStats = collections.namedtuple("DistanceStats", "n min mean rms max within")
DistanceStats.__doc__ = """Distances from n samples of one surface to another: smallest, mean, root mean square, largest,
and per threshold the number of samples within it (`within`, a tuple of ints)."""


WALK_BOUNDS = {"never": 0, "shallow": 1, "always": 2}


def set_walk_bounds(mode="shallow"):
    """Process-wide form of the walk's stack (vsa_closest_walk_config): does a pushed child keep its bound beside it?
    "shallow" (default): with the 24-entry stack of trees less than 24 deep, not with the 48-entry one; "never";
    "always".  The results do not depend on it; tools/mesh_distance_bench.py measures "never" and "always"."""
    if mode not in WALK_BOUNDS:
        raise ValueError(f"unknown mode {mode!r} (expected one of {tuple(WALK_BOUNDS)})")
    _lib.call("vsa_closest_walk_config", WALK_BOUNDS[mode])


def point_cloud_mesh(points, device="cuda"):
    """A point cloud [P, 3] as a TensorMesh whose face i is (i, i, i): every face has zero area, its record's closest
    point is the point itself, and `sample_surface` draws the points uniformly.  For the tracers of this module
    (`builder="device"`) and for `builder="ploc"`; the host builder's binned SAH is not meant for boxes without
    extent and is not offered here."""
    pts = torch.as_tensor(points, dtype=torch.float32)
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError(f"point_cloud_mesh: expected points [P, 3] with P >= 1, got {tuple(pts.shape)}")
    idx = torch.arange(pts.shape[0], dtype=torch.int32)
    return TensorMesh(pts, idx[:, None].expand(-1, 3).contiguous(), device=device)


def _resolve(mesh, what):
    """(tracer, mesh_id) of a mesh argument."""
    if isinstance(mesh, TensorMesh):
        if mesh.faces.shape[0] < 1:
            raise ValueError(f"{what}: the mesh has no faces")
        return RayTracer([mesh], builder="device"), 0
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2 and isinstance(mesh[0], RayTracer):
        tracer, mesh_id = mesh[0], int(mesh[1])
        tracer.require_q16(what, walk=False)     # (a source is only sampled; the walk's entry points check the depth)
        if not 0 <= mesh_id < tracer.nr_meshes:
            raise ValueError(f"{what}: mesh_id {mesh_id} outside 0..{tracer.nr_meshes - 1}")
        return tracer, mesh_id
    raise TypeError(f"{what}: expected a TensorMesh or (RayTracer, mesh_id), got {type(mesh).__name__}")


def _check_n(n, what):
    n = int(n)
    if n < 1:
        raise ValueError(f"{what}: n must be >= 1, got {n}")
    return n


def _area_prefix(handle):
    """Inclusive prefix [F] i64 of the integer area weights of a shell's leaf-ordered records (vsa_surface_area_prefix)."""
    tracer, mesh_id = handle
    first, nr = tracer.mesh_tri_offset[mesh_id], tracer.mesh_nr_tris[mesh_id]
    nbytes = _lib.workspace_bytes("vsa_surface_area_prefix_workspace_bytes", nr)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=tracer.device)
    prefix = torch.empty(nr, dtype=torch.int64, device=tracer.device)
    _lib.call("vsa_surface_area_prefix", tracer.tris, first, nr, ws, nbytes, prefix, _lib.stream_ptr())
    return prefix


@torch.no_grad()
def closest_points(points, mesh):
    """{dist [N], face [N] (original face ids), slot [N], bary [N, 2]} of the closest point of `mesh` to each of points
    [N, 3] f32 (cuda).  With a TensorMesh, `slot` indexes the records of a tracer that is gone when the call returns:
    pass (tracer, mesh_id) to use it."""
    tracer, mesh_id = _resolve(mesh, "closest_points")
    return tracer.closest(points, mesh_id)


@torch.no_grad()
def closest_positions(points, mesh):
    """[N, 3] f32: the points of `mesh` closest to `points`, (v0 + u e1) + v e2 of the closest record in fp32."""
    tracer, mesh_id = _resolve(mesh, "closest_positions")
    res = tracer.closest(points, mesh_id)
    rec = tracer.tris[res["slot"].clamp_min(0).long()]
    u, v = res["bary"][:, :1], res["bary"][:, 1:]
    return (rec[:, 0:3] + u * rec[:, 4:7]) + v * rec[:, 8:11]


def _sample(handle, prefix, n, seed):
    tracer, mesh_id = handle
    dev = tracer.device
    points = torch.empty(n, 3, device=dev)
    slot = torch.empty(n, dtype=torch.int32, device=dev)
    bary = torch.empty(n, 2, device=dev)
    _lib.call("vsa_surface_sample", tracer.tris, tracer.mesh_tri_offset[mesh_id], tracer.mesh_nr_tris[mesh_id], prefix,
              n, ctypes.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), points, slot, bary, _lib.stream_ptr())
    return points, slot, bary


@torch.no_grad()
def sample_surface(mesh, n, seed=0):
    """n stratified, area-weighted samples of `mesh`: (points [n, 3] f32, face [n] i64 original face ids, bary [n, 2] f32
    the weights of the face's second and third vertex).  Sample i sits at (i + xi) / n of the total area in the order of
    the tracer's leaf-ordered records, so a face of area a out of A receives n a / A samples to within one.  The same
    (mesh records, n, seed) give the same bytes."""
    handle = _resolve(mesh, "sample_surface")
    n = _check_n(n, "sample_surface")
    points, slot, bary = _sample(handle, _area_prefix(handle), n, seed)
    return points, handle[0].slot_face_id[slot.long()].long(), bary


def _thresholds(thresholds, what):
    th = [float(t) for t in thresholds]
    if len(th) > MAX_THRESHOLDS:
        raise ValueError(f"{what}: at most {MAX_THRESHOLDS} thresholds, got {len(th)}")
    if any(not t >= 0.0 for t in th):
        raise ValueError(f"{what}: thresholds must be >= 0, got {th}")
    return th


def _stats(n, lo, hi, s1, s2, within):
    return DistanceStats(n, float(lo), s1 / n, math.sqrt(s2 / n), float(hi), tuple(int(w) for w in within))


def _surface_distance(src, dst, n, seed, th):
    (ts, ms), (td, md) = src, dst
    dev = td.device
    prefix = _area_prefix(src)
    stats = torch.empty(12, dtype=torch.int64, device=dev)
    partials = torch.empty(2 * ((n + 63) // 64), dtype=torch.float64, device=dev)
    tau = (ctypes.c_float * max(len(th), 1))(*th)
    qnodes, tris, root, frame, _, depth = td.q16_tree_args(md)
    _lib.call("vsa_surface_distance", ts.tris, ts.mesh_tri_offset[ms], ts.mesh_nr_tris[ms], prefix, qnodes, tris, root[0],
              frame, depth, n, ctypes.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), tau, len(th), stats, partials,
              _lib.stream_ptr())
    w = stats.cpu().numpy()                                   # the one blocking read
    lo, hi = w[0:2].astype(np.uint32).view(np.float32)
    s1, s2 = w[2:4].view(np.float64)
    return _stats(n, lo, hi, float(s1), float(s2), w[4:4 + len(th)])


@torch.no_grad()
def surface_distance(src, dst, n=1_000_000, seed=0, thresholds=()):
    """DistanceStats of the distances from n samples of `src` (those of `sample_surface(src, n, seed)`) to the closest
    point of `dst`: one fused launch that makes the samples in registers, walks `dst` and reduces, then one blocking
    read.  min, max and `within` are exact (integer atomics); mean and rms come from fp64 sums added in a fixed
    order.  Thresholds are compared in fp32 (d <= float32(tau))."""
    n = _check_n(n, "surface_distance")
    th = _thresholds(thresholds, "surface_distance")
    return _surface_distance(_resolve(src, "surface_distance"), _resolve(dst, "surface_distance"), n, seed, th)


@torch.no_grad()
def surface_distance_unfused(src, dst, n=1_000_000, seed=0, thresholds=()):
    """The same statistics from the composition `sample_surface` + `closest_points` + torch reductions: samples and
    distances go through memory.  What `surface_distance` is measured against (tools/mesh_distance_bench.py); min, max
    and `within` are equal, mean and rms agree to the order of the fp64 sums."""
    n = _check_n(n, "surface_distance_unfused")
    th = _thresholds(thresholds, "surface_distance_unfused")
    src, (td, md) = _resolve(src, "surface_distance_unfused"), _resolve(dst, "surface_distance_unfused")
    points, _, _ = _sample(src, _area_prefix(src), n, seed)
    d = td.closest(points, md)["dist"]
    tau = torch.tensor(th, dtype=torch.float32, device=d.device)
    d64 = d.double()
    out = torch.cat([d.min()[None].double(), d.max()[None].double(), d64.sum()[None], (d64 * d64).sum()[None],
                     (d[None, :] <= tau[:, None]).sum(1).double()]).cpu().tolist()
    return _stats(n, out[0], out[1], out[2], out[3], out[4:])


def _f_score(p, r):
    return 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0


def _both_ways(a, b, n, seed, th):
    ab, ba = _surface_distance(a, b, n, seed, th), _surface_distance(b, a, n, seed, th)
    precision = [w / n for w in ab.within]
    recall = [w / n for w in ba.within]
    return {"ab": ab, "ba": ba, "chamfer": ab.mean + ba.mean, "hausdorff": max(ab.max, ba.max), "thresholds": list(th),
            "precision": precision, "recall": recall, "f_score": [_f_score(p, r) for p, r in zip(precision, recall)]}


@torch.no_grad()
def mesh_distance(a, b, n=1_000_000, seed=0, thresholds=()):
    """Both directions of `surface_distance`: {ab, ba (DistanceStats), chamfer = mean_ab + mean_ba, hausdorff =
    max(max_ab, max_ba) (of the samples), thresholds, and per threshold precision = the share of a's samples within it
    of b, recall = the share of b's samples within it of a, f_score = their harmonic mean (0 when both are 0)}."""
    n = _check_n(n, "mesh_distance")
    th = _thresholds(thresholds, "mesh_distance")
    return _both_ways(_resolve(a, "mesh_distance"), _resolve(b, "mesh_distance"), n, seed, th)


@torch.no_grad()
def evaluate_mesh(pred, gt, n=1_000_000, seed=0, thresholds=()):
    """`mesh_distance(pred, gt)` under the DTU names: accuracy = the mean distance pred -> gt, completeness = gt ->
    pred, overall = their mean; the other entries of `mesh_distance` beside them.  `gt` may be a scan through
    `point_cloud_mesh`."""
    res = mesh_distance(pred, gt, n, seed, thresholds)
    res.update(accuracy=res["ab"].mean, completeness=res["ba"].mean, overall=0.5 * (res["ab"].mean + res["ba"].mean))
    return res


@torch.no_grad()
def shell_clearance(meshes, n=1_000_000, seed=0):
    """For each consecutive pair of shells (k, k + 1) the DistanceStats both ways: a list of K - 1 dicts {pair, out
    (shell k -> k + 1), in (k + 1 -> k)}.  A `min` near 0 means the two shells touch or cross.  `meshes`: a list of
    TensorMeshes (one tracer is built for all of them) or a RayTracer."""
    n = _check_n(n, "shell_clearance")
    tracer = RayTracer.over(meshes)
    handles = [_resolve((tracer, k), "shell_clearance") for k in range(tracer.nr_meshes)]
    return [{"pair": (k, k + 1), "out": _surface_distance(handles[k], handles[k + 1], n, seed, []),
             "in": _surface_distance(handles[k + 1], handles[k], n, seed, [])} for k in range(tracer.nr_meshes - 1)]


@torch.no_grad()
def simplification_error(original, simplified, n=1_000_000, seed=0, thresholds=()):
    """`mesh_distance(original, simplified)` with every length also relative to the diagonal of the original's bounding
    box: the extra entries diagonal, chamfer_rel, hausdorff_rel, mean_ab_rel, mean_ba_rel, rms_ab_rel, rms_ba_rel,
    max_ab_rel, max_ba_rel."""
    n = _check_n(n, "simplification_error")
    th = _thresholds(thresholds, "simplification_error")
    a, b = _resolve(original, "simplification_error"), _resolve(simplified, "simplification_error")
    res = _both_ways(a, b, n, seed, th)
    tracer, mesh_id = a
    first, nr = tracer.mesh_tri_offset[mesh_id], tracer.mesh_nr_tris[mesh_id]
    rec = tracer.tris[first:first + nr]
    corners = torch.cat([rec[:, 0:3], rec[:, 0:3] + rec[:, 4:7], rec[:, 0:3] + rec[:, 8:11]])
    diag = float((corners.amax(0) - corners.amin(0)).double().norm())
    res["diagonal"] = diag
    for key in ("chamfer", "hausdorff"):
        res[key + "_rel"] = res[key] / diag
    for way in ("ab", "ba"):
        for field in ("mean", "rms", "max"):
            res[f"{field}_{way}_rel"] = getattr(res[way], field) / diag
    return res


__all__ = ["DistanceStats", "set_walk_bounds", "closest_points", "closest_positions", "sample_surface", "surface_distance",
           "surface_distance_unfused", "mesh_distance", "evaluate_mesh", "point_cloud_mesh", "shell_clearance",
           "simplification_error"]
