"""A sign for meshes that are not closed, on the device: the generalised winding number of a mesh and the census of its
edges.  The reference has no such stage: the rule is this library's own (include/volsurfs_hip.h "Mesh winding number",
DESIGN §31), unpinned; the exact sum is restated in float64 in tests/mesh_sdf_restated.py.

w(q) = sum over the faces of the signed solid angle / 4 pi is about 1 inside and about 0 outside a mesh whose faces wind
outward.  Unlike the pseudonormal sign of `mesh_sdf` it degrades gracefully: across a hole it passes smoothly from one to
the other, and where parts overlap it counts them.  `mesh_sdf`'s entry points take it as their sign with
`sign="winding"` (inside iff w > 1/2) or, for the meshes whose `edge_census` finds anything, with `sign="auto"`.

A mesh is a cuda `TensorMesh` or a pair `(RayTracer, mesh_id)`, as in `mesh_distance`.

* `winding_number` — w per point, raw, so that a caller can threshold differently.
* `edge_census`, `is_closed` — boundary, non-manifold and inconsistently wound edges (csrc/mesh_winding.hip:
  vsa_mesh_edge_census).
"""
import ctypes

import torch

from . import _lib
from .mesh import TensorMesh, check_mesh
from .mesh_distance import _resolve
from .raytrace import RayTracer

CENSUS = ("boundary", "non_manifold", "inconsistent")


@torch.no_grad()
def winding_number(points, mesh, beta=2.0):
    """w [N] f32 of points [N, 3] f32 (cuda) for `mesh` (`RayTracer.winding_number`): subtrees of the mesh's BVH farther
    than `beta` times their radius are taken by their area vector; beta > 1, math.inf sums every triangle exactly."""
    tracer, mesh_id = _resolve(mesh, "winding_number")
    return tracer.winding_number(points, mesh_id, beta)


@torch.no_grad()
def edge_census(mesh, device=None):
    """{boundary, non_manifold, inconsistent}: the number of undirected edges with one face, with more than two, and
    with two faces that traverse them in the same direction, over the faces with a positive area (a zero-area face
    counts nowhere, as in the pseudonormal tables).  All zero: a closed, consistently wound manifold.  One blocking
    read."""
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2 and isinstance(mesh[0], RayTracer):
        tracer, mesh_id = _resolve(mesh, "edge_census")
        return dict(tracer.edge_census(mesh_id))
    if device is not None and mesh.vertices.device != torch.device(device):
        mesh = TensorMesh(mesh.vertices, mesh.faces, None, device=device)
    V, F = check_mesh(mesh, "edge_census")
    if F.shape[0] < 1:
        raise ValueError("edge_census: the mesh has no faces")
    nbytes = _lib.workspace_bytes("vsa_mesh_edge_census_workspace_bytes", V.shape[0], F.shape[0])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=V.device)
    counts = (ctypes.c_longlong * 3)()
    _lib.call("vsa_mesh_edge_census", V, V.shape[0], F, F.shape[0], ws, nbytes, ctypes.cast(counts, ctypes.c_void_p),
              _lib.stream_ptr())
    return {k: int(counts[i]) for i, k in enumerate(CENSUS)}


def is_closed(mesh):
    """True when `edge_census` finds nothing: the pseudonormal sign means inside / outside for this mesh."""
    return not any(edge_census(mesh).values())


__all__ = ["CENSUS", "winding_number", "edge_census", "is_closed"]
