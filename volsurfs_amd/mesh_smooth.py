"""Smooth shells on the device: Taubin's lambda | mu fairing that moves vertices, and only vertices, and keeps a stack of
shells nested (csrc/mesh_smooth.hip).  Marching cubes of a hash-grid field leaves voxel-scale noise on the surface; box
projection cuts it into thousands of small charts and the quadric simplifier spends its faces on it.
The reference never smooths: the rule is this library's own (include/volsurfs_hip.h "Mesh smoothing"),
restated in tests/mesh_smooth_restated.py and unpinned.

Everything is fp32 in this order.  The ring of a vertex v is the corner slots 3 f + c with faces[f, c] == v in
ascending slot order (a face that names v twice is in it twice).  A vertex is a boundary vertex when it is an endpoint
of an undirected edge that occurs exactly once among the 3 F corner-to-next-corner edges; with `fix_boundary` boundary
vertices never move, and a vertex no face names never moves.

* A half-step with weight w: for every vertex that may move, acc = 0, then per ring slot in order acc = (acc + P[a]) +
  P[b] with a, b the face's next two corners; cen = acc / float(2 slots); Q[v] = P[v] + w (cen - P[v]).  A Q[v] that is
  not finite is dropped: the vertex keeps P[v] and counts as stuck.  All vertices read P and write Q.
* One iteration is a half-step with `lam`, then one with `mu` on its result; mu = 0 is plain Laplacian smoothing, which
  shrinks; the default mu = -0.53 undoes the shrinkage.
* The guard, once per iteration, with P the positions before it and Q after it: a face is bad when one of its vertices
  differs in bits from P and it crosses a face of a guard (`mesh_intersect`'s exact rule); every vertex of a bad face
  that still differs from P is put back to its bits in P (reverted); the rounds repeat until one reverts nothing.  One
  blocking read per round.

After an iteration every face that crosses a guard face has all three vertices where they were before it: the crossing
pairs of the output with a guard are a subset of the input's, and a shell that crossed nothing crosses nothing.  Always:
faces, UVs, vertex count and vertex order are unchanged (atlases and trained textures stay valid, trees are `refit`,
never rebuilt); `iterations=0`, or a mesh where nothing may move, comes back with the same bits; the same input gives
the same bytes on every call and for every builder of the guards' trees.  NOT promised, but reported: that the shell
does not cross itself (self_crossings_after), anything about shells that are not guards.

* `smooth_mesh(mesh, guards=...)` — one mesh, unguarded (2 x iterations launches, no read until the statistics) or
  against 1..4 guard meshes.
* `smooth_shells(meshes)` — a stack in `shell_stack.stack_order`'s order: the anchor against its two input neighbours, then
  outward and inward, each shell against its already smoothed neighbour and its other input neighbour, so the crossing
  pairs of two consecutive outputs are a subset of the input's.
* `smooth_meshes(meshes_dir, out_dir)` — a `meshes*/` directory into the same names and formats.  The pipeline order is
  `clean_meshes` -> `smooth_meshes` -> `cull_meshes` -> `simplify_meshes_nested` -> (`untangle_meshes`) ->
  `compute_meshes_atlas`; it may also run after the atlas, since only vertices move.
"""
import collections
import math
import numbers

import torch

from . import _lib
from .mesh import TensorMesh
from .mesh_intersect import check_shells
from .raytrace import RayTracer
from .shell_stack import (MAX_GUARDS, StackReports, check_stack, displacement, guard_block, load_shell_dir,
                          resolve_guards, save_shell_dir, self_crossing_count, stack_order, with_vertices)

SmoothReport = collections.namedtuple(
    "SmoothReport", "shell guards iterations moved_vertices max_displacement boundary_vertices stuck reverted "
                    "guard_rounds self_crossings_after")
SmoothReport.__doc__ = """One mesh of `smooth_mesh` / `smooth_shells`: shell = its index in the stack (0 for one mesh),
guards = the meshes it was guarded by, lower shell first, as ("in", k) = input shell k or ("out", k) = the already
smoothed shell k (for `smooth_mesh`: ("guard", i)); iterations as asked; moved_vertices = the vertices whose bits
changed; max_displacement = the largest distance of a moved vertex from its input position (fp64 of the fp32
coordinates); boundary_vertices = the boundary vertices, fixed or not; stuck = the (half-step, vertex) results dropped
because they were not finite, summed over all half-steps; reverted = the vertices the guard put back, summed over the
iterations; guard_rounds = the guard's rounds, summed (each iteration's last round reverts nothing);
self_crossings_after = the crossing pairs i < j of the output's own faces (None where the output holds a vertex that is
not finite: no tree is built over such a mesh)."""


class SmoothReports(StackReports):
    """The K `SmoothReport`s of `smooth_shells`, inner to outer, with the stack's own figures: crossings_in /
    crossings_out = the crossing face pairs of every consecutive pair (k, k + 1) of the inputs / of the outputs
    (`mesh_intersect.shell_crossings`), nested = `mesh_intersect.shells_nested` of the outputs."""


def workspace_bytes(nr_verts, nr_faces):
    """Device workspace of one smoothing of a mesh with `nr_verts` vertices and `nr_faces` faces."""
    return _lib.workspace_bytes("vsa_mesh_smooth_workspace_bytes", int(nr_verts), int(nr_faces))


def _check_rule(iterations, lam, mu):
    if isinstance(iterations, bool) or not isinstance(iterations, numbers.Integral) or iterations < 0:
        raise ValueError(f"smooth: iterations must be an integer >= 0, got {iterations!r}")
    iterations, lam, mu = int(iterations), float(lam), float(mu)
    if not 0.0 < lam <= 1.0:
        raise ValueError(f"smooth: lam must lie in (0, 1], got {lam}")
    if not (mu <= 0.0 and math.isfinite(mu)):
        raise ValueError(f"smooth: mu must be a finite number <= 0, got {mu}")
    return iterations, lam, mu


def _check_mesh(mesh, what):
    """(vertices f32 [V, 3], faces i32 [F, 3]) of the mesh to smooth, contiguous on cuda and in range.  Vertices that
    are not finite are the rule's business (stuck), not an error."""
    if not isinstance(mesh, TensorMesh):
        raise TypeError(f"{what}: expected a TensorMesh, got {type(mesh).__name__}")
    v, f = mesh.vertices, mesh.faces
    if not (v.is_cuda and f.is_cuda):
        raise ValueError(f"{what}: the mesh must be on cuda, got {v.device} / {f.device}")
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or v.shape[0] < 1 or f.shape[0] < 1:
        raise ValueError(f"{what}: expected vertices [V, 3] and faces [F, 3] with V, F >= 1, got {tuple(v.shape)} / "
                         f"{tuple(f.shape)}")
    v = v.detach().to(torch.float32).contiguous()
    f = f.detach().to(torch.int32).contiguous()
    lo, hi = torch.aminmax(f)
    if int(lo) < 0 or int(hi) >= v.shape[0]:
        raise _lib.VolsurfsHipError(f"{what}: face indices out of range [0, {v.shape[0]}): min {int(lo)}, max {int(hi)}")
    return v, f


@torch.no_grad()
def _smooth(v0, f, iterations, lam, mu, fix_boundary, block, log=None):
    """The launches: (vertices, {moved_vertices, max_displacement, boundary_vertices, stuck, reverted, guard_rounds,
    finite}) of the checked arrays (v0, f) against the guards of `block` (`shell_stack.guard_block`) or None."""
    dev = v0.device
    V, F = v0.shape[0], f.shape[0]
    nbytes = workspace_bytes(V, F)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    state = torch.zeros(2, dtype=torch.int64, device=dev)         # stuck, reverted
    st = _lib.stream_ptr()
    _lib.call("vsa_mesh_smooth_prepare", f, V, F, ws, nbytes, st)
    guard_args, _ = block or (None, None)                         # (its second entry keeps the trees alive)
    cur, mid, new = v0, torch.empty_like(v0), torch.empty_like(v0)
    fixed = int(bool(fix_boundary))
    rnd = reverted = rounds = 0
    for _ in range(iterations):
        _lib.call("vsa_mesh_smooth_step", cur, mid, f, V, F, 0, lam, fixed, ws, nbytes, state, st)
        _lib.call("vsa_mesh_smooth_step", mid, new, f, V, F, 1, mu, fixed, ws, nbytes, state, st)
        back, n, first = 0, 0, rnd
        while guard_args is not None:
            _lib.call("vsa_mesh_smooth_guard", cur, new, f, V, F, *guard_args, first, rnd, ws, nbytes, st)
            _lib.call("vsa_mesh_smooth_revert", cur, new, V, F, rnd, ws, nbytes, state[1:], st)
            total = int(state[1].item())                          # the round's one blocking read
            rnd, n = rnd + 1, n + 1
            if total == reverted + back:
                break
            back = total - reverted
        reverted, rounds = reverted + back, rounds + n
        if log is not None:
            log.append((back, n))
        cur, new = new, (torch.empty_like(v0) if cur is v0 else cur)
    changed, disp = displacement(cur, v0)
    boundary = ws[:4 * V].view(torch.int32)
    s = torch.stack([changed.sum().double(), disp.max(), boundary.sum().double(), state[0].double(),
                     torch.isfinite(cur).all().double()]).cpu().tolist()
    out = cur.clone() if cur is v0 else cur
    return out, {"moved_vertices": int(s[0]), "max_displacement": float(s[1]), "boundary_vertices": int(s[2]),
                 "stuck": int(s[3]), "reverted": reverted, "guard_rounds": rounds, "finite": bool(s[4])}


def _self_count(tracer, mesh_id):
    return int(self_crossing_count(tracer, mesh_id).item())


def _report(shell, names, iterations, st, selfs):
    return SmoothReport(shell, tuple(names), iterations, st["moved_vertices"], st["max_displacement"],
                        st["boundary_vertices"], st["stuck"], st["reverted"], st["guard_rounds"], selfs)


def smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, guards=None, log=None):
    """(TensorMesh, SmoothReport): the cuda TensorMesh `mesh` after `iterations` Taubin iterations by the module's rule.
    The output carries the input's faces, UVs, `has_uvs` and `vertex_colors`; the input's tensors are not written.

    guards: None or [] (the unguarded path) or 1..4 meshes, each a cuda TensorMesh (it gets a
    RayTracer(builder="device") of its own) or a pair (RayTracer, mesh_id) of a tracer with q16 nodes: after every
    iteration, no face that moved crosses a face of a guard.  `log` (a list) takes one (reverted, guard rounds) per
    iteration.  Argument errors raise before any HIP call."""
    iterations, lam, mu = _check_rule(iterations, lam, mu)
    if guards is not None and len(guards) > MAX_GUARDS:
        raise ValueError(f"smooth_mesh: 1..{MAX_GUARDS} guards, got {len(guards)}")
    v0, f = _check_mesh(mesh, "smooth_mesh")
    resolved = resolve_guards(guards, "smooth_mesh") if guards is not None and len(guards) else None
    block = guard_block(resolved, "smooth_mesh") if resolved else None
    v, st = _smooth(v0, f, iterations, lam, mu, fix_boundary, block, log)
    out = with_vertices(mesh, v)
    selfs = _self_count(RayTracer([out], builder="device"), 0) if st["finite"] else None
    names = [("guard", i) for i in range(len(resolved or ()))]
    return out, _report(0, names, iterations, st, selfs)


@torch.no_grad()
def smooth_shells(meshes, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, anchor=None, builder="device"):
    """(meshes, reports): the K >= 2 shells `meshes` (inner to outer, cuda TensorMeshes) each smoothed under the guard
    of its neighbours, in `shell_stack.stack_order`'s order: the anchor (default K // 2) against the input shells anchor - 1
    and anchor + 1; then outward, shell k against the already smoothed shell k - 1 and the input shell k + 1 (if there is
    one); then inward, mirrored.  Two tracers are built with `builder`, one over the inputs and one that is refit, never
    rebuilt, as the shells are smoothed; the result does not depend on the builder.

    For every consecutive pair the crossing face pairs of the outputs are a subset of the inputs': a stack that comes in
    without crossings goes out without.  `reports` is a `SmoothReports`: one `SmoothReport` per shell, and crossings_in,
    crossings_out and nested of the stack.  Argument errors raise before any HIP call."""
    iterations, lam, mu = _check_rule(iterations, lam, mu)
    meshes, K, anchor = check_stack(meshes, anchor, builder, "smooth_shells")
    arrays = [_check_mesh(m, f"smooth_shells: shell {k}") for k, m in enumerate(meshes)]
    inputs = RayTracer(meshes, builder=builder)
    done = RayTracer(meshes, builder=builder)                     # refit shell by shell: ("out", k) is its shell k
    out, stats = list(meshes), [None] * K
    for k, names in stack_order(K, anchor):
        guards = [(inputs if which == "in" else done, g) for which, g in names]
        v, stats[k] = _smooth(*arrays[k], iterations, lam, mu, fix_boundary, guard_block(guards, "smooth_shells"))
        stats[k]["guards"] = names
        out[k] = with_vertices(meshes[k], v)
        done.refit(out)
    reports = SmoothReports(
        _report(k, st["guards"], iterations, st, _self_count(done, k) if st["finite"] else None)
        for k, st in enumerate(stats))
    return out, reports.fill(inputs, done)


def smooth_meshes(meshes_dir, out_dir, **kw):
    """`smooth_shells` of a `meshes*/` directory (`<level>.ply` / `.obj`, sorted by level as
    `VolSurfs.from_meshes_path` sorts them) into `out_dir` under the same names and in the same formats, exactly as
    `untangle_meshes` keeps them: an OBJ its per-corner UVs, a PLY its wedge UVs, its vertex colours and its ascii /
    binary form.  Returns (reports, `check_shells(out_dir)`).  It sits between `clean_meshes` and `cull_meshes`; it may
    also run after `compute_meshes_atlas`: only vertices move, so the atlas stays valid."""
    names, meshes, colors = load_shell_dir(meshes_dir)
    out, reports = smooth_shells(meshes, **kw)
    save_shell_dir(meshes_dir, out_dir, names, out, colors)
    return reports, check_shells(out_dir)


__all__ = ["SmoothReport", "SmoothReports", "smooth_mesh", "smooth_shells", "smooth_meshes", "workspace_bytes"]
