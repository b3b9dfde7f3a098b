"""Untangle a stack of shells on the device: move vertices, and only vertices, until shell k lies inside shell k + 1
(csrc/shell_untangle.hip).  The renderer composites the K shells in shell order and never sorts by depth, which is only
right for nested shells; `mesh_intersect.check_shells` says when they are not, this stage repairs it.  The reference has
no such stage: the rule is this library's own (include/volsurfs_hip.h "Shell untangling"), restated in
tests/shell_untangle_restated.py and unpinned.

The anchor shell (the middle one by default) never moves; the order is `shell_stack.stack_order`'s, each shell against
its "out" neighbour.  The shells outside it are taken from the anchor outward, each
moving OUTWARD (side +1) against its already final inner neighbour; then the shells inside it from the anchor inward,
each moving INWARD (side -1) against its already final outer neighbour.  For one moving shell M against one fixed shell
X every vertex of M carries a level, 0 at first, and the rounds repeat:

1. project — every vertex p of M, referenced by a face or not, asks X as `RayTracer.signed_distance(p, X, sign, beta)`
   does.  With m = margin * 2^min(level, max_level), the vertex is violated iff side * dist < m; a violated vertex moves
   to p + t g, t = side * (1.25 m) - dist, g the unit residual away from X's surface on the side dist names (the
   pseudonormal of the closest feature where the vertex lies on X).  A g that is not finite leaves the vertex: stuck.
2. count — the crossing face pairs P of M's faces against X (the count pass of `mesh_intersect`: nothing is emitted).
3. stop when nothing moved and P == 0 (converged); otherwise every vertex of every crossing face of M is raised one
   level, once per round, and the next round follows.  After `max_rounds` rounds: converged = False.

Vertex clearance alone does not clear faces (a vertex of X can poke through a face of M whose own vertices are clear);
raising the margin of exactly those faces pulls them off X.  One blocking read per round.

When a pair converges (and no vertex is stuck): every vertex of M has side * dist >= margin to X; no face of M crosses a
face of X, so for closed shells `shells_nested` is True.  Always: faces, UVs, vertex count and vertex order are
unchanged (atlases and trained textures stay valid, trees are `refit`, never rebuilt); a shell that needed nothing comes
back with the same bits; the same input gives the same bytes on every call and for every builder.  NOT guaranteed: that
M does not cross itself afterwards (reported: self_crossings_after), that a pair converges (reported: converged),
anything about shells that are not consecutive.

* `untangle_shells(meshes)` — the stack; `RayTracer.untangle` is its one pair.
* `untangle_meshes(meshes_dir, out_dir)` — a `meshes*/` directory into the same names and formats: after
  `simplify_meshes`, or after `compute_meshes_atlas` (the atlas stays valid).
"""
import collections
import math
import struct

import torch

from . import _lib
from .mesh_intersect import arrays_of, check_shells, leaf_order, tree_of
from .mesh_sdf import pseudonormals
from .raytrace import RayTracer
from .shell_stack import (check_stack, displacement, load_shell_dir, save_shell_dir, self_crossing_count, stack_order,
                          with_vertices)

UntangleReport = collections.namedtuple(
    "UntangleReport", "shell side against rounds moved_vertices max_displacement max_level stuck crossings_before "
                      "crossings_after self_crossings_after converged")
UntangleReport.__doc__ = """One shell of `untangle_shells`: shell = its index, side = +1 (moved outward), -1 (inward) or
0 (the anchor: against None, nothing ran), rounds = the rounds run, moved_vertices = the vertices whose bits changed,
max_displacement = the largest distance of a moved vertex from its input position (fp64 of the fp32 coordinates),
max_level = the highest level a vertex reached, stuck = the stuck vertices of the last round, crossings_before / _after
= the crossing face pairs against the fixed neighbour, self_crossings_after = the shell's own crossing pairs i < j."""

MAX_LEVEL_CAP = 30


def _check_rule(margin, max_rounds, max_level, sign):
    margin = float(margin)
    if not (margin > 0.0 and math.isfinite(margin)):
        raise ValueError(f"untangle: margin must be a positive finite number, got {margin}")
    if int(max_rounds) < 1:
        raise ValueError(f"untangle: max_rounds must be >= 1, got {max_rounds}")
    if not 0 <= int(max_level) <= MAX_LEVEL_CAP:
        raise ValueError(f"untangle: max_level must be in 0..{MAX_LEVEL_CAP}, got {max_level}")
    if sign not in RayTracer.SIGNS:
        raise ValueError(f"sign must be one of {RayTracer.SIGNS}, got {sign!r}")
    return margin, int(max_rounds), int(max_level)


@torch.no_grad()
def untangle_pair(tracer, mesh_id, against, side, margin=1e-3, max_rounds=16, max_level=6, sign="pseudonormal",
                  beta=2.0, log=None):
    """`RayTracer.untangle`: the rounds of shell `mesh_id` against shell `against` of one tracer, then the tracer's
    `refit`.  Returns the shell's `UntangleReport`; `log` (a list) takes one (moved, stuck, max |t|, P) per round."""
    margin, max_rounds, max_level = _check_rule(margin, max_rounds, max_level, sign)
    mesh_id, against, side = int(mesh_id), int(against), int(side)
    K = tracer.nr_meshes
    if not (0 <= mesh_id < K and 0 <= against < K) or mesh_id == against:
        raise ValueError(f"untangle: shells {mesh_id} and {against} must be two of 0..{K - 1}")
    if side not in (1, -1):
        raise ValueError(f"untangle: side must be +1 (outward) or -1 (inward), got {side}")
    tracer.require_q16("untangle")
    rule = tracer.sign_rule(sign, [against])
    beta = tracer._check_beta(beta)
    dev = tracer.device
    # (X's table alone, not `tracer.pseudonormal_tables()`: the other shells' tables are not needed, and a moving
    # shell may hold a NaN vertex, which `pseudonormals` refuses)
    table = pseudonormals(tracer._meshes[against], device=dev)
    moments, moment_root = None, 0
    if rule == "winding":
        moments, entries = tracer.winding_moments()
        moment_root = int(entries[against])
    _, _, tv, tf = tree_of((tracer, against), "untangle")
    mesh = tracer._meshes[mesh_id]
    v0, f = arrays_of(mesh, dev, "untangle")
    v = v0.clone()
    V, F, Ft = v.shape[0], f.shape[0], tf.shape[0]
    order = leaf_order(tracer, mesh_id)
    if order.shape[0] != F:
        raise _lib.VolsurfsHipError(f"the tracer holds {order.shape[0]} faces of a mesh of {F}")
    nbytes = _lib.workspace_bytes("vsa_shell_untangle_workspace_bytes", V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cbytes = _lib.workspace_bytes("vsa_mesh_cross_workspace_bytes", F, 0, 0)
    cws = torch.empty(cbytes, dtype=torch.uint8, device=dev)
    count_q = torch.empty(F, dtype=torch.int32, device=dev)
    count_t = torch.empty(Ft, dtype=torch.int32, device=dev)
    offsets = torch.empty(F, dtype=torch.int32, device=dev)
    state = torch.zeros(4, dtype=torch.int64, device=dev)
    before = torch.zeros(1, dtype=torch.int64, device=dev)
    qnodes, tris, root, frame, _, depth = tracer.q16_tree_args(against)
    cross_args = (qnodes, tris, root[0], frame, depth, tv, tv.shape[0], tf, Ft, v, V, f, F, order, 0)
    st = _lib.stream_ptr()
    _lib.call("vsa_mesh_cross_count", *cross_args, count_q, count_t, offsets, before, cws, cbytes, st)
    rounds, converged, last = 0, False, (0, 0, 0, 0)
    for rnd in range(max_rounds):
        _lib.call("vsa_shell_untangle_project", qnodes, tris, root[0], frame, depth, table, 0, moments,
                  moment_root, beta, v, V, side, margin, max_level, rnd, ws, nbytes, state, st)
        _lib.call("vsa_mesh_cross_count", *cross_args, count_q, count_t, offsets, state[3:], cws, cbytes, st)
        _lib.call("vsa_shell_untangle_escalate", count_q, f, F, V, rnd, ws, nbytes, st)
        last = moved, stuck, t_bits, pairs = state.cpu().tolist()          # the round's one blocking read
        rounds = rnd + 1
        if log is not None:
            log.append((moved, stuck, struct.unpack("<f", struct.pack("<I", t_bits))[0], pairs))
        if moved == 0 and pairs == 0:
            converged = True
            break
    changed, disp = displacement(v, v0)
    meshes = list(tracer._meshes)
    meshes[mesh_id] = with_vertices(mesh, v)
    tracer.refit(meshes)
    selfs = self_crossing_count(tracer, mesh_id)
    level = ws[:4 * V].view(torch.int32)
    summary = torch.stack([changed.sum().double(), disp.max(), level.max().double(), before[0].double(),
                           selfs[0].double()]).cpu().tolist()
    return UntangleReport(mesh_id, side, against, rounds, int(summary[0]), float(summary[1]), int(summary[2]),
                          int(last[1]), int(summary[3]), int(last[3]), int(summary[4]), converged)


@torch.no_grad()
def untangle_shells(meshes, anchor=None, margin=1e-3, max_rounds=16, max_level=6, sign="pseudonormal", beta=2.0,
                    log=None):
    """(meshes, report): the K >= 2 shells `meshes` (inner to outer; a list of cuda TensorMeshes, for which one tracer
    is built with builder="device", or a RayTracer, which is refit in place) untangled by the module's rule.  `anchor`
    (default K // 2) never moves.  The returned meshes are new TensorMeshes with the input's faces, UVs and vertex
    colours; `report` is a list of K `UntangleReport`, the anchor's with side 0.  `log` (a dict) takes the round log
    of every moved shell: {shell: [(moved, stuck, max |t|, P), ...]}.  Argument errors raise before any HIP call."""
    _check_rule(margin, max_rounds, max_level, sign)
    if not float(beta) > 1.0:
        raise ValueError(f"beta must be > 1 (math.inf: every leaf is summed exactly), got {beta}")
    meshes, K, anchor = check_stack(meshes, anchor, None, "untangle_shells")
    tracer = RayTracer.over(meshes)
    reports = [None] * K
    kw = dict(margin=margin, max_rounds=max_rounds, max_level=max_level, sign=sign, beta=beta)
    for k, guards in stack_order(K, anchor)[1:]:                  # (the anchor, first in the order, never moves)
        against = dict(guards)["out"]                             # the already final neighbour
        side = 1 if k > against else -1
        rounds = [] if log is not None else None
        reports[k] = tracer.untangle(k, against, side, log=rounds, **kw)
        if log is not None:
            log[k] = rounds
    reports[anchor] = UntangleReport(anchor, 0, None, 0, 0, 0.0, 0, 0, 0, 0,
                                     int(self_crossing_count(tracer, anchor).item()), True)
    return [with_vertices(m, m.vertices) for m in tracer._meshes], reports


def untangle_meshes(meshes_dir, out_dir, **kw):
    """`untangle_shells` of a `meshes*/` directory (`<level>.ply` / `.obj`, sorted by level as
    `VolSurfs.from_meshes_path` sorts them) into `out_dir` under the same names and in the same formats: an OBJ keeps
    its per-corner UVs, a PLY its wedge UVs, its vertex colours and its ascii / binary form.  Returns (report,
    `check_shells(out_dir)`).  It can sit after `simplify_meshes`, or after `compute_meshes_atlas`: only vertices move,
    so the atlas stays valid."""
    names, meshes, colors = load_shell_dir(meshes_dir)
    out, report = untangle_shells(meshes, **kw)
    save_shell_dir(meshes_dir, out_dir, names, out, colors)
    return report, check_shells(out_dir)


__all__ = ["UntangleReport", "untangle_pair", "untangle_shells", "untangle_meshes"]
