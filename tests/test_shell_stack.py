"""The seam the shell-stack stages share (volsurfs_amd/shell_stack.py; csrc/cross_walk.h: CrossGuards,
cross_guards_bind, cross_guards_hit): one guard block, built once, serves vsa_simplify_guarded and vsa_mesh_smooth_guard
and gives each the bytes `simplify_mesh(guards=)` and `smooth_mesh(guards=)` give from TensorMesh guards and from
(RayTracer, mesh_id) guards.  What those bytes must be is the business of tests/test_simplify_guarded.py and
tests/test_mesh_smooth.py (the numpy restatements)."""
import pytest
import torch

from tests import simplify_guarded_restated as sgr
from volsurfs_amd import shell_stack
from volsurfs_amd.mesh import TensorMesh, icosphere

gpu = pytest.mark.gpu

# icosphere(2) at radius 0.52 between guards at 0.5 and 0.54.  At a tenth of its 320 faces the edges are about three
# times as long; a chord's sagitta (length^2 / 8 r) grows with the square, from 0.005 to 0.05, past the 0.02 between the
# shells: without the guard the faces would dip through the inner shell, so the guard has verdicts to turn down.
RADII, RATIO = (0.5, 0.52, 0.54), 0.1


def test_stack_order_is_simplify_stack_order_and_the_restatement():
    from volsurfs_amd import simplify
    assert simplify.stack_order is shell_stack.stack_order
    for K in (2, 3, 5):
        for anchor in range(K):
            assert shell_stack.stack_order(K, anchor) == sgr.stack_order(K, anchor)


def _bits(mesh_or_vertices):
    v = getattr(mesh_or_vertices, "vertices", mesh_or_vertices)
    return v.cpu().view(torch.int32)


@gpu
def test_one_guard_block_serves_both_stages():
    from volsurfs_amd import mesh_smooth as msm, simplify as smp
    from volsurfs_amd.raytrace import RayTracer
    inner, mid, outer = (TensorMesh(*icosphere(2, r), device="cuda") for r in RADII)
    tracer = RayTracer([inner, outer], builder="device")
    as_meshes, as_pairs = [inner, outer], [(tracer, 0), (tracer, 1)]
    block = shell_stack.guard_block(shell_stack.resolve_guards(as_pairs, "test"), "test")
    assert block[0][0] == 2 and len(block[0]) == 10

    V, F, ratio = smp._check(mid, RATIO)
    v, f, st = smp._simplify_guarded(V, F, smp.target_faces(F.shape[0], ratio), block)
    assert st["guard_rejected"] > 0
    for guards in (as_meshes, as_pairs):
        out, ref = smp.simplify_mesh(mid, RATIO, return_stats=True, guards=guards)
        assert ref == st
        assert torch.equal(out.faces.cpu(), f.cpu()) and torch.equal(_bits(out), _bits(v))

    v0, f0 = msm._check_mesh(mid, "test")
    v, st = msm._smooth(v0, f0, 3, 0.5, -0.53, True, block)      # (the same block, after the simplifier's launches)
    for guards in (as_meshes, as_pairs):
        out, rep = msm.smooth_mesh(mid, iterations=3, guards=guards)
        assert torch.equal(_bits(out), _bits(v)) and torch.equal(out.faces, mid.faces)
        assert (rep.moved_vertices, rep.max_displacement, rep.reverted, rep.guard_rounds, rep.stuck) == \
               (st["moved_vertices"], st["max_displacement"], st["reverted"], st["guard_rounds"], st["stuck"])
    assert st["moved_vertices"] > 0 and st["guard_rounds"] >= 3
