"""A2 on the GPU: the device LBVH builder and refit (csrc/bvh_device.hip, RayTracer(builder="device")).

The cases that hold for any device builder are in tests/bvh_builder_cases.py (tests/test_bvh_ploc.py runs them for
builder="ploc"); what holds for the LBVH alone is here: its entry points' argument checks and the guard on its SAH
cost."""
import ctypes

import pytest

from tests import bvh_builder_cases as cases
from volsurfs_amd.mesh import icosphere


# ---------------------------------------------------------------------------------------------- no GPU needed

def test_device_builder_entry_points_reject_bad_arguments_before_touching_the_device():
    from volsurfs_amd import _lib
    L = _lib.lib()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)                        # never dereferenced: the checks come first
    h = ctypes.c_void_p()
    ERR_ARG = -1
    assert L.vsa_bvh_dev_build(null, one, 3, 1, 4, null, ctypes.byref(h)) == ERR_ARG
    assert L.vsa_bvh_dev_build(one, null, 3, 1, 4, null, ctypes.byref(h)) == ERR_ARG
    assert L.vsa_bvh_dev_build(one, one, 3, 1, 4, null, None) == ERR_ARG
    assert L.vsa_bvh_dev_build(one, one, 3, 0, 4, null, ctypes.byref(h)) == ERR_ARG
    assert L.vsa_bvh_dev_build(one, one, 3, -5, 4, null, ctypes.byref(h)) == ERR_ARG
    assert L.vsa_bvh_dev_build(one, one, 0, 1, 4, null, ctypes.byref(h)) == ERR_ARG
    assert L.vsa_bvh_dev_sizes(null, None, None, None) == ERR_ARG
    assert L.vsa_bvh_dev_export(null, one, one, one, 0, 0, one, null) == ERR_ARG
    assert L.vsa_bvh_dev_refit(null, one, 3, null) == ERR_ARG
    assert L.vsa_bvh_dev_destroy(null) == 0


def test_unknown_builder_is_refused():
    from volsurfs_amd import _lib
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.raytrace import RayTracer
    v, f = icosphere(1, 0.3)
    with pytest.raises(_lib.VolsurfsHipError, match="builder"):
        RayTracer([TensorMesh(v, f, device="cpu")], builder="bogus")


def test_device_builder_needs_the_meshes_on_the_gpu():
    cases.builder_needs_the_meshes_on_the_gpu("device")


# ---------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["q16", "f32"])
@pytest.mark.parametrize("subdiv,n", [(0, 1000), (2, 4096), (4, 4096), (5, 2000)])
def test_device_tree_bit_exact_vs_bruteforce(subdiv, n, fmt):
    cases.tree_bit_exact_vs_bruteforce("device", subdiv, n, fmt)


@pytest.mark.gpu
def test_device_tree_equals_host_tree_on_every_traversal_form():
    cases.tree_equals_host_tree_on_every_traversal_form("device")


@pytest.mark.gpu
@pytest.mark.parametrize("leaf_size", [1, 4, 8])
def test_device_tree_structure(leaf_size):
    cases.tree_structure("device", leaf_size)


@pytest.mark.gpu
def test_device_build_is_deterministic():
    from volsurfs_amd.mesh import nested_shells
    cases.assert_deterministic(nested_shells(K=3, subdiv=5, noise=0.05), builder="device")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["q16", "f32"])
def test_device_tree_edge_cases(fmt):
    cases.tree_edge_cases("device", fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("stress", [False, True])
def test_device_tree_sah_cost_is_not_degenerate(stress):
    """A guard against a correct but degenerate tree (not a measured target)."""
    from volsurfs_amd.mesh import nested_shells, stress_shells
    from volsurfs_amd.raytrace import RayTracer
    meshes = stress_shells(K=5, subdiv=6) if stress else nested_shells(K=3, subdiv=5)
    host, dev = RayTracer(meshes).sah_cost(), RayTracer(meshes, builder="device").sah_cost()
    for h, d in zip(host, dev):
        assert d <= 1.5 * h, (host, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["q16", "f32"])
def test_device_refit_after_the_vertices_moved_is_bit_exact_and_keeps_the_slots(fmt):
    cases.refit_after_the_vertices_moved_is_bit_exact_and_keeps_the_slots("device", fmt)


@pytest.mark.gpu
def test_volsurfs_with_the_device_tree_renders_the_host_trees_pixels():
    cases.volsurfs_with_the_tree_renders_the_host_trees_pixels("device")


@pytest.mark.gpu
def test_pipeline_step_with_the_device_tree_equals_the_host_trees():
    cases.pipeline_step_with_the_tree_equals_the_host_trees("device")
