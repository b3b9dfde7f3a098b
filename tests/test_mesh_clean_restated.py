"""The yardstick of tests/test_mesh_clean.py tested without a GPU: tests/mesh_clean_restated.py against the seven-sphere
numbers and the hand-built adjacency cases of the rule (include/volsurfs_hip.h "Mesh cleaning")."""
import numpy as np
import pytest

import mesh_clean_restated as R


def test_seven_spheres_numbers():
    v, f = R.seven_spheres()
    assert f.shape == (6920, 3) and v.dtype == np.float32 and f.dtype == np.int32
    cl, n, area = R.cluster_connected_triangles(v, f)
    # the multiset is the construction's; the order is that of the clusters' smallest faces under this permutation
    # (f[default_rng(0).permutation(F)])
    assert sorted(n.tolist()) == sorted([5120, 320, 1280, 80, 80, 20, 20])
    assert n.tolist() == [5120, 1280, 80, 20, 80, 320, 20]
    first = [int(np.nonzero(cl == c)[0][0]) for c in range(7)]
    assert first == sorted(first) and first[0] == 0
    # an icosphere of radius r approaches 4 pi r^2 from below
    r = {5120: 0.5, 1280: 0.3, 320: 0.1}
    for c in range(7):
        if int(n[c]) in r:
            assert 0.97 < area[c] / (4 * np.pi * r[int(n[c])] ** 2) < 1.0
    for k, thr, kept in ((1, 5120, 5120), (2, 1280, 6400), (3, 320, 6720), (4, 80, 6880), (5, 80, 6880),
                         (1000, 50, 6880)):
        out = R.post_process_mesh(v, f, k)
        assert (out["threshold"], out["faces"].shape[0]) == (thr, kept), k
        assert np.array_equal(out["vertices"][out["faces"]], v[f[out["face_index"]]])       # the same triangles
        assert np.array_equal(out["vertices"], v[out["vertex_index"]])
        assert (np.diff(out["face_index"]) > 0).all() and (np.diff(out["vertex_index"]) > 0).all()
    assert R.post_process_mesh(v, f, 4)["clusters_kept"] == 5                               # the tie at 80: both stay
    with pytest.raises(ValueError):
        R.post_process_mesh(v, f, 0)


@pytest.mark.parametrize("name", sorted(R.corner_cases()))
def test_corner_cases(name):
    v, f, expected = R.corner_cases()[name]
    cl, n, area = R.cluster_connected_triangles(v, f)
    assert np.array_equal(cl, expected) and np.array_equal(n, np.bincount(expected))
    assert np.allclose(area.sum(), R.face_areas(v, f).sum(), rtol=1e-14)
    out = R.post_process_mesh(v, f, 1000, min_cluster_faces=1)
    if name == "twice_named_vertex":
        assert np.array_equal(out["faces"], [[0, 1, 2], [3, 4, 5]]) and out["vertex_index"].tolist() == [0, 1, 2, 4, 5, 6]
        lone = R.post_process_mesh(v, [[0, 1, 2], [3, 3, 2], [4, 5, 6]], 1000, min_cluster_faces=1)
        assert lone["vertices"].shape[0] == 7 and lone["face_index"].tolist() == [0, 2]
    elif name == "unreferenced_vertices":
        assert out["vertex_index"].tolist() == [1, 2, 3, 5, 6, 7, 8] and out["faces"].shape[0] == 4
    else:
        assert out["faces"].shape[0] == f.shape[0]


def test_removals_and_empty():
    v, f = R.seven_spheres()
    assert R.remove_triangles_by_mask(v, f, np.zeros(f.shape[0], bool))[1].tobytes() == f.tobytes()
    assert R.remove_triangles_by_mask(v, f, np.ones(f.shape[0], bool))[1].shape == (0, 3)
    wv, wf, idx = R.remove_unreferenced_vertices(v, f[:10])
    assert np.array_equal(wv[wf], v[f[:10]]) and wv.shape[0] == np.unique(f[:10]).shape[0]
    out = R.post_process_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3)
    assert R.threshold([5, 9, 7], 2, 0) == 7 and R.threshold([5, 9, 7], 10, 0) == 5 and R.threshold([5, 9, 7], 1) == 50


def test_blob_field_is_a_ball_and_separate_blobs():
    grid, origin, spacing, big, centres = R.blob_field(48)
    assert grid.shape == (48, 48, 48) and grid.dtype == np.float32 and len(centres) >= 24
    assert (grid <= big).all() and float(grid[24, 24, 24]) < -0.5
    for i, (c, r) in enumerate(centres):
        assert np.linalg.norm(c) - r > 0.55
        assert all(np.linalg.norm(c - c2) > r + r2 for c2, r2 in centres[:i])
