#!/usr/bin/env python3
"""Generate tests/golden/bg_mesh.npz by running the REFERENCE's own `MeshExtractor.extract_mesh_unbounded`
(volsurfs_py/utils/mesh_from_depth.py, imported in place through tools/ref_import.py) on the CPU.

Runs only in the build container (it needs the reference tree); only arrays go into the fixture.  The scene is that of
tests/bg_mesh_restated.py::fixture_scene.  The reference's `to_cam_open3d`, `getProjectionMatrix`,
`compute_sdf_perframe` and `compute_unbounded_tsdf` run as they are; what is replaced around them:
  * the absent third-party modules by placeholders (ref_import), `imageio` among them;
  * `torch.Tensor.cuda` by the identity for the run (and `torch.Tensor.float` by `.double()` in the float64 run);
  * `marching_cubes_with_contraction` (skimage, trimesh) by a function that calls the `sdf` closure it is handed on
    the fixture's query points and colour points and records the results; the stand-in mesh it returns carries the
    colour points as vertices, so that the `with_vertex_colors` pass of the reference fuses the colours there.
A second run under torch.set_default_dtype(torch.float64) with double inputs and `full_proj_transform` recomputed in
double gives the float64 value of the same rule; `maxdiff` (the largest |f32 - f64| over the query points and the
colour points) and `flips` (points where it exceeds 1e-3: a view's sample entered or left the mean because a mask
comparison rounded the other way) are printed and stored.
Usage:  python tools/make_bg_mesh_golden.py"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

import ref_import  # noqa: E402
import bg_mesh_restated as BG  # noqa: E402

FLIP = 1e-3


class _StandInMesh:
    def __init__(self, vertices):
        self.vertices, self.vertex_colors = vertices, None

    @property
    def as_open3d(self):
        return self


def run_reference(mfd, depths, rgbs, c2ws, ixts, query, rgb_points, double):
    """-> (tsdf at query, tsdf at rgb_points, rgb at rgb_points, full_proj_transform) as numpy arrays."""
    got = {}

    def stand_in(sdf, **kwargs):
        got["tsdf"] = sdf(query).numpy()
        got["tsdf_pts"] = sdf(rgb_points).numpy()
        return _StandInMesh(rgb_points.numpy())

    mfd.marching_cubes_with_contraction = stand_in
    ex = mfd.MeshExtractor(depths, rgbs, [c.numpy() for c in c2ws], ixts, with_vertex_colors=True)
    if double:
        ex.full_proj_transform = BG.projection_matrices([c.numpy() for c in c2ws], ixts, torch.float64)
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        mesh = ex.extract_mesh_unbounded(resolution=BG.FIXTURE_RESOLUTION)
    return got["tsdf"], got["tsdf_pts"], np.asarray(mesh.vertex_colors), ex.full_proj_transform.numpy()


def main():
    ref_import.ABSENT.append("imageio")
    ref_import.install_placeholders({"open3d.utility": {"Vector3dVector": lambda a: a}})
    import volsurfs_py.utils.mesh_from_depth as mfd
    depths, rgbs, c2ws, ixts, query, rgb_points = BG.fixture_scene()
    cuda, to_float = torch.Tensor.cuda, torch.Tensor.float
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        t32, tp32, c32, proj = run_reference(mfd, depths, rgbs, c2ws, ixts, query, rgb_points, False)
        torch.set_default_dtype(torch.float64)
        torch.Tensor.float = lambda self, *a, **k: self.double()      # the reference's own `.float()` casts
        dbl = lambda xs: [x.double() for x in xs]
        t64, tp64, c64, _ = run_reference(mfd, dbl(depths), dbl(rgbs), dbl(c2ws), dbl(ixts), query.double(),
                                          rgb_points.double(), True)
    finally:
        torch.set_default_dtype(torch.float32)
        torch.Tensor.cuda, torch.Tensor.float = cuda, to_float
    assert t32.dtype == np.float32 and c32.dtype == np.float32 and t64.dtype == np.float64
    assert np.array_equal(proj, BG.projection_matrices(c2ws, ixts).numpy()), "the restated matrices differ"
    diffs = [np.abs(a.astype(np.float64) - b) for a, b in ((t32, t64), (tp32, tp64), (c32, c64))]
    flips = int(sum((d > FLIP).sum() for d in diffs))
    maxdiff = float(max(d.max() for d in diffs))
    touched = int((t32 != 1).sum())
    print(f"{touched} of {t32.size} query points touched, {int((tp32 != 1).sum())} of {tp32.size} colour points; "
          f"flips = {flips}, maxdiff = {maxdiff:.2e} (tsdf {diffs[0].max():.2e}, tsdf at colour points "
          f"{diffs[1].max():.2e}, rgb {diffs[2].max():.2e})")
    arrs = {"depths": torch.stack(depths).numpy(), "rgbs": torch.stack(rgbs).numpy(),
            "c2ws": torch.stack(c2ws).numpy(), "intrinsics": torch.stack(ixts).numpy(), "proj": proj,
            "rgb_points": rgb_points.numpy(), "tsdf": t32, "tsdf_points": tp32, "rgb": c32,
            "tsdf_f64": t64, "tsdf_points_f64": tp64, "rgb_f64": c64,
            "resolution": np.int64(BG.FIXTURE_RESOLUTION), "query_n": np.int64(BG.FIXTURE_QUERY_N),
            "maxdiff": np.float64(maxdiff), "flips": np.int64(flips), "touched": np.int64(touched)}
    path = os.path.join(GOLD, "bg_mesh.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
