"""The background mesh of the reference's baker: projective TSDF fusion of rendered depth maps on the device
(volsurfs_py/utils/mesh_from_depth.py:150-342 `MeshExtractor`, baker.py:454-579 `--extract_bg_mesh`), with the fusion
in HIP (csrc/tsdf_fuse.hip, rule in include/volsurfs_hip.h "TSDF fusion" and DESIGN §24).

* `MeshExtractor` — the reference's class: V depth maps, colour maps, poses and intrinsics in, a mesh out.
  `fuse_lattice` / `fuse_points` are its two passes; `extract_mesh_unbounded` is fuse -> marching cubes -> inverse
  contraction and clip -> vertex colours, everything on the device.
* `extract_bg_mesh` — the baker stage: render every camera, keep the renders in `tmp_renders/*.npz`, fuse, write
  `meshes/bg.ply`.  The reference stops after building the extractor's argument lists (its call is commented out,
  baker.py:601-602); what follows them here is this project's decision.

Differences from the reference, on purpose: any resolution >= 2 (its multiple-of-512 assert comes from its 512^3
skimage crops, whose repeated boundary planes above 512 are not mirrored); vertices arrive merged, one per crossed
lattice edge, so there is no `merge_vertices(digits_vertex=6)`; the default inverse contraction is the reference's own
C++ rule (RaySamplerGPU.cuh:595-650; mvdatasets' `uncontract_points` is absent and unpinned); `extract_mesh_bounded`
(Open3D's ScalableTSDFVolume) is not provided.
"""
import math
import os

import numpy as np
import torch

from . import _lib
from .isosurface import _uvless, marching_cubes
from .mesh import TensorMesh, save_ply

ZNEAR, ZFAR = 0.1, 100        # to_cam_open3d's getProjectionMatrix(0.1, 100, ...)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def full_proj_transforms(c2ws, intrinsics):
    """mesh_from_depth.py:122-147, 345-374: [V, 4, 4] f32, projection(0.1, 100, fovx, fovy) @ inv(c2w).  The fovs
    come from the intrinsics with the image width and height taken as 2 cx and 2 cy (`intrinsic_to_fov`), so
    normalised coordinate +-1 is pixel 0 / 2 c, whatever the maps' size.  Float64 on the host (the inverse in the
    pose's own type, as numpy gives it), cast once."""
    out = []
    for c2w, K in zip(c2ws, intrinsics):
        c2w, K = _host(c2w), _host(K)
        if c2w.shape != (4, 4) or K.shape != (3, 3):
            raise ValueError(f"expected 4x4 poses and 3x3 intrinsics, got {c2w.shape} and {K.shape}")
        fov_x = 2 * np.arctan2(K[0, 2] * 2, 2 * K[0, 0])
        fov_y = 2 * np.arctan2(K[1, 2] * 2, 2 * K[1, 1])
        P = np.zeros((4, 4))
        P[0, 0], P[1, 1], P[3, 2] = 1 / math.tan(fov_x / 2), 1 / math.tan(fov_y / 2), 1.0
        P[2, 2], P[2, 3] = ZFAR / (ZFAR - ZNEAR), -(ZFAR * ZNEAR) / (ZFAR - ZNEAR)
        out.append(torch.from_numpy(P @ np.linalg.inv(c2w)))
    return torch.stack(out).float()


@torch.no_grad()
def uncontract_points(points, max_range=32.0):
    """The vertex step: the inverse contraction of points [P, 3] (RaySamplerGPU.cuh:595-650 without the ray part),
    clipped per component to +-max_range (vsa_tsdf_uncontract_points).  A point outside the contraction's image
    (|2 p| >= 2) goes to +-max_range along its non-zero components."""
    points = _lib.check_f32(points.contiguous())
    out = torch.empty_like(points)
    _lib.call("vsa_tsdf_uncontract_points", points, points.shape[0], float(max_range), out, _lib.stream_ptr())
    return out


class MeshExtractor:
    """mesh_from_depth.py:150-342 with the reference's arguments: `depthmaps` a list of [1, H, W] tensors (camera z,
    0 where nothing was hit), `rgbs` of [3, H, W], `c2ws` of 4x4 camera-to-world poses (x right, y down, z forward),
    `intrinsics` of 3x3 matrices.  The maps are stacked on the device and stay there.

    Two quirks of the reference are kept as the defaults:
      * the TSDF is fused at the CONTRACTED lattice positions as if they were world positions (the reference has
        `samples = inv_contraction(samples)` commented out, mesh_from_depth.py:264), while the vertices do go through
        the inverse contraction afterwards.  Inside the unit ball the contraction is the identity, so a scene there is
        unaffected.  `uncontract_samples=True` is the consistent form.
      * a voxel further than sdf_trunc behind a surface is masked out and keeps the initial tsdf = 1 instead of a
        negative value, so the grid crosses 0 a second time there: a second, inward-facing sheet lies about
        sdf_trunc behind every observed surface."""

    def __init__(self, depthmaps, rgbs, c2ws, intrinsics, with_vertex_colors=False, device="cuda"):
        if not len(depthmaps) or not len(depthmaps) == len(rgbs) == len(c2ws) == len(intrinsics):
            raise ValueError("MeshExtractor: one depth map, colour map, pose and intrinsics per view, at least one view")
        self.depthmaps = torch.stack([torch.as_tensor(d, dtype=torch.float32) for d in depthmaps]).to(device).contiguous()
        self.rgbmaps = torch.stack([torch.as_tensor(c, dtype=torch.float32) for c in rgbs]).to(device).contiguous()
        V, _, H, W = self.depthmaps.shape
        if self.depthmaps.shape != (V, 1, H, W) or self.rgbmaps.shape != (V, 3, H, W):
            raise ValueError(f"MeshExtractor: depth maps [1, H, W] and colour maps [3, H, W] of one size, got "
                             f"{tuple(self.depthmaps.shape)} and {tuple(self.rgbmaps.shape)}")
        self.nr_views, self.height, self.width = V, H, W
        self.with_vertex_colors = bool(with_vertex_colors)
        self.full_proj_transform = full_proj_transforms(c2ws, intrinsics).to(device).contiguous()

    @staticmethod
    def truncation(resolution):
        """(voxel_size, sdf_trunc) = (2 / resolution, 5 voxel_size), mesh_from_depth.py:263, 304-306."""
        voxel_size = 1.0 * 2 / int(resolution)
        return voxel_size, 5 * voxel_size

    @torch.no_grad()
    def fuse_lattice(self, resolution=512, uncontract_samples=False, sdf_trunc=None):
        """The fused grid [n, n, n] f32 on the lattice torch.linspace(-1, 1, n)^3 ("ij" order), n = resolution."""
        n = int(resolution)
        trunc = self.truncation(n)[1] if sdf_trunc is None else float(sdf_trunc)
        dev = self.depthmaps.device
        axis = torch.linspace(-1.0, 1.0, max(n, 1), dtype=torch.float32).to(dev)
        out = torch.empty(max(n, 0), max(n, 0), max(n, 0), device=dev)
        _lib.call("vsa_tsdf_fuse_lattice", self.full_proj_transform, self.depthmaps, self.nr_views, self.height,
                  self.width, axis, n, trunc, bool(uncontract_samples), out, _lib.stream_ptr())
        return out

    @torch.no_grad()
    def fuse_points(self, points, return_rgb=False, sdf_trunc=None, resolution=512, uncontract_samples=False):
        """tsdf [P] of points [P, 3], and with `return_rgb` (tsdf, rgb [P, 3]): the reference's
        compute_unbounded_tsdf(points, ..., return_rgb).  sdf_trunc defaults to that of `resolution`."""
        points = _lib.check_f32(points.contiguous())
        if points.dim() != 2 or points.shape[1] != 3:
            raise _lib.VolsurfsHipError(f"fuse_points: expected points [P, 3], got {tuple(points.shape)}")
        trunc = self.truncation(resolution)[1] if sdf_trunc is None else float(sdf_trunc)
        P = points.shape[0]
        tsdf = torch.empty(P, device=points.device)
        rgb = torch.empty(P, 3, device=points.device) if return_rgb else None
        _lib.call("vsa_tsdf_fuse_points", self.full_proj_transform, self.depthmaps,
                  self.rgbmaps if return_rgb else None, self.nr_views, self.height, self.width, points, P, trunc,
                  bool(uncontract_samples), tsdf, rgb, _lib.stream_ptr())
        return (tsdf, rgb) if return_rgb else tsdf

    @torch.no_grad()
    def extract_mesh_unbounded(self, resolution=512, uncontract_samples=False, inv_contraction="default",
                               max_range=32.0, cluster_to_keep=None):
        """mesh_from_depth.py:213-342: the level-0 surface of the fused lattice (`isosurface.marching_cubes`, inside
        where tsdf < 0), its vertices through the inverse contraction and clipped to +-max_range, and, with
        `with_vertex_colors`, the colours fused at the final vertex positions as the reference does (world positions,
        no contraction).  `inv_contraction`: "default" (uncontract_points), None (vertices stay contracted, no clip,
        as marching_cubes_with_contraction does without one) or a callable [V, 3] -> [V, 3], clipped afterwards.
        `cluster_to_keep`: None leaves the mesh as fused; an integer runs `mesh_clean.post_process_mesh` on it, the
        colours included (the reference's commented-out post-processing, mesh_from_depth.py:449-464).
        Returns a TensorMesh (no UVs), or (mesh, colours [V, 3] f32) with `with_vertex_colors`."""
        n = int(resolution)
        grid = self.fuse_lattice(n, uncontract_samples)
        mesh = marching_cubes(grid, 0.0, [-1.0] * 3, [2.0 / (n - 1)] * 3)[0]
        del grid
        verts = mesh.vertices
        if isinstance(inv_contraction, str):
            if inv_contraction != "default":
                raise ValueError(f"inv_contraction must be 'default', None or a callable, got {inv_contraction!r}")
            verts = uncontract_points(verts, max_range)
        elif inv_contraction is not None:
            verts = inv_contraction(verts).to(torch.float32).clamp(-float(max_range), float(max_range)).contiguous()
        mesh = _uvless(verts, mesh.faces)
        colors = self.fuse_points(verts, return_rgb=True, resolution=n)[1] if self.with_vertex_colors else None
        if cluster_to_keep is not None:
            from .mesh_clean import post_process_mesh
            if colors is None:
                mesh = post_process_mesh(mesh, cluster_to_keep)
            else:
                mesh, colors = post_process_mesh(mesh, cluster_to_keep, vertex_colors=colors)
        return mesh if colors is None else (mesh, colors)


# ---- the baker stage (baker.py:454-579)

RENDER_FILES = {"depths_fg": "depth_fg", "depths_bg": "depth_bg", "fg_mask": "weights_sum", "rgbs": "rgb"}


@torch.no_grad()
def _render_camera(method, camera, keys):
    """{key: [H, W, C]} of the volumetric render of one camera, outside training, in the chunks `method.render` uses;
    render_rays' full "volumetric" entry is read because `render` keeps only RENDER_KEYS (no depth_fg / depth_bg)."""
    from .camera import get_camera_rays
    was = method.is_training
    method.is_training = False
    try:
        rays_o, rays_d, _ = get_camera_rays(camera)
        chunk = int(method.hyper_params.test_rays_batch_size)
        outs = {k: [] for k in keys}
        for a in range(0, rays_o.shape[0], chunk):
            v = method.render_rays(rays_o[a:a + chunk], rays_d[a:a + chunk])["renders"]["volumetric"]
            for k in keys:
                outs[k].append(v[k])
    finally:
        method.is_training = was
    return {k: torch.cat(v, 0).reshape(camera.height, camera.width, -1) for k, v in outs.items()}


def ray_length_to_camera_z(depth, camera):
    """depth [H, W, 1] along unit-length rays -> camera z: z = t (d . forward), forward = column 2 of the pose.
    `camera.get_camera_rays` normalises its directions (csrc/raygen.hip: d = normalise(R Kinv (x, y, 1))), so the
    ray parameter the methods report as depth is a Euclidean length."""
    from .camera import get_camera_rays
    _, rays_d, _ = get_camera_rays(camera)
    cos = (rays_d * camera.c2w[:3, 2].to(rays_d.device)).sum(-1)
    return depth * cos.reshape(camera.height, camera.width, 1)


@torch.no_grad()
def extract_bg_mesh(method, cameras, out_dir=None, resolution=512, depth="fg", depth_is_ray_length=True,
                    with_vertex_colors=True, reuse_renders=True, cluster_to_keep=None, **extractor_kwargs):
    """The baker's `--extract_bg_mesh` (baker.py:454-579) for a method with a background model (it raises for one
    without; the reference prints and exits).  Every camera is rendered in "volumetric" mode; rgb, depth_fg, depth_bg
    and weights_sum go to `<out_dir>/tmp_renders/{rgbs,depths_fg,depths_bg,fg_mask}.npz` keyed by the camera index, as
    [H, W, C] arrays, and are read back from there when `reuse_renders` and depths_fg.npz exists (baker.py:466-528).
    `depth`: "fg" is the reference's choice (baker.py:549), "composed" the line it has commented out (baker.py:548),
    depth_fg mask + depth_bg (1 - mask).  The fused mesh is written to `<out_dir>/meshes/bg.ply` (baker.py:631) with
    uchar vertex colours when `with_vertex_colors`.  out_dir None: nothing is written or reused.

    The reference stops before the fusion, so two things are this project's: the `depth` switch, and
    `depth_is_ray_length` (default True): the methods' depth is the parameter along unit-length rays
    (`camera.get_camera_rays` normalises its directions), the fusion compares with camera z, so the depth is
    converted on the device, z = t (ray direction . camera forward axis).  False hands the renders over unconverted,
    the reference's unfinished state.  `cluster_to_keep`: None writes the fused mesh as it is; an integer removes its
    floaters first (`mesh_clean.post_process_mesh` on the unbounded mesh, colours included).  `extractor_kwargs` go to
    `extract_mesh_unbounded`.
    Returns (mesh, colours or None)."""
    if depth not in ("fg", "composed"):
        raise ValueError(f"depth must be 'fg' or 'composed', got {depth!r}")
    if getattr(method, "models", {}).get("bg") is None:
        raise ValueError(f"method {getattr(method, 'method_name', type(method).__name__)} has no background model: "
                         "background mesh extraction is not supported")
    cameras = list(cameras)
    if not cameras:
        raise ValueError("extract_bg_mesh: no cameras")
    tmp = None if out_dir is None else os.path.join(out_dir, "tmp_renders")
    renders = None
    if tmp is not None and reuse_renders and os.path.exists(os.path.join(tmp, "depths_fg.npz")):
        renders = {}
        for name in RENDER_FILES:
            with np.load(os.path.join(tmp, f"{name}.npz")) as data:
                renders[name] = {k: data[k] for k in data}
        if sorted(renders["depths_fg"], key=int) != [str(i) for i in range(len(cameras))]:
            raise ValueError(f"{tmp}: renders of {len(renders['depths_fg'])} cameras, {len(cameras)} cameras given")
    if renders is None:
        renders = {name: {} for name in RENDER_FILES}
        for idx, cam in enumerate(cameras):
            out = _render_camera(method, cam, tuple(RENDER_FILES.values()))
            for name, key in RENDER_FILES.items():
                renders[name][str(idx)] = out[key].cpu().numpy()
        if tmp is not None:
            os.makedirs(tmp, exist_ok=True)
            for name in RENDER_FILES:
                np.savez(os.path.join(tmp, f"{name}.npz"), **renders[name])
    dev = "cuda"
    depths, rgbs, c2ws, ixts = [], [], [], []
    for idx, cam in enumerate(cameras):
        k = str(idx)
        d = torch.from_numpy(renders["depths_fg"][k]).to(dev)
        if depth == "composed":
            m = torch.from_numpy(renders["fg_mask"][k]).to(dev)
            d = d * m + torch.from_numpy(renders["depths_bg"][k]).to(dev) * (1 - m)
        if depth_is_ray_length:
            d = ray_length_to_camera_z(d, cam)
        depths.append(d.permute(2, 0, 1).float())
        rgbs.append(torch.from_numpy(renders["rgbs"][k]).to(dev).permute(2, 0, 1).float())
        c2w = torch.eye(4, dtype=torch.float64)
        c2w[:3] = cam.c2w.double().cpu()
        c2ws.append(c2w.numpy())
        ixts.append(cam.intrinsics.double().numpy())
    extractor = MeshExtractor(depths, rgbs, c2ws, ixts, with_vertex_colors=with_vertex_colors, device=dev)
    if cluster_to_keep is not None:
        extractor_kwargs = dict(extractor_kwargs, cluster_to_keep=cluster_to_keep)
    res = extractor.extract_mesh_unbounded(resolution=resolution, **extractor_kwargs)
    mesh, colors = res if with_vertex_colors else (res, None)
    if out_dir is not None:
        if mesh.faces.shape[0] == 0:
            raise ValueError("the fused grid has no level-0 surface: nothing to save")
        os.makedirs(os.path.join(out_dir, "meshes"), exist_ok=True)
        save_ply(os.path.join(out_dir, "meshes", "bg.ply"),
                 TensorMesh(mesh.vertices, mesh.faces, None, device=mesh.vertices.device), vertex_colors=colors)
    return mesh, colors
