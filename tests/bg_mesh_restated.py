"""The rule of the TSDF fusion (include/volsurfs_hip.h, "TSDF fusion") restated in plain torch for any device and any
float type, per view, as volsurfs_py/utils/mesh_from_depth.py:220-300 formulates it (a homogeneous-point product, two
`grid_sample` calls and masked read-modify-writes per view), the projection matrices of its `to_cam_open3d`, the
inverse contraction, and the two analytic sphere scenes: the fixture's, which tools/make_bg_mesh_golden.py hands to
the reference's own class, and the larger one of the end-to-end test.  Not collected by pytest."""
import math

import numpy as np
import torch


def projection_matrices(c2ws, intrinsics, dtype=torch.float32):
    """[V, 4, 4]: proj(0.1, 100, fovx, fovy) @ inv(c2w) per view, the fovs from the intrinsics with the image size
    taken as (2 cx, 2 cy); computed in float64 from the inputs as given (the inverse in the pose's own type), then cast
    (mesh_from_depth.py:122-147, 345-374)."""
    out = []
    znear, zfar = 0.1, 100
    for c2w, K in zip(c2ws, intrinsics):
        c2w = c2w.detach().cpu().numpy() if isinstance(c2w, torch.Tensor) else np.asarray(c2w)
        K = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
        w2c = np.linalg.inv(c2w)
        fov_x = 2 * np.arctan2(K[0, 2] * 2, 2 * K[0, 0])
        fov_y = 2 * np.arctan2(K[1, 2] * 2, 2 * K[1, 1])
        P = np.zeros((4, 4))
        P[0, 0] = 1 / math.tan(fov_x / 2)
        P[1, 1] = 1 / math.tan(fov_y / 2)
        P[3, 2] = 1.0
        P[2, 2] = zfar / (zfar - znear)
        P[2, 3] = -(zfar * znear) / (zfar - znear)
        out.append(torch.from_numpy(P @ w2c))
    return torch.stack(out).to(dtype)


@torch.no_grad()
def fuse_restated(points, depthmaps, rgbmaps, proj, sdf_trunc, order=None):
    """-> (tsdf [P], rgb [P, 3], weights [P]) of points [P, 3]: depthmaps [V, 1, H, W], rgbmaps [V, 3, H, W], proj
    [V, 4, 4], all of the points' device and float type.  `order`: the views' order (default 0 .. V-1)."""
    tsdfs = torch.ones_like(points[:, 0])
    rgbs = torch.zeros_like(points)
    weights = torch.ones_like(points[:, 0])
    for i in (range(proj.shape[0]) if order is None else order):
        h = torch.cat([points, torch.ones_like(points[:, :1])], -1) @ proj[i].t()
        z = h[:, -1:]
        pix = h[:, :2] / z
        mask = ((pix > -1.0) & (pix < 1.0) & (z > 0)).all(-1)
        tap = lambda img: torch.nn.functional.grid_sample(img[None], pix[None, None], mode="bilinear",
                                                          padding_mode="border", align_corners=True)
        sdf = (tap(depthmaps[i]).reshape(-1, 1) - z).flatten()
        rgb = tap(rgbmaps[i]).reshape(3, -1).T
        mask = mask & (sdf > -sdf_trunc)
        s = torch.clamp(sdf / sdf_trunc, min=-1.0, max=1.0)[mask]
        w = weights[mask]
        wp = w + 1
        tsdfs[mask] = (tsdfs[mask] * w + s) / wp
        rgbs[mask] = (rgbs[mask] * w[:, None] + rgb[mask]) / wp[:, None]
        weights[mask] = wp
    return tsdfs, rgbs, weights


def uncontract_restated(points):
    """The inverse contraction of the rule -> (points [P, 3], inside [P] bool: norm of 2 p below 2)."""
    q = points * 2.0
    norm = torch.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
    factor = 1.0 / (2.0 - norm)
    out = torch.where((norm > 1.0)[:, None], (factor[:, None] * points) / norm[:, None], points)
    return out, norm < 2.0


# ---- analytic scenes: a sphere at the origin seen by pinhole cameras on a ring, all looking at the origin

def look_at_pose(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """Camera-to-world [4, 4] float64, columns x right, y down, z forward, centre."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, eye
    return c2w


def ring_eyes(nr_views, ring_radius, height):
    return [(ring_radius * math.cos(2.0 * math.pi * v / nr_views), ring_radius * math.sin(2.0 * math.pi * v / nr_views),
             height) for v in range(int(nr_views))]


def sphere_views(eyes, size, focal, sphere_radius=0.5, miss_rgb=(0.1, 0.2, 0.3)):
    """One view per eye position, looking at the origin -> (depthmaps [V] of [1, H, W], rgbmaps [V] of [3, H, W],
    c2ws [V] of [4, 4], intrinsics [V] of [3, 3]), float32 torch tensors on the CPU.  Depth is the camera z of the hit and 0 on a miss; colour is 0.5 + 0.5 normal at the hit.
    Pixel (row r, column c) looks through the image point (c W / (W - 1), r H / (H - 1)): the rule's `align_corners`
    mapping of the tap, under which normalised coordinate -1 is pixel 0 and +1 is pixel W - 1."""
    H = W = int(size)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]], np.float64)
    cols = np.arange(W, dtype=np.float64) * W / (W - 1)
    rows = np.arange(H, dtype=np.float64) * H / (H - 1)
    dx, dy = np.meshgrid((cols - K[0, 2]) / focal, (rows - K[1, 2]) / focal, indexing="xy")
    d_cam = np.stack([dx, dy, np.ones_like(dx)], -1)                         # z component 1: t is camera z
    depths, rgbs, c2ws, ixts = [], [], [], []
    for eye in eyes:
        c2w = look_at_pose(eye)
        d = d_cam @ c2w[:3, :3].T
        o = c2w[:3, 3]
        A, B, C = (d * d).sum(-1), 2.0 * (d @ o), o @ o - sphere_radius ** 2
        disc = B * B - 4.0 * A * C
        hit = disc > 0
        t = np.where(hit, (-B - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * A), 0.0)
        n = (o + t[..., None] * d) / sphere_radius
        rgb = np.where(hit[..., None], 0.5 + 0.5 * n, np.asarray(miss_rgb))
        depths.append(torch.from_numpy(t[None].astype(np.float32)))
        rgbs.append(torch.from_numpy(rgb.transpose(2, 0, 1).astype(np.float32).copy()))
        c2ws.append(torch.from_numpy(c2w.astype(np.float32)))
        ixts.append(torch.from_numpy(K.astype(np.float32)))
    return depths, rgbs, c2ws, ixts


def fibonacci_sphere(n, radius=1.0):
    """[n, 3] float64 points spread over the sphere."""
    i = np.arange(n, dtype=np.float64) + 0.5
    phi = np.arccos(1.0 - 2.0 * i / n)
    theta = math.pi * (1.0 + 5.0 ** 0.5) * i
    return radius * np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], -1)


FIXTURE_RESOLUTION = 64          # voxel_size = 2 / 64, sdf_trunc = 5 voxel_size
FIXTURE_QUERY_N = 48
FIXTURE_RGB_POINTS = 4096


def fixture_scene():
    """The committed fixture's inputs: a sphere of radius 0.5, 6 views of 64 x 64, focal 80, on a ring of radius 2 at
    height 0.4; the query points are the 48^3 lattice of [-1, 1]^3, the colour points 4096 Fibonacci points at radii
    0.5 (1 + 0.03 sin(0.37 i))."""
    depths, rgbs, c2ws, ixts = sphere_views(ring_eyes(6, 2.0, 0.4), 64, 80.0)
    ax = torch.linspace(-1.0, 1.0, FIXTURE_QUERY_N, dtype=torch.float32)
    query = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    i = np.arange(FIXTURE_RGB_POINTS, dtype=np.float64)
    pts = fibonacci_sphere(FIXTURE_RGB_POINTS, 0.5) * (1.0 + 0.03 * np.sin(0.37 * i))[:, None]
    return depths, rgbs, c2ws, ixts, query, torch.from_numpy(pts.astype(np.float32))


def e2e_scene(nr_views=32, size=128, focal=150.0):
    """The end-to-end test's inputs: the same sphere, `nr_views` views of size x size from Fibonacci points of the
    sphere of radius 2.2, so that every part of the surface faces some camera."""
    return sphere_views(fibonacci_sphere(nr_views, 2.2), size, focal)
