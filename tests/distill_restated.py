"""The virtual-camera rule of teacher distillation (csrc/hemisphere_camera.h, include/volsurfs_hip.h "Teacher
distillation") restated in numpy: the camera rule, the virtual batch and the mixed batch in the kernels'
fp32 operation order, on oracle.packed.Pcg32 and oracle.raygen.pinhole_ray / reel_batch.  CPU only; shared by
tests/test_distill.py.

PARITY UNPINNED: `sample_cameras_on_hemisphere` is mvdatasets' (an empty submodule of the reference checkout); the rule
is this library's own."""
import numpy as np

from oracle.packed import Pcg32
from oracle.raygen import pinhole_ray, reel_batch

f32 = np.float32
ATTEMPTS = 16
CAM_STRIDE = 2 * ATTEMPTS     # draws per camera: a function of the constant, NOT of a patched `attempts` argument


def check_args(radius, up_axis, up_sign, min_height, max_height):
    """What the host entry points refuse."""
    if up_axis not in (0, 1, 2) or up_sign not in (1, -1):
        raise ValueError("up axis")
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError("radius")
    if not (min_height >= 0.0 and min_height <= max_height and max_height < 1.0):
        raise ValueError("heights")


def hemisphere_direction(rng, c, min_height, max_height, attempts=ATTEMPTS):
    """-> ((dx, dy, dz) in the hemisphere's own frame before the division by its length, candidates tried, fell_back).
    `rng` is the call's stream (not moved)."""
    lo, hi = f32(min_height), f32(max_height)
    g = rng.copy()
    g.advance(c * CAM_STRIDE)
    for k in range(attempts):
        a = f32(f32(f32(2.0) * g.next_float()) - f32(1.0))
        b = f32(f32(f32(2.0) * g.next_float()) - f32(1.0))
        s = f32(f32(a * a) + f32(b * b))
        h = np.abs(f32(f32(1.0) - f32(f32(2.0) * s)))
        if s < f32(1.0) and h >= lo and h <= hi:
            t = np.sqrt(f32(f32(1.0) - s))
            return (f32(f32(f32(2.0) * a) * t), f32(f32(f32(2.0) * b) * t), h), k + 1, False
    hm = f32(f32(0.5) * f32(lo + hi))
    return (np.sqrt(f32(f32(1.0) - f32(hm * hm))), f32(0.0), hm), attempts, True


def hemisphere_camera(rng, c, radius, up_axis=2, up_sign=1, min_height=0.0, max_height=0.95, attempts=ATTEMPTS,
                      info=None):
    """Camera c's camera-to-world matrix [3,4] f32.  `info` (a dict) receives "attempts" and "fell_back"."""
    (dx, dy, dz), tried, fell_back = hemisphere_direction(rng, c, min_height, max_height, attempts)
    if info is not None:
        info["attempts"], info["fell_back"] = tried, fell_back
    radius = f32(radius)
    n = np.sqrt(f32(f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz)))
    dx, dy, dz = f32(dx / n), f32(dy / n), f32(dz / n)
    rho = np.sqrt(f32(f32(dx * dx) + f32(dy * dy)))
    sg = f32(up_sign)
    zu, z1, z2 = f32(-f32(sg * dz)), f32(-dx), f32(-dy)
    x1, x2 = f32(f32(-f32(sg * dy)) / rho), f32(f32(sg * dx) / rho)
    col = [(f32(0.0), x1, x2),
           (f32(f32(z1 * x2) - f32(z2 * x1)), f32(-f32(zu * x2)), f32(zu * x1)),
           (zu, z1, z2),
           (f32(radius * f32(sg * dz)), f32(radius * dx), f32(radius * dy))]
    c2w = np.zeros((3, 4), f32)
    for r in range(3):
        w = (r - up_axis + 3) % 3
        for j in range(4):
            c2w[r, j] = col[j][w]
    return c2w


def hemisphere_cameras(rng, C, radius, up_axis=2, up_sign=1, min_height=0.0, max_height=0.95, attempts=ATTEMPTS,
                       stats=None):
    """[C,3,4] f32: what vsa_hemisphere_cameras writes for the stream `rng`.  `stats` (a dict) receives the largest
    number of candidates any camera tried and the number of fallbacks."""
    out = np.zeros((C, 3, 4), f32)
    most, fallbacks, info = 0, 0, {}
    for c in range(C):
        out[c] = hemisphere_camera(rng, c, radius, up_axis, up_sign, min_height, max_height, attempts, info)
        most, fallbacks = max(most, info["attempts"]), fallbacks + int(info["fell_back"])
    if stats is not None:
        stats["max_attempts"], stats["fallbacks"] = most, fallbacks
    return out


def virtual_batch(rng, C, kinv, H, W, B, jitter, radius, up_axis=2, up_sign=1, min_height=0.0, max_height=0.95):
    """(camera_idx [B] i32, rays_o [B,3], rays_d [B,3], points_2d [B,2]) of vsa_virtual_rays_batch."""
    cam = np.zeros(B, np.int32)
    o, d, p = np.zeros((B, 3), f32), np.zeros((B, 3), f32), np.zeros((B, 2), f32)
    poses = {}
    for b in range(B):
        g = rng.copy()
        g.advance(C * CAM_STRIDE + b * (3 + (2 if jitter else 0)))
        c = min(int(f32(g.next_float() * f32(C))), C - 1)
        col = min(int(f32(g.next_float() * f32(W))), W - 1)
        row = min(int(f32(g.next_float() * f32(H))), H - 1)
        jx = jy = f32(0.5)
        if jitter:
            jx, jy = g.next_float(), g.next_float()
        cam[b] = c
        if c not in poses:
            poses[c] = hemisphere_camera(rng, c, radius, up_axis, up_sign, min_height, max_height)
        x, y = f32(f32(col) + jx), f32(f32(row) + jy)
        o[b], d[b] = pinhole_ray(poses[c], kinv, x, y)
        p[b] = (x, y)
    return cam, o, d, p


def mixed_batch(v_rng, C, kinv, radius, hemisphere, n_v, c2w_all, kinv_all, rgbs, masks, n_r, R, jitter, rng,
                with_mask=None):
    """(rays_o, rays_d, gt_rgb, gt_mask or None, virtual camera_idx, real camera_idx) of vsa_distill_rays_batch;
    `hemisphere` = (up_axis, up_sign, min_height, max_height).  gt_rgb[:n_v] is zero here and unwritten on the device."""
    H, W = rgbs.shape[1:3]
    cv, ov, dv, _ = virtual_batch(v_rng, C, kinv, H, W, n_v, True, radius, *hemisphere)
    cr, orr, dr, gt, gm, _ = reel_batch(c2w_all, kinv_all, rgbs, masks, n_r, R, jitter, rng)
    o, d = np.concatenate([ov, orr]), np.concatenate([dv, dr])
    gt_rgb = np.concatenate([np.zeros((n_v, 3), f32), np.repeat(gt, R, 0)])
    want = (masks is not None) if with_mask is None else with_mask
    gt_mask = None
    if want:
        real = np.repeat(gm, R, 0) if gm is not None else np.ones((n_r * R, 1), f32)
        gt_mask = np.concatenate([np.ones((n_v, 1), f32), real])
    return o, d, gt_rgb, gt_mask, cv, cr
