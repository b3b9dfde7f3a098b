"""numpy restatement of the dataset loader's rules, written from their description and sharing no code with
volsurfs_amd/datasets.py or csrc/image_prepare.hip:

* `prepare` — the image rule of include/volsurfs_hip.h "Image preparation": alpha over a background, box subsampling,
  the mask; float32 operation for float32 operation, so that the kernel is compared bit for bit.
* `blender_camera` — a Blender-format frame to intrinsics and a camera-to-world pose.
* `dtu_camera` — a NeuS / IDR world_mat . scale_mat to intrinsics, rotation and centre.
"""
import math

import numpy as np

F32 = np.float32


def prepare(src, mask, s, bg):
    """src [C,H0,W0,ch] u8, mask [C,H0,W0] u8 or None, s >= 1, bg 3 floats -> (rgb [C,H,W,3] f32, mask [C,H,W] f32 or
    None)."""
    src = np.asarray(src)
    C, H0, W0, ch = src.shape
    H, W, n = H0 // s, W0 // s, s * s
    blocks = src[:, :H * s, :W * s].reshape(C, H, s, W, s, ch).astype(np.int64)
    if ch == 4:
        colour, a = blocks[..., :3], blocks[..., 3]
    elif ch == 3:
        colour, a = blocks, np.full(blocks.shape[:-1], 255, np.int64)
    else:
        colour, a = np.repeat(blocks, 3, axis=-1), np.full(blocks.shape[:-1], 255, np.int64)
    A = a.sum(axis=(2, 4))
    P = (colour * a[..., None]).sum(axis=(2, 4))
    assert P.max(initial=0) < 2 ** 24
    alpha = A.astype(F32) / F32(255 * n)
    prem = P.astype(F32) / F32(65025 * n)
    rest = F32(1.0) - alpha
    assert alpha.dtype == F32 and prem.dtype == F32 and rest.dtype == F32
    bg = np.asarray(bg, F32)
    rgb = prem + rest[..., None] * bg           # two float32 operations, each rounded
    assert rgb.dtype == F32
    if mask is not None:
        M = np.asarray(mask)[:, :H * s, :W * s].reshape(C, H, s, W, s).astype(np.int64).sum(axis=(2, 4))
        out_mask = M.astype(F32) / F32(255 * n)
    elif ch == 4:
        out_mask = alpha
    else:
        out_mask = None
    return rgb, out_mask


def blender_camera(transform_matrix, camera_angle_x, width, height):
    """(K [3,3], c2w [4,4]) f64: the file's camera looks down -z with y up; ours looks down +z with y down."""
    fx = 0.5 * width / math.tan(0.5 * camera_angle_x)
    K = np.array([[fx, 0.0, 0.5 * width], [0.0, fx, 0.5 * height], [0.0, 0.0, 1.0]])
    c2w = np.array(transform_matrix, np.float64).reshape(4, 4)
    c2w[:, 1] = -c2w[:, 1]
    c2w[:, 2] = -c2w[:, 2]
    return K, c2w


def dtu_camera(world_mat, scale_mat):
    """(K, R world-to-camera, c) f64 of P = (world_mat . scale_mat)[:3, :4] = K [R | -R c]: Gram-Schmidt on the rows of
    M = P[:, :3] from the last one up (M = K R with K upper triangular: row 2 of M is K22 r2, row 1 is K11 r1 + K12 r2,
    row 0 is K00 r0 + K01 r1 + K02 r2)."""
    P = (np.asarray(world_mat, np.float64) @ np.asarray(scale_mat, np.float64))[:3, :4]
    if np.linalg.det(P[:, :3]) < 0:
        P = -P
    M = P[:, :3]
    K, R = np.zeros((3, 3)), np.zeros((3, 3))
    K[2, 2] = np.linalg.norm(M[2])
    R[2] = M[2] / K[2, 2]
    K[1, 2] = M[1] @ R[2]
    v = M[1] - K[1, 2] * R[2]
    K[1, 1] = np.linalg.norm(v)
    R[1] = v / K[1, 1]
    K[0, 2], K[0, 1] = M[0] @ R[2], M[0] @ R[1]
    v = M[0] - K[0, 2] * R[2] - K[0, 1] * R[1]
    K[0, 0] = np.linalg.norm(v)
    R[0] = v / K[0, 0]
    c = -np.linalg.inv(M) @ P[:, 3]
    return K / K[2, 2], R, c
