"""Pinhole ray generation for the synthetic bench / tests (the reference takes
its rays from mvdatasets.get_camera_rays, base_method.py:389-394, which is not
in the tree; SURVEY §8f row 2 lists a device ray generator as 'next')."""
import torch


def pinhole_rays(H, W, focal, cam_pos=(0.0, 0.0, -1.5), device="cuda"):
    """Row-major pixel-centre rays of a camera at cam_pos looking down +z."""
    ys, xs = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float32),
                            torch.arange(W, device=device, dtype=torch.float32), indexing="ij")
    dx = (xs + 0.5 - 0.5 * W) / focal
    dy = (ys + 0.5 - 0.5 * H) / focal
    d = torch.stack([dx, dy, torch.ones_like(dx)], -1).reshape(-1, 3)
    d = torch.nn.functional.normalize(d, dim=-1).contiguous()
    o = torch.tensor(cam_pos, device=device, dtype=torch.float32).expand(H * W, 3).contiguous()
    return o, d


# ---------------------------------------------------------------------------
# device ray generation + the training-ray sampler.  The call shapes are
# the reference's (mvdatasets `get_camera_rays`, base_method.py:389-394;
# `TensorReel.get_next_rays_batch`, trainer.py:176-190); mvdatasets itself is an empty
# submodule in the reference checkout, so the pinhole arithmetic is this library's own
# definition (csrc/raygen.hip, restated in oracle/raygen.py) — parity unpinned.
import ctypes

from . import _lib
from .volsurfs import _Pcg32State


class Camera:
    """Pinhole camera: `intrinsics` [3,3] (pixels), `pose` = camera-to-world [3,4] or [4,4]
    (columns: camera x right, y down, z forward; last column the centre), `height`, `width`."""

    def __init__(self, intrinsics, pose, height, width, device="cuda"):
        K = torch.as_tensor(intrinsics, dtype=torch.float64).reshape(3, 3)
        c2w = torch.as_tensor(pose, dtype=torch.float64)
        if c2w.shape not in ((3, 4), (4, 4)):
            raise ValueError("pose must be [3,4] or [4,4]")
        self.height, self.width = int(height), int(width)
        self.intrinsics = K.to(torch.float32)
        self.intrinsics_inv = torch.linalg.inv(K).to(torch.float32).contiguous().to(device)
        self.c2w = c2w[:3, :4].to(torch.float32).contiguous().to(device)

    @staticmethod
    def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, -1.0, 0.0), focal=800.0, height=800, width=800,
                device="cuda"):
        eye, target, up = (torch.tensor(v, dtype=torch.float64) for v in (eye, target, up))
        z = torch.nn.functional.normalize(target - eye, dim=0)
        x = torch.nn.functional.normalize(torch.linalg.cross(-up, z), dim=0)
        y = torch.linalg.cross(z, x)
        pose = torch.stack([x, y, z, eye], 1)
        K = [[focal, 0, 0.5 * width], [0, focal, 0.5 * height], [0, 0, 1]]
        return Camera(K, pose, height, width, device)


_m_rng = _Pcg32State()   # one process-wide stream, advanced by 2^32 per jittered call like the
                         # reference's own samplers (src/RaySampler.cu:139-142)


def get_camera_rays(camera, nr_rays_per_pixel=1, jitter_pixels=False, device="cuda"):
    """-> rays_o [H*W*R,3], rays_d [H*W*R,3], points_2d [H*W*R,2]; pixel-major, the R rays of a
    pixel consecutive (what BaseMethod.render's supersample mean expects)."""
    n = camera.height * camera.width * int(nr_rays_per_pixel)
    o = torch.empty(n, 3, device=device)
    d = torch.empty(n, 3, device=device)
    p = torch.empty(n, 2, device=device)
    _lib.call("vsa_camera_rays", camera.c2w, camera.intrinsics_inv, camera.height, camera.width,
              int(nr_rays_per_pixel), bool(jitter_pixels), ctypes.c_uint64(_m_rng.state),
              ctypes.c_uint64(_m_rng.inc), o, d, p, _lib.stream_ptr())
    if jitter_pixels:
        _m_rng.advance()
    return o, d, p


class TensorReel:
    """All training views resident in HBM (a 100-view 800x800 fp32 set is 0.77 GB of 288):
    `get_next_rays_batch` draws (camera, pixel) pairs and emits rays + ground truth in one
    launch, with no host round trip inside the training loop."""

    def __init__(self, cameras, rgbs, masks=None, device="cuda"):
        if not cameras:
            raise ValueError("TensorReel needs at least one camera")
        self.height, self.width = cameras[0].height, cameras[0].width
        if any((c.height, c.width) != (self.height, self.width) for c in cameras):
            raise ValueError("all cameras of a reel must have the same resolution")
        self.c2w = torch.stack([c.c2w for c in cameras]).contiguous()
        self.intrinsics_inv = torch.stack([c.intrinsics_inv for c in cameras]).contiguous()
        self.intrinsics = torch.stack([c.intrinsics for c in cameras])      # [C,3,3] on the host, as given
        C = len(cameras)
        self.rgbs = torch.as_tensor(rgbs, dtype=torch.float32).to(device).contiguous()
        if self.rgbs.shape != (C, self.height, self.width, 3):
            raise ValueError("rgbs must be [C,H,W,3]")
        self.masks = None
        if masks is not None:
            self.masks = torch.as_tensor(masks, dtype=torch.float32).to(device).reshape(
                C, self.height, self.width).contiguous()
        self.nr_cameras = C
        self.rng = _Pcg32State()

    def get_next_rays_batch(self, batch_size=512, jitter_pixels=False, nr_rays_per_pixel=1):
        """-> (camera_idx [B], rays_o [B*R,3], rays_d [B*R,3], {"rgb": [B,3], "mask": [B,1]},
        points_2d [B*R,2])."""
        B, R = int(batch_size), int(nr_rays_per_pixel)
        dev = self.rgbs.device
        cam = torch.empty(B, dtype=torch.int32, device=dev)
        o = torch.empty(B * R, 3, device=dev)
        d = torch.empty(B * R, 3, device=dev)
        p = torch.empty(B * R, 2, device=dev)
        vals = {"rgb": torch.empty(B, 3, device=dev)}
        if self.masks is not None:
            vals["mask"] = torch.empty(B, 1, device=dev)
        _lib.call("vsa_reel_next_rays_batch", self.c2w, self.intrinsics_inv, self.rgbs, self.masks,
                  self.nr_cameras, self.height, self.width, B, R, bool(jitter_pixels),
                  ctypes.c_uint64(self.rng.state), ctypes.c_uint64(self.rng.inc), cam, o, d,
                  vals["rgb"], vals.get("mask"), p, _lib.stream_ptr())
        self.rng.advance()
        return cam, o, d, vals, p


# ---------------------------------------------------------------------------
# Teacher distillation (trainer.py:132-166 of the reference): virtual cameras on a hemisphere around the scene, drawn
# on the device.  `sample_cameras_on_hemisphere` is mvdatasets' (an empty submodule): the rule is this library's own
# (csrc/hemisphere_camera.h, restated in tests/distill_restated.py) — parity unpinned, call shapes the
# reference's.
HEMISPHERE_ATTEMPTS = 16                         # csrc/hemisphere_camera.h
HEMISPHERE_CAM_STRIDE = 2 * HEMISPHERE_ATTEMPTS  # draws of the call's stream that one camera owns

_hemisphere_rng = _Pcg32State()   # the stream of sample_cameras_on_hemisphere(rng=None), advanced by 2^32 per call


def _check_hemisphere(radius, nr_cameras, up_axis, up_sign, min_height, max_height):
    if int(nr_cameras) < 0:
        raise ValueError("nr_cameras must be >= 0")
    if up_axis not in (0, 1, 2) or up_sign not in (1, -1):
        raise ValueError("up_axis must be 0, 1 or 2 and up_sign +1 or -1")
    if not 0.0 < float(radius) < float("inf"):
        raise ValueError("radius must be positive and finite")
    if not (float(min_height) >= 0.0 and float(min_height) <= float(max_height) and float(max_height) < 1.0):
        raise ValueError("heights must satisfy 0 <= min_height <= max_height < 1 (at height 1 the view direction is "
                         "the up axis and the pose is undefined)")


def _hemisphere_poses(rng, nr_cameras, radius, up_axis, up_sign, min_height, max_height, device):
    c2w = torch.empty(int(nr_cameras), 3, 4, device=device)
    _lib.call("vsa_hemisphere_cameras", int(nr_cameras), float(radius), int(up_axis), int(up_sign), float(min_height),
              float(max_height), ctypes.c_uint64(rng.state), ctypes.c_uint64(rng.inc), c2w, _lib.stream_ptr())
    return c2w


def _cameras_of(intrinsics, c2w, height, width, device):
    return [Camera(intrinsics, pose, height, width, device) for pose in c2w.cpu()]


def sample_cameras_on_hemisphere(intrinsics, width, height, radius, nr_cameras=100, up_axis=2, up_sign=1,
                                 min_height=0.0, max_height=0.95, rng=None, device="cuda"):
    """-> list of `nr_cameras` Camera on the hemisphere of `radius` around the origin, uniform by area over the band
    of heights [min_height, max_height] (fractions of the radius along the up axis), each looking at the origin with
    the up axis as image-up; all share `intrinsics` [3,3], `height`, `width`.  The argument names of the reference's
    call (trainer.py:138-144) come first.

    The hemisphere's height axis is the signed world axis `up_sign * e[up_axis]`.  The default is +z: what
    `datasets.load_scene` produces for Blender scenes, whose poses keep Blender's z-up world (`opengl_to_camera` flips
    the camera's axes, not the world's; `rotate_scene_x_axis_deg` is 0 by default).  A DTU scene has no canonical up:
    give the axis.  `rng`: a `_Pcg32State` (advanced by 2^32 by this call); None takes this module's own stream."""
    _check_hemisphere(radius, nr_cameras, up_axis, up_sign, min_height, max_height)
    rng = _hemisphere_rng if rng is None else rng
    c2w = _hemisphere_poses(rng, nr_cameras, radius, up_axis, up_sign, min_height, max_height, device)
    rng.advance()
    return _cameras_of(intrinsics, c2w, height, width, device)


class VirtualCameras:
    """The virtual half of a distilled training batch (trainer.py:132-159): every call of `get_next_rays_batch`
    stands for `nr_cameras` FRESH cameras on the hemisphere and a batch of jittered rays drawn from them, as one launch
    with no pose table in memory — each lane makes its camera's pose in registers from the call's PCG32 stream.  The
    stream advances by 2^32 per call, like the reel's."""

    def __init__(self, intrinsics, height, width, radius, nr_cameras=100, up_axis=2, up_sign=1, min_height=0.0,
                 max_height=0.95, device="cuda"):
        if int(nr_cameras) < 1 or int(height) < 1 or int(width) < 1:
            raise ValueError("VirtualCameras needs nr_cameras, height and width >= 1")
        _check_hemisphere(radius, nr_cameras, up_axis, up_sign, min_height, max_height)
        K = torch.as_tensor(intrinsics, dtype=torch.float64).reshape(3, 3).cpu()
        self._K = K                                   # fp64, as given: cameras() inverts what this inverts
        self.intrinsics = K.to(torch.float32)
        self.intrinsics_inv = torch.linalg.inv(K).to(torch.float32).contiguous().to(device)   # as Camera's
        self.height, self.width, self.nr_cameras = int(height), int(width), int(nr_cameras)
        self.radius, self.up_axis, self.up_sign = float(radius), int(up_axis), int(up_sign)
        self.min_height, self.max_height = float(min_height), float(max_height)
        self.device = device
        self.rng = _Pcg32State()

    def _hemisphere_args(self):
        return (self.radius, self.up_axis, self.up_sign, self.min_height, self.max_height)

    def get_next_rays_batch(self, batch_size=512, jitter_pixels=True):
        """-> (camera_idx [B] int32, rays_o [B,3], rays_d [B,3], points_2d [B,2]); one ray per sample."""
        B = int(batch_size)
        cam = torch.empty(B, dtype=torch.int32, device=self.device)
        o, d = torch.empty(B, 3, device=self.device), torch.empty(B, 3, device=self.device)
        p = torch.empty(B, 2, device=self.device)
        _lib.call("vsa_virtual_rays_batch", self.intrinsics_inv, self.nr_cameras, self.height, self.width,
                  *self._hemisphere_args(), B, bool(jitter_pixels), ctypes.c_uint64(self.rng.state),
                  ctypes.c_uint64(self.rng.inc), cam, o, d, p, _lib.stream_ptr())
        self.rng.advance()
        return cam, o, d, p

    def poses(self):
        """c2w [C,3,4] of the cameras the NEXT call draws from (the stream does not move)."""
        return _hemisphere_poses(self.rng, self.nr_cameras, *self._hemisphere_args(), self.device)

    def cameras(self):
        """The Camera list the next call draws from: the same bits as the poses its rays are made with."""
        return _cameras_of(self._K, self.poses(), self.height, self.width, self.device)


def mixed_rays_batch(virtual, reel, n_virtual, n_real, jitter_pixels=True, nr_rays_per_pixel=1, with_mask=None):
    """The batch [virtual | real] of a distilled iteration (trainer.py:132-214) as ONE launch into single allocations:
    `n_virtual` jittered rays of `virtual` (a VirtualCameras), then `n_real` samples of `reel` with `nr_rays_per_pixel`
    rays each, drawn exactly as `virtual.get_next_rays_batch(n_virtual)` and `reel.get_next_rays_batch(n_real,
    jitter_pixels, nr_rays_per_pixel)` draw them; both streams advance as those two calls advance them.

    -> (rays_o [N,3], rays_d [N,3], gt_rgb [N,3], gt_mask [N,1] or None, virtual_camera_idx [n_virtual],
    real_camera_idx [n_real]), N = n_virtual + n_real * nr_rays_per_pixel.  Ground truth is per ray: the real half
    repeats its pixel's value for each of its rays.  gt_rgb[:n_virtual] is NOT written (the teacher's render goes
    there).  gt_mask is [ones | the reel's masks]; `with_mask` None gives it when the reel has masks, True always
    (ones for a reel without masks), False never."""
    nv, nr, R = int(n_virtual), int(n_real), int(nr_rays_per_pixel)
    if nv < 0 or nr < 0 or R < 1:
        raise ValueError("mixed_rays_batch: n_virtual, n_real >= 0 and nr_rays_per_pixel >= 1")
    if (virtual.height, virtual.width) != (reel.height, reel.width):
        raise ValueError("mixed_rays_batch: the virtual cameras and the reel must have the same resolution")
    dev = reel.rgbs.device
    n = nv + nr * R
    o, d, gt = (torch.empty(n, 3, device=dev) for _ in range(3))
    want_mask = (reel.masks is not None) if with_mask is None else bool(with_mask)
    mask = torch.empty(n, 1, device=dev) if want_mask else None
    cam_v = torch.empty(nv, dtype=torch.int32, device=dev)
    cam_r = torch.empty(nr, dtype=torch.int32, device=dev)
    _lib.call("vsa_distill_rays_batch", virtual.intrinsics_inv, virtual.nr_cameras, *virtual._hemisphere_args(), nv,
              True, ctypes.c_uint64(virtual.rng.state), ctypes.c_uint64(virtual.rng.inc), reel.c2w,
              reel.intrinsics_inv, reel.rgbs, reel.masks, reel.nr_cameras, reel.height, reel.width, nr, R,
              bool(jitter_pixels), ctypes.c_uint64(reel.rng.state), ctypes.c_uint64(reel.rng.inc), cam_v, cam_r, o, d,
              gt, mask, None, _lib.stream_ptr())
    virtual.rng.advance()
    reel.rng.advance()
    return o, d, gt, mask, cam_v, cam_r
