"""Camera hits of the K shells by screen-space bins (csrc/shell_raster.hip; include/volsurfs_hip.h "Shell
rasterization"): `trace_all`'s hit records for every sample of one camera, bit for bit, with no ray in
memory and no BVH walk.

* `RayTracer.rasterize(camera, supersample, t_min, out, want_dirs)` / `tracer_rasterize` — (hit_t, hit_slot, hit_uv) as
  `trace_all` lays them out, for the s x s sample grid of `face_view_counts` (s = 1: the unjittered rays of
  `get_camera_rays`).  One blocking read between the setup and the draw call sizes the pair list.
* `rasterize_shells(meshes, camera, ...)` — the same call from a list of meshes.
* `RasterStats` — (behind, straddling, binned, pairs) of a call; the tracer keeps the last one in `raster_stats`.

It reads only the tracer's triangle records and slot ranges: any builder, either node format.
"""
import collections
import ctypes
import math

import torch

from . import _lib
from .raytrace import RayTracer

RasterStats = collections.namedtuple("RasterStats", "behind straddling binned pairs")


def _camera_tensors(camera, dev):
    """(c2w [3, 4], K [3, 3], Kinv [3, 3]) of a `camera.Camera` as contiguous f32 tensors on `dev`."""
    def on(t, *shape):
        t = torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"rasterize: expected a camera tensor of shape {shape}, got {tuple(t.shape)}")
        return t
    return on(camera.c2w, 3, 4), on(camera.intrinsics, 3, 3), on(camera.intrinsics_inv, 3, 3)


def _ranges(tracer):
    K = tracer.nr_meshes
    return (ctypes.c_int32 * K)(*tracer.mesh_tri_offset), (ctypes.c_int32 * K)(*tracer.mesh_nr_tris)


@torch.no_grad()
def tracer_rasterize(tracer, camera, supersample=1, t_min=0.0, out=None, want_dirs=False, stage_ms=None):
    """`RayTracer.rasterize`.  stage_ms: a dict that receives the device ms of {setup, fill, raster} (synchronises;
    measurement only)."""
    s, t_min = int(supersample), float(t_min)
    if not 1 <= s <= 8:
        raise ValueError(f"supersample must be in 1..8, got {supersample}")
    if not (t_min >= 0.0 and math.isfinite(t_min)):
        raise ValueError(f"t_min must be a finite number >= 0 (a face behind the camera is never binned), got {t_min}")
    dev = tracer.device
    if torch.device(dev).type != "cuda":
        raise _lib.VolsurfsHipError("rasterize needs the tracer's meshes on the GPU")
    H, W, K = int(camera.height), int(camera.width), tracer.nr_meshes
    if H < 1 or W < 1:
        raise ValueError(f"rasterize: a camera of {H} x {W} pixels")
    N = H * W * s * s
    if N >= 1 << 31:
        raise _lib.VolsurfsHipError(f"{H} x {W} pixels at supersample {s}: 2^31 samples or more; render the frame in parts")
    c2w, k, kinv = _camera_tensors(camera, dev)
    if out is not None:
        hit_t, hit_slot, hit_uv = out
        _lib.check_f32(hit_t, K, N)
        _lib.check_f32(hit_uv, K, N, 2)
        if hit_slot.dtype != torch.int32 or tuple(hit_slot.shape) != (K, N) or not hit_slot.is_contiguous():
            raise _lib.VolsurfsHipError("rasterize: out[1] must be a contiguous int32 [K, N] tensor")
    else:
        hit_t = torch.empty(K, N, device=dev)
        hit_slot = torch.empty(K, N, dtype=torch.int32, device=dev)
        hit_uv = torch.empty(K, N, 2, device=dev)
    rays_d = torch.empty(N, 3, device=dev) if want_dirs else None
    nr_slots = int(tracer.tris.shape[0])
    first, count = _ranges(tracer)
    nbytes = _lib.workspace_bytes("vsa_shell_raster_workspace_bytes", nr_slots, K, H, W, s)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    head = (tracer.tris, nr_slots, first, count, K, c2w, k, kinv, H, W, s, t_min, ws, nbytes)
    stats = (ctypes.c_longlong * 4)()
    st = _lib.stream_ptr()
    if stage_ms is not None:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
    _lib.call("vsa_shell_raster_setup", *head, stats, st)                 # (one blocking read)
    if stage_ms is not None:
        ev[1].record()
        ev[1].synchronize()
        stage_ms["setup"] = ev[0].elapsed_time(ev[1])
    tracer.raster_stats = RasterStats(*(int(v) for v in stats))
    nr_pairs = tracer.raster_stats.pairs
    pairs = torch.empty(nr_pairs, dtype=torch.int32, device=dev) if nr_pairs else None
    ms = _lib.stage_array(("fill", "raster"), stage_ms)
    _lib.call("vsa_shell_raster_draw", *head, nr_pairs, pairs, hit_t, hit_slot, hit_uv, rays_d, ms, st)
    _lib.stage_update(("fill", "raster"), stage_ms, ms)
    return (hit_t, hit_slot, hit_uv, rays_d) if want_dirs else (hit_t, hit_slot, hit_uv)


def rasterize_shells(meshes, camera, supersample=1, t_min=0.0, out=None, want_dirs=False, tracer=None):
    """`RayTracer.rasterize` from a list of K cuda TensorMeshes.  `tracer`: a RayTracer of these meshes (default: one
    is built on the device)."""
    meshes = list(meshes)
    if tracer is None and any(m.vertices.device.type != "cuda" for m in meshes):
        raise _lib.VolsurfsHipError("rasterize_shells needs the meshes on the GPU")
    tracer = RayTracer.over(meshes if tracer is None else tracer, len(meshes))
    return tracer_rasterize(tracer, camera, supersample, t_min, out, want_dirs)


def check_hits_mode(hits):
    if hits not in ("trace", "raster"):
        raise ValueError(f'hits must be "trace" or "raster", got {hits!r}')
    return hits


def grid_side(nr_rays_per_pixel):
    """s with s * s == nr_rays_per_pixel, or ValueError: the raster path samples a pixel on an s x s grid."""
    R = int(nr_rays_per_pixel)
    s = math.isqrt(R) if R > 0 else 0
    if s < 1 or s * s != R or s > 8:
        raise ValueError(f'hits="raster" puts a pixel\'s rays on an s x s grid, s in 1..8: nr_rays_per_pixel = {R} is '
                         "no such square")
    return s


def camera_hits(tracer, camera, supersample=1, t_min=0.0):
    """What a render needs in place of `get_camera_rays` + `trace_all`: (rays_o [N, 3], rays_d [N, 3], (hit_t,
    hit_slot, hit_uv)); the origins are the camera centre, expanded without a copy."""
    hit_t, hit_slot, hit_uv, rays_d = tracer_rasterize(tracer, camera, supersample, t_min, want_dirs=True)
    rays_o = camera.c2w.to(rays_d.device)[:, 3].expand(rays_d.shape[0], 3)
    return rays_o, rays_d, (hit_t, hit_slot, hit_uv)


__all__ = ["RasterStats", "tracer_rasterize", "rasterize_shells", "camera_hits"]
