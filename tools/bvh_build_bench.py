"""Host binned-SAH build vs device LBVH build (RayTracer(builder="host" / "device")): build and refit times, the trees'
SAH cost, and the traversal of a full 800x800 frame through each tree (hot: cost feedback on, after warm-up; cold:
cost_feedback = False), with walk_stats().  One JSON line per input, then a table.

    python tools/bvh_build_bench.py [--reps 10] [--frames 20] [--only configs1,configs4,stress]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from volsurfs_amd.camera import pinhole_rays  # noqa: E402
from volsurfs_amd.mesh import TensorMesh, nested_shells, stress_shells  # noqa: E402
from volsurfs_amd.raytrace import RayTracer  # noqa: E402

INPUTS = {
    "configs1": ("nested_shells(K=5, subdiv=6)", lambda: nested_shells(K=5, subdiv=6)),
    "configs4": ("nested_shells(K=7, subdiv=8)", lambda: nested_shells(K=7, subdiv=8)),
    "stress": ("stress_shells(K=5, subdiv=6)", lambda: stress_shells(K=5, subdiv=6)),
}


def device_ms(fn, reps):
    """Median of `reps` runs of fn() between device events on the current stream (fn synchronises itself)."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def frame_ms(rt, o, d, frames, hot):
    rt.cost_feedback = hot
    rt._fb = None
    for _ in range(3):
        rt.trace_all(o, d)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(frames):
        a.record()
        rt.trace_all(o, d)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    rt.cost_feedback = True
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--only", default=",".join(INPUTS))
    args = ap.parse_args()
    o, d = pinhole_rays(800, 800, focal=1111.1, cam_pos=(0.0, 0.0, -1.5))
    rows = []
    for key in args.only.split(","):
        desc, make = INPUTS[key]
        meshes = make()
        ntris = sum(int(m.faces.shape[0]) for m in meshes)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = RayTracer(meshes)
        torch.cuda.synchronize()
        host_s = time.perf_counter() - t0
        for _ in range(2):                                          # warm-up (code objects, allocator)
            RayTracer(meshes, builder="device")
        dev = RayTracer(meshes, builder="device")
        # the build alone: every shell's vsa_bvh_dev_build + vsa_bvh_dev_sizes (the sizes call synchronises)
        from volsurfs_amd import _lib
        import ctypes
        L = _lib.lib()

        def build_only():
            hs = []
            st = _lib.stream_ptr()
            for m in meshes:
                h = ctypes.c_void_p()
                assert L.vsa_bvh_dev_build(m.vertices.data_ptr(), m.faces.data_ptr(), m.vertices.shape[0],
                                           m.faces.shape[0], 4, st, ctypes.byref(h)) == 0
                hs.append(h)
            for h in hs:
                assert L.vsa_bvh_dev_sizes(h, None, None, None) == 0
            build_only.handles = hs

        def build_and_free():
            build_only()
            for h in build_only.handles:
                L.vsa_bvh_dev_destroy(h)
        build_and_free()
        # (allocation included: hipMalloc of the handle's buffers is part of a build)
        dev_build_ms = device_ms(build_and_free, args.reps)
        tracer_ms = device_ms(lambda: RayTracer(meshes, builder="device"), max(3, args.reps // 3))
        moved = [TensorMesh(m.vertices * 1.01, m.faces) for m in meshes]
        refit_ms = device_ms(lambda: dev.refit(moved), args.reps)
        dev.refit(meshes)
        host_refit_s = time.perf_counter()
        host.refit(moved)
        host_refit_s = time.perf_counter() - host_refit_s
        host.refit(meshes)
        row = {
            "input": desc, "triangles": ntris,
            "host_build_s": round(host_s, 3), "host_refit_s": round(host_refit_s, 3),
            "device_build_ms": round(dev_build_ms, 2), "device_tracer_ms": round(tracer_ms, 2),
            "device_refit_ms": round(refit_ms, 2),
            "build_speedup": round(host_s * 1e3 / dev_build_ms, 1),
            "sah_host": [round(c, 1) for c in host.sah_cost()], "sah_device": [round(c, 1) for c in dev.sah_cost()],
            "nodes_host": host.nodes.shape[0], "nodes_device": dev.nodes.shape[0],
            "depth_host": host.max_depth, "depth_device": dev.max_depth,
        }
        for name, rt in (("host", host), ("device", dev)):
            row[f"frame_hot_ms_{name}"] = round(frame_ms(rt, o, d, args.frames, True), 3)
            row[f"frame_cold_ms_{name}"] = round(frame_ms(rt, o, d, args.frames, False), 3)
            row[f"walk_{name}"] = rt.walk_stats(o, d)
        row["frame_hot_ratio"] = round(row["frame_hot_ms_device"] / row["frame_hot_ms_host"], 3)
        row["frame_cold_ratio"] = round(row["frame_cold_ms_device"] / row["frame_cold_ms_host"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del host, dev, meshes, moved
        torch.cuda.empty_cache()
    print()
    print(f"{'input':32s} {'tris':>9s} {'host s':>7s} {'dev ms':>7s} {'x':>6s} {'refit ms':>8s} "
          f"{'SAH h/d':>13s} {'hot h/d ms':>15s} {'cold h/d ms':>15s}")
    for r in rows:
        print(f"{r['input']:32s} {r['triangles']:9d} {r['host_build_s']:7.3f} {r['device_build_ms']:7.2f} "
              f"{r['build_speedup']:6.1f} {r['device_refit_ms']:8.2f} "
              f"{statistics.mean(r['sah_host']):6.1f}/{statistics.mean(r['sah_device']):6.1f} "
              f"{r['frame_hot_ms_host']:7.3f}/{r['frame_hot_ms_device']:7.3f} "
              f"{r['frame_cold_ms_host']:7.3f}/{r['frame_cold_ms_device']:7.3f}")


if __name__ == "__main__":
    main()
