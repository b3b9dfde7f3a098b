"""Host binned-SAH build vs the device LBVH and PLOC builds (RayTracer(builder="host" / "device" / "ploc")): build and
refit times, the trees' SAH cost, depth and size, and the traversal of a full 800x800 frame through each tree (hot: cost
feedback on, after warm-up; cold: cost_feedback = False), with walk_stats().  One JSON line per input, then a table.
--radii 8,16,32 adds PLOC's build time, SAH cost and frame times at each search radius (the default's choice).

    python tools/bvh_build_bench.py [--reps 10] [--frames 20] [--only configs1,configs4,stress] [--radii 8,16,32]
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
    ap.add_argument("--radii", default="", help="PLOC search radii to sweep, e.g. 8,16,32")
    args = ap.parse_args()
    radii = [int(r) for r in args.radii.split(",") if r]
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
        from volsurfs_amd import _lib
        import ctypes
        L = _lib.lib()

        def build_and_free(builder, radius=RayTracer.PLOC_RADIUS):
            """The build alone: every shell's vsa_bvh_dev_build(_ploc) + vsa_bvh_dev_sizes (which synchronises), then
            vsa_bvh_dev_destroy.  (Allocation included: hipMalloc of the handle's buffers is part of a build.)"""
            hs = []
            st = _lib.stream_ptr()
            for m in meshes:
                h = ctypes.c_void_p()
                args_ = (m.vertices.data_ptr(), m.faces.data_ptr(), m.vertices.shape[0], m.faces.shape[0], 4)
                if builder == "ploc":
                    assert L.vsa_bvh_dev_build_ploc(*args_, radius, st, ctypes.byref(h)) == 0
                else:
                    assert L.vsa_bvh_dev_build(*args_, st, ctypes.byref(h)) == 0
                hs.append(h)
            for h in hs:
                assert L.vsa_bvh_dev_sizes(h, None, None, None) == 0
            for h in hs:
                L.vsa_bvh_dev_destroy(h)

        moved = [TensorMesh(m.vertices * 1.01, m.faces) for m in meshes]
        host_refit_s = time.perf_counter()
        host.refit(moved)
        host_refit_s = time.perf_counter() - host_refit_s
        host.refit(meshes)
        host_sah = host.sah_cost()
        row = {"input": desc, "triangles": ntris, "host_build_s": round(host_s, 3),
               "host_refit_s": round(host_refit_s, 3), "sah_host": [round(c, 1) for c in host_sah],
               "nodes_host": host.nodes.shape[0], "depth_host": host.max_depth}
        row["frame_hot_ms_host"] = round(frame_ms(host, o, d, args.frames, True), 3)
        row["frame_cold_ms_host"] = round(frame_ms(host, o, d, args.frames, False), 3)
        row["walk_host"] = host.walk_stats(o, d)
        for name in ("device", "ploc"):
            for _ in range(2):                                      # warm-up (code objects, allocator)
                build_and_free(name)
            rt = RayTracer(meshes, builder=name)
            build_ms = device_ms(lambda: build_and_free(name), args.reps)
            row[f"{name}_build_ms"] = round(build_ms, 2)
            row[f"{name}_tracer_ms"] = round(device_ms(lambda: RayTracer(meshes, builder=name), max(3, args.reps // 3)), 2)
            row[f"{name}_refit_ms"] = round(device_ms(lambda: rt.refit(moved), args.reps), 2)
            rt.refit(meshes)
            row[f"{name}_build_speedup"] = round(host_s * 1e3 / build_ms, 1)
            row[f"sah_{name}"] = [round(c, 1) for c in rt.sah_cost()]
            row[f"sah_ratio_{name}"] = round(statistics.mean(rt.sah_cost()) / statistics.mean(host_sah), 3)
            row[f"nodes_{name}"] = rt.nodes.shape[0]
            row[f"depth_{name}"] = rt.max_depth
            row[f"frame_hot_ms_{name}"] = round(frame_ms(rt, o, d, args.frames, True), 3)
            row[f"frame_cold_ms_{name}"] = round(frame_ms(rt, o, d, args.frames, False), 3)
            row[f"walk_{name}"] = rt.walk_stats(o, d)
            row[f"frame_hot_ratio_{name}"] = round(row[f"frame_hot_ms_{name}"] / row["frame_hot_ms_host"], 3)
            row[f"frame_cold_ratio_{name}"] = round(row[f"frame_cold_ms_{name}"] / row["frame_cold_ms_host"], 3)
            del rt
        for r in radii:
            build_and_free("ploc", r)
            rt = RayTracer(meshes, builder="ploc", ploc_radius=r)
            row.setdefault("ploc_radius_sweep", []).append({
                "radius": r, "build_ms": round(device_ms(lambda: build_and_free("ploc", r), args.reps), 2),
                "sah_ratio": round(statistics.mean(rt.sah_cost()) / statistics.mean(host_sah), 4),
                "depth": rt.max_depth,
                "frame_hot_ms": round(frame_ms(rt, o, d, args.frames, True), 3),
                "frame_cold_ms": round(frame_ms(rt, o, d, args.frames, False), 3)})
            del rt
        print(json.dumps(row), flush=True)
        rows.append(row)
        del host, meshes, moved
        torch.cuda.empty_cache()
    print()
    print(f"{'input':30s} {'tris':>9s} {'host s':>6s} {'dev/ploc ms':>13s} {'refit d/p':>11s} "
          f"{'SAH h/d/p':>17s} {'hot h/d/p ms':>21s} {'cold h/d/p ms':>21s}")
    for r in rows:
        print(f"{r['input']:30s} {r['triangles']:9d} {r['host_build_s']:6.3f} "
              f"{r['device_build_ms']:6.2f}/{r['ploc_build_ms']:6.2f} {r['device_refit_ms']:5.2f}/{r['ploc_refit_ms']:5.2f} "
              f"{statistics.mean(r['sah_host']):5.1f}/{statistics.mean(r['sah_device']):5.1f}/"
              f"{statistics.mean(r['sah_ploc']):5.1f} "
              f"{r['frame_hot_ms_host']:6.3f}/{r['frame_hot_ms_device']:6.3f}/{r['frame_hot_ms_ploc']:6.3f} "
              f"{r['frame_cold_ms_host']:6.3f}/{r['frame_cold_ms_device']:6.3f}/{r['frame_cold_ms_ploc']:6.3f}")


if __name__ == "__main__":
    main()
