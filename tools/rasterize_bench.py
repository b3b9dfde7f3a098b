"""Shell rasterization (volsurfs_amd.rasterize, csrc/shell_raster.hip) against the calls that existed
before it, for the same samples, in one process on one GPU.

Cases (--cases, comma separated):
  lobed     K = 5 level sets of the noisy lobed SDF of tools/simplify_bench.py on a 512^3 grid, each simplified to 0.025
            of its faces (about 16 000 each), 800 x 800: an orbit view and a view from inside, supersample 1 and 2;
  dense     one unsimplified level set of that tool's sphere on the 512^3 grid (sub-pixel triangles), the orbit view;
  frame     BASELINE configs[4]'s frame: 1920 x 1080, K = 7 icosphere shells of subdiv 8 (1.31 M faces each);
  render    whole renders: render_baked_camera of K = 5 baked subdiv-6 shells at 800 x 800 under both `hits` values.

Timed per case, --reps times after a warm-up, the paths alternating inside every repetition, device time from events,
min / median / max in ms:
  raygen_trace  get_camera_rays + RayTracer.trace_all (its default launch-order feedback): the composition before this
                change.  At supersample 2 it traces the pixel centres of the doubled image with Kinv . diag(1/2, 1/2, 1):
                the same rays bit for bit, in another order;
  trace         trace_all alone on those rays, already in memory;
  raster        RayTracer.rasterize, the whole call (workspace and pair-list allocation and the blocking read included);
and once per case, from the call's own stage events: setup (with the scan and the read), fill, raster pass.
The hit records of the two paths are compared (they must be equal bit for bit).  Recorded beside the times: RasterStats,
pairs per (shell, tile), triangle tests per (sample, shell) of the raster pass (its tile's list plus the shell's
straddling faces) and of the trace (walk_stats' tri_tests).  Needs a GPU; writes one JSON file.

    python tools/rasterize_bench.py [--out profiles/rasterize.json] [--cases lobed,dense,frame,render] [--reps 7]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, DELTA, RATIO = 5, 0.0025, 0.025


def _doubled(c):
    """The camera of the doubled image whose pixel centres are the 2 x 2 sub-pixel samples of `c`."""
    import torch
    from volsurfs_amd.camera import Camera
    d = Camera(c.intrinsics, torch.cat([c.c2w.cpu(), torch.tensor([[0.0, 0.0, 0.0, 1.0]])]), 2 * c.height, 2 * c.width)
    d.c2w = c.c2w
    d.intrinsics_inv = (c.intrinsics_inv * torch.tensor([0.5, 0.5, 1.0], device=c.intrinsics_inv.device)).contiguous()
    return d


def _alternating(paths, reps):
    """{name: {min, median, max}} of the callables of `paths`, run one after the other inside every repetition."""
    import torch
    for fn in paths.values():
        fn()                                                # warm-up: code objects, allocator, feedback buffers
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {k: {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}
            for k, v in ms.items()}


def _hits_case(tracer, cam, s, reps):
    import torch
    from volsurfs_amd.camera import get_camera_rays
    from volsurfs_amd.rasterize import tracer_rasterize
    H, W, Kk = cam.height, cam.width, tracer.nr_meshes
    ray_cam = cam if s == 1 else _doubled(cam)
    o, d, _ = get_camera_rays(ray_cam)
    held = {}

    def raygen_trace():
        oo, dd, _ = get_camera_rays(ray_cam)
        held["trace"] = tracer.trace_all(oo, dd)

    def trace():
        held["trace"] = tracer.trace_all(o, d)

    def raster():
        held["raster"] = tracer.rasterize(cam, supersample=s)

    row = _alternating({"raygen_trace": raygen_trace, "trace": trace, "raster": raster}, reps)
    stage = {}
    tracer_rasterize(tracer, cam, s, stage_ms=stage)
    row["raster_stage_ms"] = {k: round(v, 3) for k, v in stage.items()}
    # equality: raster sample n = ((row W + col) s^2 + j s + i) is pixel (row s + j, col s + i) of the doubled image
    n = torch.arange(H * W * s * s, device="cuda")
    pixel, sub = n // (s * s), n % (s * s)
    at = ((pixel // W) * s + sub // s) * (W * s) + (pixel % W) * s + sub % s
    row["records_equal"] = bool(all(torch.equal(r.view(torch.int32), t[:, at].contiguous().view(torch.int32))
                                    for r, t in zip(held["raster"], held["trace"])))
    st = tracer.raster_stats
    tiles = math.ceil(H * s / 8) * math.ceil(W * s / 8)
    walk = tracer.walk_stats(o, d)
    row.update({"samples": H * W * s * s, "hits": int((held["raster"][1] >= 0).sum()), "stats": st._asdict(),
                "pairs_per_tile": round(st.pairs / (Kk * tiles), 2),
                "raster_tri_tests_per_sample": round(st.pairs / (Kk * tiles) + st.straddling / Kk, 2),
                "trace_tri_tests_per_sample": round(walk["tri_tests"] / (H * W * s * s * Kk), 2),
                "trace_node_visits_per_sample": round(walk["lane_visits"] / (H * W * s * s * Kk), 2),
                "raygen_trace_over_raster": round(row["raygen_trace"]["median"] / row["raster"]["median"], 2),
                "trace_over_raster": round(row["trace"]["median"] / row["raster"]["median"], 2)})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rasterize.json"))
    ap.add_argument("--cases", default="lobed,dense,frame,render")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--size", type=int, default=800)
    a = ap.parse_args()
    cases = a.cases.split(",")

    import torch
    if not torch.cuda.is_available():
        sys.exit("rasterize_bench needs a GPU")
    from volsurfs_amd.camera import Camera
    from volsurfs_amd.raytrace import RayTracer

    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "cases": {}}

    def record(name, row):
        result["cases"][name] = row
        print(json.dumps({name: row}), flush=True)
        if row.get("records_equal") is False:
            sys.exit(f"{name}: the raster records differ from the trace's")

    size = a.size
    orbit = Camera.look_at((1.5 * math.cos(math.radians(30.0)), -0.75, 0.0), focal=float(size), height=size, width=size)
    inside = Camera.look_at((0.05, 0.02, 0.10), (1.0, 0.3, 0.2), focal=0.5 * size, height=size, width=size)
    if "lobed" in cases or "dense" in cases:
        from tools.simplify_bench import _fields
        from volsurfs_amd import isosurface as iso
        from volsurfs_amd.simplify import simplify_mesh
        if "lobed" in cases:
            full, _ = iso.extract_level_sets(_fields()["lobed_noisy"], a.n, K, delta_surfs=DELTA)
            meshes = [simplify_mesh(m, RATIO) for m in full]
            tracer = RayTracer(meshes, builder="device")
            faces = [int(m.faces.shape[0]) for m in meshes]
            for view, cam in (("orbit", orbit), ("inside", inside)):
                for s in (1, 2):
                    record(f"lobed_{view}_s{s}", dict(_hits_case(tracer, cam, s, a.reps), faces=faces, K=K,
                                                      height=size, width=size, supersample=s))
            del tracer, meshes, full
        if "dense" in cases:
            dense, _ = iso.extract_level_sets(_fields()["sphere"], a.n, 1, delta_surfs=DELTA)
            tracer = RayTracer(dense, builder="device")
            record("dense_orbit_s1", dict(_hits_case(tracer, orbit, 1, a.reps), faces=[int(dense[0].faces.shape[0])],
                                          K=1, height=size, width=size, supersample=1))
            del tracer, dense
    if "frame" in cases:
        from volsurfs_amd._lib import VolsurfsHipError
        from volsurfs_amd.mesh import nested_shells
        meshes = nested_shells(K=7, subdiv=8)
        tracer = RayTracer(meshes, builder="device")
        cam = Camera.look_at((0.0, 0.0, -1.5), focal=1080.0, height=1080, width=1920)
        try:
            record("frame_1080p_K7_subdiv8", dict(_hits_case(tracer, cam, 1, a.reps), K=7, height=1080, width=1920,
                                                  faces=[int(m.faces.shape[0]) for m in meshes], supersample=1))
        except VolsurfsHipError as e:
            record("frame_1080p_K7_subdiv8", {"error": str(e), "stats": tracer.raster_stats and tracer.raster_stats._asdict()})
        del tracer, meshes
    if "render" in cases:
        from volsurfs_amd.mesh import nested_shells
        from volsurfs_amd.methods import VolSurfs
        m = VolSurfs(nested_shells(K=5, subdiv=6), max_rays=size * size, bg_color=(1.0, 1.0, 1.0))
        m.bake()
        cam = Camera.look_at((0.0, 0.0, -1.5), focal=float(size), height=size, width=size)
        held = {}
        row = _alternating({"hits_trace": lambda: held.update(trace=m.render_baked_camera(cam)),
                            "hits_raster": lambda: held.update(raster=m.render_baked_camera(cam, hits="raster"))}, a.reps)
        row["buffers_equal"] = bool(all(torch.equal(held["trace"][k], held["raster"][k]) for k in held["trace"]))
        row["trace_over_raster"] = round(row["hits_trace"]["median"] / row["hits_raster"]["median"], 2)
        row.update({"K": 5, "subdiv": 6, "height": size, "width": size, "stats": m.raytracer.raster_stats._asdict()})
        record("render_baked_camera_800", row)
        if not row["buffers_equal"]:
            sys.exit("render_baked_camera: the two hits values give different buffers")

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
