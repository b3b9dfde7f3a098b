"""Face visibility (volsurfs_amd.visibility, csrc/face_visibility.hip): the fused counting launch against
the composition of the calls that existed before it, in one process on one GPU.

Workload: K = 5 level sets of the noisy lobed SDF of tools/simplify_bench.py on a 512^3 grid at the reference's
delta_surfs = 0.0025, each simplified to 0.025 of its faces (the shells tools/atlas_bench.py atlases: about 16 000
faces each), one device-built tracer; 100 cameras on an orbit of radius 1.5 at 30 degrees elevation, 800 x 800, focal
800; supersample 1 and 2.

Timed, each 10 times after a warm-up, device time from events around the whole path, min / median / max in ms:
  fused        vsa_face_view_counts, one launch over all views (cameras stacked once, outside the window), for both tile
               shapes ("8x8", "row");
  fused_per_view  the same kernel launched once per view (default tile);
  composition  per view: get_camera_rays -> RayTracer.trace_all -> the hits' original face ids gathered -> one
               torch.bincount over the K shells.  (The misses are masked out first: sent to a spare bin instead, two
               million adds per view land on one address and the composition takes 25 ms per view.)  At supersample 2
               the composition traces the pixel centres of the doubled image with Kinv . diag(1/2, 1/2, 1): the same
               rays bit for bit.
The counts of every path are compared (they must be equal), and the culled fraction at min_hits = 1 with rings 0 and 1
is recorded.  Needs a GPU; writes one JSON file.

    python tools/visibility_bench.py [--out profiles/visibility.json] [--views 100] [--size 800] [--n 512] [--reps 10]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, DELTA, RATIO = 5, 0.0025, 0.025


def _orbit(nr_views, size, focal, radius=1.5, elevation_deg=30.0):
    from volsurfs_amd.camera import Camera
    el = math.radians(elevation_deg)
    cams = []
    for i in range(nr_views):
        az = 2.0 * math.pi * i / nr_views
        eye = (radius * math.cos(el) * math.cos(az), -radius * math.sin(el), radius * math.cos(el) * math.sin(az))
        cams.append(Camera.look_at(eye, focal=focal, height=size, width=size))
    return cams


def _doubled(cams):
    """The cameras of the doubled image whose pixel centres are the 2 x 2 sub-pixel samples of `cams`."""
    import torch
    from volsurfs_amd.camera import Camera
    out = []
    for c in cams:
        d = Camera(c.intrinsics, torch.cat([c.c2w.cpu(), torch.tensor([[0.0, 0.0, 0.0, 1.0]])]), 2 * c.height, 2 * c.width)
        d.c2w = c.c2w
        d.intrinsics_inv = (c.intrinsics_inv * torch.tensor([0.5, 0.5, 1.0], device=c.intrinsics_inv.device)).contiguous()
        out.append(d)
    return out


def _timed(fn, reps):
    import torch
    fn()                                                    # warm-up: code objects, allocator, feedback buffers
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility.json"))
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("visibility_bench needs a GPU")
    from tools.simplify_bench import _fields
    from volsurfs_amd import _lib, isosurface as iso, visibility as vis
    from volsurfs_amd.camera import get_camera_rays
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.simplify import simplify_mesh

    meshes, _ = iso.extract_level_sets(_fields()["lobed_noisy"], a.n, K, delta_surfs=DELTA)
    meshes = [simplify_mesh(m, RATIO) for m in meshes]
    nr_faces = [int(m.faces.shape[0]) for m in meshes]
    base = [sum(nr_faces[:k]) for k in range(K)]
    total = sum(nr_faces)
    tracer = RayTracer(meshes, builder="device")
    cams = _orbit(a.views, a.size, float(a.size))
    result = {"device": torch.cuda.get_device_name(0), "grid": a.n, "shells": K, "faces": nr_faces,
              "tree_depth": tracer.max_depth, "views": a.views, "height": a.size, "width": a.size, "reps": a.reps,
              "supersample": {}}

    face_base = (ctypes.c_longlong * K)(*base)
    counts = torch.zeros(total, dtype=torch.int32, device="cuda")
    slot_face = tracer.slot_face_id.long()
    shell_base = torch.tensor(base, dtype=torch.int64, device="cuda")[:, None]

    for s in (1, 2):
        c2w, kinv, H, W = vis._stack_cameras(cams, "cuda")

        def fused(views=slice(None), nr=a.views):
            _lib.call("vsa_face_view_counts", tracer.qnodes, tracer.tris, tracer._roots, tracer._frames, K,
                      tracer.max_depth, c2w[views], kinv[views], nr, H, W, s, 0.0, face_base, counts, _lib.stream_ptr())

        def fused_all():
            counts.zero_()
            fused()

        def fused_per_view():
            counts.zero_()
            for v in range(a.views):
                fused(slice(v, v + 1), 1)

        comp_cams = cams if s == 1 else _doubled(cams)
        comp = torch.zeros(total + 1, dtype=torch.int64, device="cuda")

        def composition():
            comp.zero_()
            for cam in comp_cams:
                o, d, _ = get_camera_rays(cam)
                _, slot, _ = tracer.trace_all(o, d)
                hit = slot >= 0
                ids = (slot_face[slot.clamp(min=0).long()] + shell_base)[hit]
                comp[:total].add_(torch.bincount(ids, minlength=total))
                comp[total] += hit.numel() - ids.numel()

        row = {"samples": a.views * H * W * s * s, "walks": a.views * H * W * s * s * K}
        for tile in vis.TILES:
            vis.set_tile(tile)
            row[f"fused_{tile}_ms"] = _timed(fused_all, a.reps)
            row[f"counts_{tile}"] = counts.clone()
        vis.set_tile("8x8")
        row["fused_per_view_ms"] = _timed(fused_per_view, a.reps)
        per_view_counts = counts.clone()
        row["composition_ms"] = _timed(composition, a.reps)
        got = {t: row.pop(f"counts_{t}").to(torch.int64) & 0xFFFFFFFF for t in vis.TILES}
        row["counts_equal"] = bool(all(torch.equal(g, comp[:total]) for g in got.values())
                                   and torch.equal(per_view_counts.to(torch.int64) & 0xFFFFFFFF, comp[:total]))
        row["hits"] = int(comp[:total].sum())
        row["misses"] = int(comp[total])
        best = min(vis.TILES, key=lambda t: row[f"fused_{t}_ms"]["median"])
        row["best_tile"] = best
        row["composition_over_fused"] = round(row["composition_ms"]["median"] / row[f"fused_{best}_ms"]["median"], 2)
        # bytes the composition moves through memory and the fused pass does not: 24 B of ray per sample, 16 B of hit
        # record and 8 B of gathered id per (sample, shell)
        row["composition_ray_and_hit_GB"] = round((24 * row["samples"] + 24 * row["walks"]) / 1e9, 2)
        per_shell = [got["8x8"][b:b + n] for b, n in zip(base, nr_faces)]
        for rings in (0, 1):
            keep = [vis.visible_face_mask(m, c, 1, rings) for m, c in zip(meshes, per_shell)]
            row[f"culled_fraction_rings{rings}"] = round(1.0 - sum(int(k.sum()) for k in keep) / total, 4)
        result["supersample"][str(s)] = row
        print(json.dumps({str(s): row}), flush=True)
        if not row["counts_equal"]:
            sys.exit("the fused counts differ from the composition's")

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
