"""Mesh-to-mesh distance (volsurfs_amd.mesh_distance, csrc/mesh_distance.hip): the closest-point walk and
the fused sample + walk + reduce launch against the composition of the unfused calls and against the torch
formulation people use without it, in one process on one GPU.

Workloads (marching-cubes shells of tools/simplify_bench.py's fields, device-built trees):
  sphere    one n = 512 sphere shell and its 0.025 simplification in one tracer: `closest_all` for 10^6 random queries
            of [-0.5, 0.5]^3 (x 2 shells), `surface_distance` with 10^6 samples in both directions.
  lobed     the K = 5 lobed shells at delta_surfs = 0.0025 of an n^3 grid, n in {256, 512}: `simplification_error` of
            every shell against its 0.025 simplification (the numbers of DESIGN §15, in grid spacings h), and
            `shell_clearance` of the five simplified shells (n = 512: timed).
  cdist     at 10^5 x 10^5: a chunked torch.cdist point-to-point Chamfer of the two sampled clouds of the sphere pair
            against `mesh_distance` with 10^5 samples.
Timed, each --reps times after a warm-up, device time from events around the whole call (tracers built outside the
window; the area prefix and the one blocking read inside), min / median / max in ms:
  fused     `surface_distance` / `shell_clearance`;
  unfused   `surface_distance_unfused`: sample_surface -> closest -> torch reductions, on the same GPU;
  both forms of the walk's stack (`set_walk_bounds("always")` / `("never")`), with node visits and triangle tests per query from the counting
  build of the walk.
The fused and unfused statistics are compared (min, max equal).  Needs a GPU; writes one JSON file.

    python tools/mesh_distance_bench.py [--out profiles/mesh_distance.json] [--samples 1000000] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, DELTA, RATIO = 5, 0.0025, 0.025


def _timed(fn, reps):
    import torch
    fn()                                                    # warm-up: code objects, allocator
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


def _st(s):
    return {"n": s.n, "min": s.min, "mean": s.mean, "rms": s.rms, "max": s.max}


def _shells(field, n, levels):
    from volsurfs_amd import isosurface as iso
    h = 2.0 / (n - 1)
    grid = iso.sample_grid(field, n, chunk=128)
    return iso.marching_cubes(grid, levels, [-1.0] * 3, [h] * 3), h


def _cdist_chamfer(a, b, chunk=8192):
    """Point-to-point Chamfer of two clouds by chunked torch.cdist: mean nearest distance both ways."""
    import torch

    def one_way(x, y):
        best = []
        for s in range(0, x.shape[0], chunk):
            best.append(torch.cdist(x[s:s + chunk], y).min(dim=1).values)
        return torch.cat(best).double().mean()

    return float(one_way(a, b) + one_way(b, a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_distance.json"))
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("mesh_distance_bench needs a GPU")
    from tools.simplify_bench import _fields
    from volsurfs_amd import isosurface as iso, mesh_distance as md
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.simplify import simplify_mesh

    N = a.samples
    fields = _fields()
    result = {"device": torch.cuda.get_device_name(0), "samples": N, "reps": a.reps}

    # ---- sphere: a shell and its simplification
    (full,), h = _shells(fields["sphere"], 512, [0.0])
    simple = simplify_mesh(full, RATIO)
    tracer = RayTracer([full, simple], builder="device")
    gen = torch.Generator(device="cuda").manual_seed(0)
    queries = torch.rand(N, 3, device="cuda", generator=gen) - 0.5
    row = {"grid": 512, "h": h, "faces": [int(full.faces.shape[0]), int(simple.faces.shape[0])],
           "tree_depth": tracer.max_depth}
    answers = {}
    for mode, tag in (("always", "bounds"), ("never", "nodes_only")):
        md.set_walk_bounds(mode)
        row[f"closest_all_{tag}_ms"] = _timed(lambda: tracer.closest_all(queries), a.reps)
        answers[tag] = tracer.closest_all(queries)
        st = tracer.closest_stats(queries)
        row[f"closest_all_{tag}_per_query"] = {"node_visits": round(st["node_visits"] / st["queries"], 2),
                                               "tri_tests": round(st["tri_tests"] / st["queries"], 2)}
        for s, d, name in ((0, 1, "full_to_simple"), (1, 0, "simple_to_full")):
            row[f"fused_{name}_{tag}_ms"] = _timed(lambda: md.surface_distance((tracer, s), (tracer, d), N), a.reps)
            pts, _, _ = md.sample_surface((tracer, s), N)
            one = RayTracer([(full, simple)[d]], builder="device")
            st = one.closest_stats(pts)
            row[f"walk_{name}_{tag}_per_query"] = {"node_visits": round(st["node_visits"] / st["queries"], 2),
                                                   "tri_tests": round(st["tri_tests"] / st["queries"], 2)}
            del one, pts
    md.set_walk_bounds("shallow")
    row["walk_forms_equal"] = all(torch.equal(answers["bounds"][k], answers["nodes_only"][k]) for k in answers["bounds"])
    del answers
    for s, d, name in ((0, 1, "full_to_simple"), (1, 0, "simple_to_full")):
        row[f"unfused_{name}_ms"] = _timed(lambda: md.surface_distance_unfused((tracer, s), (tracer, d), N), a.reps)
        fused, unfused = md.surface_distance((tracer, s), (tracer, d), N), md.surface_distance_unfused((tracer, s), (tracer, d), N)
        row[name] = _st(fused)
        row[f"{name}_equal"] = (fused.min, fused.max) == (unfused.min, unfused.max)
        row[f"fused_{name}_ms"] = _timed(lambda: md.surface_distance((tracer, s), (tracer, d), N), a.reps)
        row[f"unfused_over_fused_{name}"] = round(row[f"unfused_{name}_ms"]["median"] /
                                                  row[f"fused_{name}_ms"]["median"], 2)
    result["sphere"] = row
    print(json.dumps({"sphere": row}), flush=True)

    # ---- cdist: what people use without this, where brute force fits
    n_small = 100_000
    pa, _, _ = md.sample_surface((tracer, 0), n_small)
    pb, _, _ = md.sample_surface((tracer, 1), n_small)
    row = {"points": n_small}
    row["cdist_ms"] = _timed(lambda: _cdist_chamfer(pa, pb), max(a.reps // 3, 3))
    row["cdist_chamfer"] = _cdist_chamfer(pa, pb)
    row["mesh_distance_ms"] = _timed(lambda: md.mesh_distance((tracer, 0), (tracer, 1), n_small), a.reps)
    row["mesh_distance_chamfer"] = md.mesh_distance((tracer, 0), (tracer, 1), n_small)["chamfer"]
    row["cdist_over_mesh_distance"] = round(row["cdist_ms"]["median"] / row["mesh_distance_ms"]["median"], 1)
    result["cdist"] = row
    print(json.dumps({"cdist": row}), flush=True)
    del tracer, full, simple, queries, pa, pb
    torch.cuda.empty_cache()

    # ---- lobed shells: the simplifier's error and the clearance of consecutive simplified shells
    result["lobed"] = {}
    for n in (256, 512):
        shells, h = _shells(fields["lobed_noisy"], n, iso.level_set_values(K, DELTA))
        simplified = [simplify_mesh(m, RATIO) for m in shells]
        errors = [md.simplification_error(m, s, N) for m, s in zip(shells, simplified)]
        row = {"h": h, "faces_in": [int(m.faces.shape[0]) for m in shells],
               "faces_out": [int(m.faces.shape[0]) for m in simplified],
               "error_h": {"mean": round(max(max(e["ab"].mean, e["ba"].mean) for e in errors) / h, 4),
                           "rms": round(max(max(e["ab"].rms, e["ba"].rms) for e in errors) / h, 4),
                           "hausdorff": round(max(e["hausdorff"] for e in errors) / h, 4)},
               "hausdorff_rel_diagonal": max(e["hausdorff_rel"] for e in errors)}
        tracer = RayTracer(simplified, builder="device")
        clearance = md.shell_clearance(tracer, N)
        row["clearance"] = [{"pair": list(c["pair"]), "out": _st(c["out"]), "in": _st(c["in"])} for c in clearance]
        row["clearance_min_over_delta"] = round(min(min(c["out"].min, c["in"].min) for c in clearance) / DELTA, 4)
        row["clearance_mean_over_delta"] = round(sum(c["out"].mean + c["in"].mean for c in clearance) / (2 * (K - 1)) / DELTA, 4)
        if n == 512:
            row["tree_depth"] = tracer.max_depth
            row["shell_clearance_fused_ms"] = _timed(lambda: md.shell_clearance(tracer, N), a.reps)
            md.set_walk_bounds("never")
            row["shell_clearance_fused_nodes_only_ms"] = _timed(lambda: md.shell_clearance(tracer, N), a.reps)
            md.set_walk_bounds("shallow")

            def composition():
                for k in range(K - 1):
                    md.surface_distance_unfused((tracer, k), (tracer, k + 1), N)
                    md.surface_distance_unfused((tracer, k + 1), (tracer, k), N)

            row["shell_clearance_unfused_ms"] = _timed(composition, a.reps)
            row["unfused_over_fused"] = round(row["shell_clearance_unfused_ms"]["median"] /
                                              row["shell_clearance_fused_ms"]["median"], 2)
        result["lobed"][str(n)] = row
        print(json.dumps({f"lobed_{n}": row}), flush=True)
        del shells, simplified, tracer
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
