"""Winding numbers of a mesh (volsurfs_amd.mesh_winding, csrc/mesh_winding.hip): the moments build, the point
query at three values of beta, the lattice field with the winding sign against its composition and against the
pseudonormal field of tools/mesh_sdf_bench.py, and `offset_shells` from an open mesh, in one process on one GPU.

Meshes (marching-cubes shells of tools/simplify_bench.py's fields at n = 512, simplified to 0.025, device-built trees):
  sphere, lobed                  tools/mesh_sdf_bench.py's two inputs (closed);
  sphere_culled, lobed_culled    the same without the faces no camera of tools/visibility_bench.py's orbit sees
                                 (`remove_invisible_faces`: 100 views, 800 x 800): open, with their edge census.
Timed, each --reps times after a warm-up, device time from events around the whole call (tracers and moments built
outside the window, except in `moments` and `offset_shells`), min / median / max in ms:
  moments         vsa_mesh_winding_moments for the tracer's tree;
  query           `winding_number` of --samples points (uniform in [-1, 1]^3) at beta = 2, 3 and inf, with the entries
                  judged and the exact triangle terms per query from the counting build of the walk, and the largest
                  difference from beta = inf;
  banded / full   `mesh_to_sdf_grid(sign="winding")` at the baker's K = 5 band and without one, with the brick counts;
  pseudonormal    the same two grids with the default sign: what the robust sign costs;
  composition     `sample_grid` of `signed_distance(sign="winding")`, chunk 128^3, and whether the full grid equals it
                  and the banded one its clamp;
  offset_shells   K = 5 shells with sign="winding", with the shells' edge census (culled inputs only).
Needs a GPU; writes one JSON file.

    python tools/mesh_winding_bench.py [--out profiles/mesh_winding.json] [--grid 512] [--samples 1000000] [--reps 10]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, DELTA, RATIO = 5, 0.0025, 0.025


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_winding.json"))
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("mesh_winding_bench needs a GPU")
    from tools.mesh_distance_bench import _shells, _timed
    from tools.simplify_bench import _fields
    from tools.visibility_bench import _orbit
    from volsurfs_amd import isosurface as iso, mesh_sdf as ms, mesh_winding as mw
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.simplify import simplify_mesh
    from volsurfs_amd.visibility import remove_invisible_faces

    n, N = a.grid, a.samples
    h = 2.0 / (n - 1)
    band = 2 * DELTA + 2.0 * math.sqrt(3.0) * h
    fields = _fields()
    cams = _orbit(100, 800, 800.0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    pts = (torch.rand(N, 3, device="cuda", generator=gen) * 2.0 - 1.0).contiguous()
    result = {"device": torch.cuda.get_device_name(0), "grid": n, "h": h, "band": band, "samples": N, "reps": a.reps}
    for name, field in (("sphere", "sphere"), ("lobed", "lobed_noisy")):
        (full,), _ = _shells(fields[field], n, [0.0])
        closed = simplify_mesh(full, RATIO)
        del full
        for variant, mesh in ((name, closed), (name + "_culled", remove_invisible_faces([closed], cams)[0])):
            tracer = RayTracer([mesh], builder="device")
            handle = (tracer, 0)
            row = {"faces": int(mesh.faces.shape[0]), "tree_depth": tracer.max_depth,
                   "nodes": int(tracer.qnodes.shape[0]), "census": mw.edge_census(mesh)}

            def moments():
                tracer._wm = None
                tracer.winding_moments()

            row["moments_ms"] = _timed(moments, a.reps)
            exact = tracer.winding_number(pts, beta=math.inf)
            row["query"] = {}
            for beta in (2.0, 3.0, math.inf):
                st = tracer.winding_stats(pts, beta)
                w = tracer.winding_number(pts, beta=beta)
                row["query"][str(beta)] = {
                    "ms": _timed(lambda: tracer.winding_number(pts, beta=beta), a.reps),
                    "entries_per_query": round(st["node_visits"] / st["queries"], 2),
                    "tri_terms_per_query": round(st["tri_terms"] / st["queries"], 2),
                    "max_abs_diff_from_exact": float((w - exact).abs().max())}
            del exact, w

            row["banded_ms"] = _timed(lambda: ms.mesh_to_sdf_grid(handle, n, 1.0, band, sign="winding"), a.reps)
            banded, counts = ms.mesh_to_sdf_grid(handle, n, 1.0, band, sign="winding")
            row.update(counts)
            row["full_ms"] = _timed(lambda: ms.mesh_to_sdf_grid(handle, n, 1.0, sign="winding"), a.reps)
            whole, _ = ms.mesh_to_sdf_grid(handle, n, 1.0, sign="winding")
            row["banded_equals_clamped_full"] = bool(torch.equal(banded, whole.clamp(-band, band)))
            del banded

            def composition():
                return iso.sample_grid(lambda p: tracer.signed_distance(p, sign="winding")["dist"], n, chunk=128)

            row["composition_ms"] = _timed(composition, a.reps)
            row["full_equals_composition"] = bool(torch.equal(whole, composition()))
            del whole
            torch.cuda.empty_cache()
            tracer.pseudonormal_tables()
            row["pseudonormal_banded_ms"] = _timed(lambda: ms.mesh_to_sdf_grid(handle, n, 1.0, band), a.reps)
            row["pseudonormal_full_ms"] = _timed(lambda: ms.mesh_to_sdf_grid(handle, n, 1.0), a.reps)
            row["banded_over_pseudonormal"] = round(row["banded_ms"]["median"] / row["pseudonormal_banded_ms"]["median"], 2)
            row["full_over_pseudonormal"] = round(row["full_ms"]["median"] / row["pseudonormal_full_ms"]["median"], 2)
            row["composition_over_full"] = round(row["composition_ms"]["median"] / row["full_ms"]["median"], 2)

            if variant.endswith("_culled"):
                def shells():
                    return ms.offset_shells(mesh, K, DELTA, nr_points_per_dim=n, sign="winding")

                row["offset_shells_ms"] = _timed(shells, a.reps)
                out, levels = shells()
                row["offset_shells"] = {"levels": levels, "faces": [int(m.faces.shape[0]) for m in out],
                                        "census": [mw.edge_census(m) for m in out]}
                del out
            result[variant] = row
            print(json.dumps({variant: row}), flush=True)
            del tracer
            torch.cuda.empty_cache()
        del closed

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
