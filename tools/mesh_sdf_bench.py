"""Signed distance to a mesh (volsurfs_amd.mesh_sdf, csrc/mesh_sdf.hip): the pseudonormal tables, the field
on the n = 512 lattice of radius 1 with and without a band, and `offset_shells` end to end, against the composition the
library offered before (chunked `RayTracer.closest` over all n^3 lattice points: unsigned, so a lower bound on a
composed signed field), in one process on one GPU.

Meshes (marching-cubes shells of tools/simplify_bench.py's fields at n = 512, simplified to 0.025, device-built trees):
  sphere    the sphere shell;
  lobed     the zero level of the lobed, noisy field.
Timed, each --reps times after a warm-up, device time from events around the whole call (tracers built outside the
window; tables built before it, except in `tables` and `offset_shells`), min / median / max in ms:
  tables          `pseudonormals`;
  banded          `mesh_to_sdf_grid` at the baker's K = 5 band (2 delta_surfs + 2 cell diagonals), with the near / far
                  brick counts, and node visits / triangle tests per query of the walked lattice points (those inside
                  the band, a million of them at the most) from the counting build of the walk;
  centres         the signed point query at every brick centre: what the classification pass asks, timed apart (the
                  queries deep inside a shell are DESIGN §27's hard case), with its counts per query;
  full            `mesh_to_sdf_grid` without a band;
  composition     `sample_grid` of `RayTracer.closest`'s distance, chunk 128^3;
  offset_shells   K = 5 shells from the mesh: tracer, tables, banded grid, one marching-cubes call;
  sign            `signed_distance` against `closest` on --samples surface samples moved by up to a cell along x.
Needs a GPU; writes one JSON file.

    python tools/mesh_sdf_bench.py [--out profiles/mesh_sdf.json] [--grid 512] [--samples 1000000] [--reps 10]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, DELTA, RATIO = 5, 0.0025, 0.025


def _per_query(st):
    return {"node_visits": round(st["node_visits"] / st["queries"], 2),
            "tri_tests": round(st["tri_tests"] / st["queries"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sdf.json"))
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("mesh_sdf_bench needs a GPU")
    from tools.mesh_distance_bench import _shells, _timed
    from tools.simplify_bench import _fields
    from volsurfs_amd import isosurface as iso, mesh_distance as md, mesh_sdf as ms
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.simplify import simplify_mesh

    n, N = a.grid, a.samples
    h = 2.0 / (n - 1)
    band = 2 * DELTA + 2.0 * math.sqrt(3.0) * h
    fields = _fields()
    result = {"device": torch.cuda.get_device_name(0), "grid": n, "h": h, "band": band, "samples": N, "reps": a.reps}
    for name, field in (("sphere", "sphere"), ("lobed", "lobed_noisy")):
        (full,), _ = _shells(fields[field], n, [0.0])
        mesh = simplify_mesh(full, RATIO)
        del full
        tracer = RayTracer([mesh], builder="device")
        handle = (tracer, 0)
        row = {"faces": int(mesh.faces.shape[0]), "tree_depth": tracer.max_depth}
        row["tables_ms"] = _timed(lambda: ms.pseudonormals(mesh), a.reps)
        tracer.pseudonormal_tables()

        row["banded_ms"] = _timed(lambda: ms.mesh_to_sdf_grid(handle, n, 1.0, band), a.reps)
        banded, counts = ms.mesh_to_sdf_grid(handle, n, 1.0, band)
        row.update(counts)
        axis = torch.linspace(-1.0, 1.0, n, dtype=torch.float32).cuda()
        inside = (banded.abs() < band).nonzero()
        row["points_inside_band"] = int(inside.shape[0])
        inside = inside[:: max(1, inside.shape[0] // 1_000_000)]
        row["banded_walk_per_query"] = _per_query(tracer.closest_stats(axis[inside].contiguous()))
        del inside

        first = torch.arange(0, n, 4, device="cuda")
        last = (first + 3).clamp_max(n - 1)
        c = 0.5 * (axis[first] + axis[last])
        centres = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3).contiguous()
        row["bricks"] = int(centres.shape[0])
        row["centres_ms"] = _timed(lambda: tracer.signed_distance(centres), a.reps)
        row["centres_per_query"] = _per_query(tracer.closest_stats(centres))
        row["centres_share_of_banded"] = round(row["centres_ms"]["median"] / row["banded_ms"]["median"], 3)
        del centres

        row["full_ms"] = _timed(lambda: ms.mesh_to_sdf_grid(handle, n, 1.0), a.reps)
        whole, _ = ms.mesh_to_sdf_grid(handle, n, 1.0)
        row["banded_equals_clamped_full"] = bool(torch.equal(banded, whole.clamp(-band, band)))
        del banded

        def composition():
            return iso.sample_grid(lambda p: tracer.closest(p)["dist"], n, chunk=128)

        row["composition_ms"] = _timed(composition, a.reps)
        row["full_abs_equals_composition"] = bool(torch.equal(whole.abs(), composition()))
        del whole
        torch.cuda.empty_cache()
        row["composition_over_banded"] = round(row["composition_ms"]["median"] / row["banded_ms"]["median"], 2)
        row["composition_over_full"] = round(row["composition_ms"]["median"] / row["full_ms"]["median"], 2)
        row["full_over_banded"] = round(row["full_ms"]["median"] / row["banded_ms"]["median"], 2)

        row["offset_shells_ms"] = _timed(lambda: ms.offset_shells(mesh, K, DELTA, nr_points_per_dim=n), a.reps)
        shells, levels = ms.offset_shells(mesh, K, DELTA, nr_points_per_dim=n)
        row["offset_shells"] = {"levels": levels, "faces": [int(m.faces.shape[0]) for m in shells]}
        nesting = ms.shell_nesting(shells, N)
        row["nesting"] = [{"pair": list(c["pair"]), "outside": c["outside"],
                           "clearance_over_delta": round(c["clearance"] / DELTA, 4)} for c in nesting]
        del shells

        pts, _, _ = md.sample_surface(handle, N)
        gen = torch.Generator(device="cuda").manual_seed(0)
        pts[:, 0] += (torch.rand(N, device="cuda", generator=gen) * 2.0 - 1.0) * h
        row["closest_ms"] = _timed(lambda: tracer.closest(pts), a.reps)
        row["signed_ms"] = _timed(lambda: tracer.signed_distance(pts), a.reps)
        row["sign_ns_per_query"] = round(1e6 * (row["signed_ms"]["median"] - row["closest_ms"]["median"]) / N, 3)
        result[name] = row
        print(json.dumps({name: row}), flush=True)
        del tracer, mesh, pts
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
