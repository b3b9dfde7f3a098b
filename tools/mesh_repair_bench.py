"""Mesh repair (volsurfs_amd/mesh_repair.py, csrc/mesh_repair.hip) on scrambled soups at about 10^5 and 10^6
faces: a lobed sphere shell (`stress_shells(K=1, subdiv)`, one closed component) and the ball-and-blobs level set of
tests/mesh_clean_restated.py (`blob_field`, many components), each un-welded to 3 F vertices, its vertices shuffled and
40 % of its faces flipped.  Per mesh, in one process:
  * `stage_ms`      device ms per stage from the library's `stage_ms` (events, one synchronisation per stage), the medians
                    of --reps runs after a warm-up: `weld` (tol = 0), `weld_tol` (tol = --tol) and `orient` (of the welded
                    mesh);
  * `weld_ms`, `weld_tol_ms`, `orient_ms`, `repair_ms`   the whole `weld_vertices`, `orient_faces` and `repair_mesh`
                    (the two edge censuses included) from events: median, min and max of --reps runs after a warm-up;
  * `host_ms`       the restatement (tests/mesh_repair_restated.py: numpy + scipy) of weld (tol = 0) and orient on the
                    same soup on the host, timed once, the transfer of the mesh not included; `ratio` = host / device.
                    The outputs are compared (`equal_to_host`).  The host's tol > 0 rule is a brute force over all
                    pairs and is not timed;
  * `census_after`  of the repaired mesh.
For the first shell, `sdf_grid_auto_ms`: `mesh_to_sdf_grid(handle, --grid, band = 3 cell diagonals, sign="auto")` on a
tracer built beforehand, of the soup (auto takes the winding number) and of the repaired mesh (auto takes the
pseudonormal): median, min and max of --reps runs.

    python tools/mesh_repair_bench.py [--reps 5] [--subdiv 6 8] [--blobs-res 256] [--out profiles/mesh_repair.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scramble(v, f, seed=11):
    """The soup of tests/mesh_repair_restated.py::soup for any mesh."""
    import numpy as np
    nf = f.shape[0]
    rng = np.random.default_rng(seed)
    order = rng.permutation(3 * nf)
    flip = rng.random(nf) < 0.4
    corners = v[f.reshape(-1).astype(np.int64)]
    inv = np.empty(3 * nf, np.int64)
    inv[order] = np.arange(3 * nf)
    faces = inv.reshape(nf, 3).astype(np.int32)
    faces[flip] = faces[flip][:, [0, 2, 1]]
    return np.ascontiguousarray(corners[order], np.float32), np.ascontiguousarray(faces)


def timed(fn, reps):
    import torch
    fn()                                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
        del out
    return [round(f(ms), 3) for f in (statistics.median, min, max)]


def stage_medians(fn, reps):
    """Medians per stage of `reps` runs of fn(stage_ms_dict) after a warm-up."""
    fn({})
    runs = []
    for _ in range(reps):
        d = {}
        fn(d)
        runs.append(d)
    return {k: round(statistics.median(r[k] for r in runs), 4) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--subdiv", type=int, nargs="*", default=[6, 8])
    ap.add_argument("--blobs-res", type=int, nargs="*", default=[256])
    ap.add_argument("--tol", type=float, default=2e-6)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import mesh_clean_restated as C
    import mesh_repair_restated as R
    from volsurfs_amd import mesh_repair as MR
    from volsurfs_amd import mesh_sdf as MS
    from volsurfs_amd.isosurface import marching_cubes
    from volsurfs_amd.mesh import TensorMesh, stress_shells
    from volsurfs_amd.raytrace import RayTracer
    assert torch.cuda.is_available(), "mesh_repair_bench needs a GPU"

    def sources():
        for s in a.subdiv:
            m = stress_shells(K=1, subdiv=s, device="cpu")[0]
            yield f"shell subdiv {s}", m.vertices.numpy().astype(np.float32), m.faces.numpy().astype(np.int32)
        for n in a.blobs_res:
            grid, origin, spacing = C.blob_field(n)[:3]
            m = marching_cubes(torch.from_numpy(grid).cuda(), 0.0, list(origin), list(spacing))[0]
            yield f"blob_field {n}", m.vertices.cpu().numpy(), m.faces.cpu().numpy()

    rows, grid_row = [], None
    for what, v, f in sources():
        sv, sf = scramble(v, f)
        soup = TensorMesh(sv, sf, None, device="cuda")
        welded, _, _, wrep = MR.weld_vertices(soup)
        fixed, flipped, component, orep = MR.orient_faces(welded)
        repaired, report = MR.repair_mesh(soup)
        row = {"mesh": what, "faces": int(sf.shape[0]), "soup_vertices": int(sv.shape[0]), "reps": a.reps,
               "tol": a.tol, "vertices_out": wrep["vertices_out"], "components": orep["components"],
               "flipped": orep["flipped"], "undecided_components": orep["undecided_components"],
               "census_after": report["census_after"]}
        row["stage_ms"] = {
            "weld": stage_medians(lambda d: MR.weld_vertices(soup, stage_ms=d), a.reps),
            "weld_tol": stage_medians(lambda d: MR.weld_vertices(soup, a.tol, stage_ms=d), a.reps),
            "orient": stage_medians(lambda d: MR.orient_faces(welded, stage_ms=d), a.reps)}
        row["weld_ms"] = timed(lambda: MR.weld_vertices(soup), a.reps)
        row["weld_tol_ms"] = timed(lambda: MR.weld_vertices(soup, a.tol), a.reps)
        row["orient_ms"] = timed(lambda: MR.orient_faces(welded), a.reps)
        row["repair_ms"] = timed(lambda: MR.repair_mesh(soup), a.reps)
        by_tol = MR.weld_vertices(soup, a.tol)
        row["weld_tol_equals_exact"] = bool(torch.equal(by_tol[1], MR.weld_vertices(soup)[1]))
        if not a.skip_host:
            t0 = time.perf_counter()
            hw = R.weld(sv, sf)
            t1 = time.perf_counter()
            ho = R.orient(hw["vertices"], hw["faces"])
            t2 = time.perf_counter()
            row["host_ms"] = {"weld": round((t1 - t0) * 1e3, 1), "orient": round((t2 - t1) * 1e3, 1)}
            row["host_threads"] = torch.get_num_threads()
            row["ratio"] = {"weld": round(row["host_ms"]["weld"] / row["weld_ms"][0], 1),
                            "orient": round(row["host_ms"]["orient"] / row["orient_ms"][0], 1)}
            row["equal_to_host"] = bool(
                np.array_equal(welded.faces.cpu().numpy(), hw["faces"]) and
                welded.vertices.cpu().numpy().tobytes() == hw["vertices"].tobytes() and
                np.array_equal(fixed.faces.cpu().numpy(), ho["faces"]) and
                np.array_equal(component.cpu().numpy(), ho["component"]) and orep == ho["report"])
            del hw, ho
        if grid_row is None and what.startswith("shell"):
            diag = math.sqrt(3.0) * 2.0 / (a.grid - 1)
            before = (RayTracer([soup], builder="device"), 0)
            after = (RayTracer([repaired], builder="device"), 0)
            grid_row = {"mesh": what, "grid": a.grid, "band": 3 * diag,
                        "rule": {"soup": before[0].sign_rule("auto"), "repaired": after[0].sign_rule("auto")}}
            grid_row["soup"] = timed(lambda: MS.mesh_to_sdf_grid(before, a.grid, 1.0, 3 * diag, sign="auto"), a.reps)
            grid_row["repaired"] = timed(lambda: MS.mesh_to_sdf_grid(after, a.grid, 1.0, 3 * diag, sign="auto"), a.reps)
            original = (RayTracer([TensorMesh(v, f, None, device="cuda")], builder="device"), 0)
            ga, _ = MS.mesh_to_sdf_grid(after, a.grid, 1.0, 3 * diag, sign="auto")
            go, _ = MS.mesh_to_sdf_grid(original, a.grid, 1.0, 3 * diag)
            grid_row["repaired_equals_original_grid"] = bool(torch.equal(ga, go))
            del before, after, original, ga, go
        rows.append(row)
        print(json.dumps(row), flush=True)
        del soup, welded, fixed, repaired
    if grid_row:
        print(json.dumps(grid_row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows, "sdf_grid_auto_ms": grid_row}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
