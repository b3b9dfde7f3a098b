"""Floater removal (volsurfs_amd/mesh_clean.py, csrc/mesh_clean.hip) at the sizes the baker meets: marching
cubes of a ball-and-blobs field at about 10^6 faces and at the scale the TSDF extraction produces (n = 512, at least
4 x 10^6 faces).

The field is built on the device.  A plain ball inside [-1, 1]^3 has too little area for these face counts (2 x 10^5 at
n = 256), so the large component is a ball of radius 0.6 cut out of a thickened gyroid sheet of wave number --freq (one
connected surface whose area grows with the wave number; its cut through the ball's boundary leaves small fragments of
its own), with --blobs small balls of radii 0.3 .. 20 voxels outside it.  Per resolution, in one process:
  * `stage_ms`         device ms per stage from the library's `stage_ms` (events, one synchronisation per stage), the
                       medians of --reps runs after a warm-up: `clusters` from vsa_mesh_clusters (areas included),
                       `filter` from vsa_mesh_filter in cluster mode;
  * `clusters_ms`, `post_process_ms`   the whole cluster_connected_triangles / post_process_mesh from events, median
                       (min - max) of --reps runs after a warm-up, with the library's own synchronisations but without
                       the per-stage ones;
  * `stage_bytes`      the bytes each stage must move (reads + writes of its arrays, computed from V, F, C and the
                       radix passes of 8 bits; a lower bound: rocPRIM's histograms and the gathers' sector overfetch
                       are not counted), and `GB_per_s` = bytes / stage time;
  * `host_ms`          the restatement (tests/mesh_clean_restated.py: numpy + scipy) on the same mesh on the host, timed
                       once after a warm-up on a small mesh, the transfer of the mesh not included; `ratio` =
                       host_ms / post_process_ms.  The outputs are compared.

    python tools/mesh_clean_bench.py [--reps 5] [--res 256 512] [--freq 34] [--out profiles/mesh_clean.json]
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

BALL_R = 0.6


def field(n, freq, nr_blobs, seed=0, device="cuda"):
    """[n, n, n] f32 on the device: max(|gyroid(freq x)| - 0.35, |x| - 0.6) and the blobs, level 0, inside below."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    ax = torch.linspace(-1.0, 1.0, n, dtype=torch.float32, device=device)
    grid = torch.empty(n, n, n, device=device)
    voxel = 2.0 / (n - 1)
    blobs = []
    radii = np.exp(rng.uniform(math.log(0.3 * voxel), math.log(20 * voxel), nr_blobs))
    for r in radii:
        for _ in range(1000):
            c = rng.uniform(-0.97 + r, 0.97 - r, 3)
            if np.linalg.norm(c) - r > BALL_R + 4 * voxel and \
                    all(np.linalg.norm(c - c2) > r + r2 + 4 * voxel for c2, r2 in blobs):
                blobs.append((c, r))
                break
    step = max(1, (1 << 24) // (n * n))
    for i0 in range(0, n, step):
        X, Y, Z = torch.meshgrid(ax[i0:i0 + step], ax, ax, indexing="ij")
        g = torch.sin(freq * X) * torch.cos(freq * Y) + torch.sin(freq * Y) * torch.cos(freq * Z) + \
            torch.sin(freq * Z) * torch.cos(freq * X)
        # (the gyroid's gradient is about freq: dividing by it makes the slab's values distance-like)
        f = torch.maximum((g.abs() - 0.35) / freq, torch.sqrt(X * X + Y * Y + Z * Z) - BALL_R)
        for c, r in blobs:
            f = torch.minimum(f, torch.sqrt((X - float(c[0])) ** 2 + (Y - float(c[1])) ** 2 + (Z - float(c[2])) ** 2)
                              - float(r))
        grid[i0:i0 + step] = f
    return grid, len(blobs)


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


def stage_bytes(V, F, C, V_out, F_out):
    """Bytes each stage must read + write.  A radix sort of N keys of `kb` bytes with values of `vb` bytes and `bits`
    key bits makes ceil(bits / 8) passes, each reading and writing N (kb + vb)."""
    s = max(1, (V - 1).bit_length())
    passes = lambda bits: -(-bits // 8)
    cb = max(1, (C - 1).bit_length())
    return {
        "edges": 12 * F + 3 * F * (8 + 4),
        "sort": passes(2 * s) * 2 * 3 * F * (8 + 4),
        "hook": 3 * F * (8 + 4) + 4 * F + 2 * 4 * F,                  # sorted keys and slots, iota, one parent read + CAS
        "roots": 2 * 4 * F + 2 * 4 * F,                               # at least the parent and the root's entry; 2 writes
        "number": 2 * 2 * 4 * F + 4 * 4 * F + 4 * F,                  # the scan, rank / root / flags / cluster, counts zeroed
        "areas": 4 * F + 2 * 4 * F + passes(cb) * 2 * F * 8 + 4 * F + 8 * F + 12 * F + 36 * F + 8 * C,
        "threshold": 2 * 2 * 4 * C,
        "mask": 12 * F + 2 * 4 * F + 2 * 4 * F + 4 * V + 12 * F,     # faces, cluster + count, two flags, vflag zeroed, set
        "compact": 2 * 2 * 4 * V + 12 * V + 4 * V + 12 * V_out + 2 * 2 * 4 * F + 12 * F + 12 * F + 4 * F + 12 * F_out,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--freq", type=float, default=34.0)
    ap.add_argument("--blobs", type=int, default=60)
    ap.add_argument("--cluster-to-keep", type=int, default=1)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import mesh_clean_restated as R
    from volsurfs_amd.isosurface import marching_cubes
    from volsurfs_amd.mesh_clean import cluster_connected_triangles, post_process_mesh
    assert torch.cuda.is_available(), "mesh_clean_bench needs a GPU"
    small = R.seven_spheres()
    R.post_process_mesh(*small, 1)                                         # the host's warm-up
    rows = []
    for n in a.res:
        grid, nr_blobs = field(n, a.freq, a.blobs)
        mesh = marching_cubes(grid, 0.0, [-1.0] * 3, [2.0 / (n - 1)] * 3)[0]
        del grid
        V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
        row = {"resolution": n, "freq": a.freq, "blobs": nr_blobs, "vertices": V, "faces": F, "reps": a.reps,
               "cluster_to_keep": a.cluster_to_keep}
        cl, cnt, area = cluster_connected_triangles(mesh)
        out, st = post_process_mesh(mesh, a.cluster_to_keep, return_stats=True)
        row.update({k: st[k] for k in ("clusters", "threshold", "clusters_kept", "faces_out", "vertices_out")})
        row["largest_cluster_faces"] = int(cnt.max())
        sc = stage_medians(lambda d: cluster_connected_triangles(mesh, stage_ms=d), a.reps)
        sf = stage_medians(lambda d: post_process_mesh(mesh, a.cluster_to_keep, stage_ms=d), a.reps)
        row["stage_ms"] = {"clusters": {k: sc[k] for k in ("edges", "sort", "hook", "roots", "number", "areas")},
                           "filter": {k: sf[k] for k in ("edges", "sort", "hook", "roots", "number", "threshold",
                                                         "mask", "compact")}}
        row["clusters_ms"] = timed(lambda: cluster_connected_triangles(mesh), a.reps)
        row["post_process_ms"] = timed(lambda: post_process_mesh(mesh, a.cluster_to_keep), a.reps)
        nb = stage_bytes(V, F, st["clusters"], st["vertices_out"], st["faces_out"])
        row["stage_bytes"] = nb
        ms = dict(sf, areas=sc["areas"])
        row["GB_per_s"] = {k: round(nb[k] / (ms[k] * 1e-3) / 1e9, 1) for k in nb if ms[k] > 0}
        if not a.skip_host:
            v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
            t0 = time.perf_counter()
            want = R.post_process_mesh(v, f, a.cluster_to_keep)
            row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["host_threads"] = torch.get_num_threads()
            row["ratio"] = round(row["host_ms"] / row["post_process_ms"][0], 1)
            row["equal_to_host"] = bool(np.array_equal(out.faces.cpu().numpy(), want["faces"]) and
                                        out.vertices.cpu().numpy().tobytes() == want["vertices"].tobytes())
            del v, f, want
        rows.append(row)
        print(json.dumps(row), flush=True)
        del mesh, out, cl, cnt, area
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
