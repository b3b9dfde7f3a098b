"""UV atlases (volsurfs_amd.atlas, csrc/atlas.hip) of simplified marching-cubes shells: for n^3 grids with n in
{256, 512, 1000}, a sphere SDF and a noisy lobed SDF, K = 5 levels at the reference's delta_surfs = 0.0025, each shell
simplified to 0.1 and 0.025 and then atlased at resolution 1024, padding 4.  Columns: faces summed over the shells,
charts and split rounds (summed / largest), mean and lowest utilization (covered texels / R^2), ms per shell (wall,
median of --reps runs after a warm-up) and its split by stage (device ms from events, one extra run with stage timing,
averaged per shell).

Each n runs in a child process of its own under `timeout`; the parent never opens the GPU and stops at the first child
that fails.  One JSON line per case, then a table.

    python tools/atlas_bench.py [--reps 3] [--only 256,512,1000]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (256, 512, 1000)
RATIOS = (0.1, 0.025)
K, DELTA, RES, PAD = 5, 0.0025, 1024, 4
STEP_TIMEOUT = 1500


def _child(n, reps):
    import statistics
    import torch
    from tools.simplify_bench import _fields
    from volsurfs_amd import atlas, isosurface as iso
    from volsurfs_amd.simplify import simplify_mesh
    for name, fn in _fields().items():
        meshes, _ = iso.extract_level_sets(fn, n, K, delta_surfs=DELTA)
        for ratio in RATIOS:
            simp = [simplify_mesh(m, ratio) for m in meshes]
            for m in simp:                                     # warm-up
                atlas.compute_atlas(m, RES, PAD)
            walls = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = [atlas.compute_atlas(m, RES, PAD, return_stats=True) for m in simp]
                torch.cuda.synchronize()
                walls.append((time.perf_counter() - t0) * 1e3 / K)
            stages = {k: 0.0 for k in atlas.STAGES}
            for m in simp:
                ms = {}
                atlas.compute_atlas(m, RES, PAD, stage_ms=ms)
                for k in stages:
                    stages[k] += ms[k] / K
            st = [s for _, s in out]
            print(json.dumps({
                "n": n, "field": name, "K": K, "ratio": ratio, "faces": sum(int(m.faces.shape[0]) for m in simp),
                "charts": sum(s["charts"] for s in st), "max_split_rounds": max(s["split_rounds"] for s in st),
                "utilization_mean": round(sum(s["utilization"] for s in st) / K, 4),
                "utilization_min": round(min(s["utilization"] for s in st), 4),
                "ms_per_shell": round(statistics.median(walls), 2),
                "stage_ms": {k: round(v, 2) for k, v in stages.items()}}), flush=True)
        del meshes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        _child(a.child, a.reps)
        return
    rows = []
    for n in (int(x) for x in a.only.split(",")):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", str(n),
               "--reps", str(a.reps)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in res.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
        if res.returncode != 0:
            print(f"n={n}: child exited with {res.returncode}; stopping", file=sys.stderr)
            sys.exit(res.returncode)
    print("| n | field | ratio | faces | charts | max split rounds | util mean | util min | ms / shell | "
          + " | ".join(("label", "charts", "pack", "emit", "raster")) + " |")
    for r in rows:
        print(f"| {r['n']} | {r['field']} | {r['ratio']} | {r['faces']} | {r['charts']} | {r['max_split_rounds']} | "
              f"{r['utilization_mean']} | {r['utilization_min']} | {r['ms_per_shell']} | "
              + " | ".join(str(v) for v in r["stage_ms"].values()) + " |")


if __name__ == "__main__":
    main()
