"""UV atlases (volsurfs_amd.atlas, csrc/atlas.hip) of simplified marching-cubes shells: for n^3 grids with n in
{256, 512, 1000}, a sphere SDF and a noisy lobed SDF, K = 5 levels at the reference's delta_surfs = 0.0025, each shell
simplified to 0.1 and 0.025 and then atlased at resolution 1024, padding 4.  Columns: faces summed over the shells,
charts and split rounds (summed / largest), mean and lowest utilization (covered texels / R^2), ms per shell (wall,
median of --reps runs after a warm-up) and its split by stage (device ms from events, one extra run with stage timing,
averaged per shell).

`--charts box,merged --min-cos 0.5,0.4,0.3` atlases the same shells once per mode (box, then merged at every min_cos)
in the same process, so the box rows are the baseline of the merged ones: merged rows add the box charts before
merging, the groups after it (summed), the merge rounds run (largest), the valid pairs left (summed), the texel density
(mean and lowest) and the `merge` stage.  `--out` writes the rows as JSON.

Each n runs in a child process of its own under `timeout`; the parent never opens the GPU and stops at the first child
that fails.  One JSON line per case, then a table.

    python tools/atlas_bench.py [--reps 3] [--only 256,512,1000] [--charts box,merged] [--min-cos 0.5,0.4,0.3]
                                [--ratios 0.1,0.025] [--out profiles/atlas_merge.json]
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


def _modes(charts, min_cos):
    """[(label, compute_atlas keywords)]: box once, merged once per min_cos."""
    out = []
    for c in charts:
        if c == "box":
            out.append(("box", {}))
        elif c == "merged":
            out += [(f"merged {mc}", {"charts": "merged", "min_cos": mc}) for mc in min_cos]
        else:
            raise SystemExit(f"--charts: unknown mode {c!r}")
    return out


def _child(n, reps, modes, ratios):
    import statistics
    import torch
    from tools.simplify_bench import _fields
    from volsurfs_amd import atlas, isosurface as iso
    from volsurfs_amd.simplify import simplify_mesh
    for name, fn in _fields().items():
        meshes, _ = iso.extract_level_sets(fn, n, K, delta_surfs=DELTA)
        for ratio in ratios:
            simp = [simplify_mesh(m, ratio) for m in meshes]
            for mode, kw in modes:
                for m in simp:                                     # warm-up
                    atlas.compute_atlas(m, RES, PAD, **kw)
                walls = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = [atlas.compute_atlas(m, RES, PAD, return_stats=True, **kw) for m in simp]
                    torch.cuda.synchronize()
                    walls.append((time.perf_counter() - t0) * 1e3 / K)
                names = atlas.MERGED_STAGES if kw else atlas.STAGES
                stages = {k: 0.0 for k in names}
                for m in simp:
                    ms = {}
                    atlas.compute_atlas(m, RES, PAD, stage_ms=ms, **kw)
                    for k in stages:
                        stages[k] += ms[k] / K
                st = [s for _, s in out]
                row = {
                    "n": n, "field": name, "K": K, "ratio": ratio, "mode": mode,
                    "faces": sum(int(m.faces.shape[0]) for m in simp),
                    "charts": sum(s["charts"] for s in st), "max_split_rounds": max(s["split_rounds"] for s in st),
                    "scale_mean": round(sum(s["scale"] for s in st) / K, 2),
                    "scale_min": round(min(s["scale"] for s in st), 2),
                    "utilization_mean": round(sum(s["utilization"] for s in st) / K, 4),
                    "utilization_min": round(min(s["utilization"] for s in st), 4),
                    "ms_per_shell": round(statistics.median(walls), 2),
                    "stage_ms": {k: round(v, 2) for k, v in stages.items()}}
                if kw:
                    row.update(box_charts=sum(s["box_charts"] for s in st), groups=sum(s["groups"] for s in st),
                               max_merge_rounds=max(s["merge_rounds"] for s in st),
                               valid_pairs_left=sum(s["valid_pairs_left"] for s in st))
                print(json.dumps(row), flush=True)
        del meshes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--charts", default="box")
    ap.add_argument("--min-cos", default="0.5")
    ap.add_argument("--ratios", default=",".join(str(r) for r in RATIOS))
    ap.add_argument("--out", default="")
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    modes = _modes(a.charts.split(","), [float(x) for x in a.min_cos.split(",")])
    ratios = [float(x) for x in a.ratios.split(",")]
    if a.child:
        _child(a.child, a.reps, modes, ratios)
        return
    rows = []
    for n in (int(x) for x in a.only.split(",")):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", str(n),
               "--reps", str(a.reps), "--charts", a.charts, "--min-cos", a.min_cos, "--ratios", a.ratios]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in res.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
        if res.returncode != 0:
            print(f"n={n}: child exited with {res.returncode}; stopping", file=sys.stderr)
            sys.exit(res.returncode)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/atlas_bench.py", "K": K, "delta_surfs": DELTA, "resolution": RES, "padding": PAD,
                       "reps": a.reps, "rows": rows}, f, indent=1)
    merged = any(kw for _, kw in modes)
    stages = ("label", "charts", "pack", "emit", "raster") + (("merge",) if merged else ())
    head = "| n | field | ratio | " + ("mode | " if merged else "") + "faces | " + \
        ("box charts | groups | merge rounds | pairs left | " if merged else "") + \
        "charts | max split rounds | " + ("scale mean | scale min | " if merged else "") + \
        "util mean | util min | ms / shell | " + " | ".join(stages) + " |"
    print(head)
    print("|" + "---|" * (head.count("|") - 1))
    for r in rows:
        line = f"| {r['n']} | {r['field']} | {r['ratio']} | "
        if merged:
            line += f"{r['mode']} | "
        line += f"{r['faces']} | "
        if merged:
            line += " | ".join(str(r.get(k, "-")) for k in ("box_charts", "groups", "max_merge_rounds",
                                                            "valid_pairs_left")) + " | "
        line += f"{r['charts']} | {r['max_split_rounds']} | "
        if merged:
            line += f"{r['scale_mean']} | {r['scale_min']} | "
        line += f"{r['utilization_mean']} | {r['utilization_min']} | {r['ms_per_shell']} | "
        line += " | ".join(str(r["stage_ms"].get(k, "-")) for k in stages) + " |"
        print(line)


if __name__ == "__main__":
    main()
