"""Shell simplification (volsurfs_amd.simplify, csrc/simplify.hip) of marching-cubes shells: for n^3 grids with n in
{256, 512, 1000}, a sphere SDF and a noisy lobed SDF, K in {1, 5} levels (K = 5 at the reference's
delta_surfs = 0.0025) and ratios 0.1 / 0.025, one `simplify_mesh` call per shell.  Columns: F in and F out summed over
the shells, the largest round count, total ms per shell (wall, median of --reps runs after a warm-up) and its split by
stage (device ms from events, one extra run with stage timing), the max radial error on the sphere in grid spacings,
and for K = 5 the fraction of rays from the centre whose K hits are not in shell order after simplification (reported
only: the reference also simplifies each shell on its own).

Each n runs in a child process of its own under `timeout`; the parent never opens the GPU and stops at the first
child that fails.  One JSON line per case, then a table.

    python tools/simplify_bench.py [--reps 3] [--only 256,512,1000]
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
STEP_TIMEOUT = 1500
SPHERE_R, DELTA, NR_RAYS = 0.3, 0.0025, 1 << 16


def _fields():
    import torch

    def sphere(p):
        return torch.linalg.vector_norm(p, dim=-1)[:, None] - SPHERE_R

    def lobed(p):
        rad = torch.linalg.vector_norm(p, dim=-1)
        phi = torch.atan2(p[:, 1], p[:, 0])
        f = rad - 0.45 * (1.0 + 0.25 * torch.sin(4.0 * phi) * torch.cos(3.0 * p[:, 2]))
        noise = 0.01 * torch.sin(97.0 * p[:, 0]) * torch.sin(89.0 * p[:, 1]) * torch.sin(83.0 * p[:, 2])
        return (f + noise)[:, None]

    return {"sphere": sphere, "lobed_noisy": lobed}


def _centre_rays(n):
    """n Fibonacci-sphere directions from the origin."""
    import torch
    i = torch.arange(n, dtype=torch.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * torch.pi * (3.0 - 5.0 ** 0.5)
    r = (1.0 - z * z).sqrt()
    d = torch.stack([r * phi.cos(), r * phi.sin(), z], -1).float().cuda()
    return torch.zeros_like(d), d


def _out_of_order(meshes):
    import torch
    from volsurfs_amd.raytrace import RayTracer
    o, d = _centre_rays(NR_RAYS)
    t, slot, _ = RayTracer(meshes, builder="ploc").trace_all(o, d)
    bad = (slot < 0).any(0)
    for k in range(len(meshes) - 1):
        bad |= t[k] >= t[k + 1]
    return float(bad.to(torch.float32).mean())


def run_size(n, reps):
    import torch
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd import simplify as smp
    torch.cuda.init()
    h = 2.0 / (n - 1)
    out = []
    for name, fn in _fields().items():
        grid = iso.sample_grid(fn, n, chunk=128)
        for K in (1, 5):
            levels = [0.0] if K == 1 else iso.level_set_values(K, DELTA)
            shells = iso.marching_cubes(grid, levels, [-1.0] * 3, [h] * 3)
            for ratio in RATIOS:
                def run():
                    return [smp.simplify_mesh(m, ratio, return_stats=True) for m in shells]

                res = run()
                wall = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = run()
                    torch.cuda.synchronize()
                    wall.append(1e3 * (time.perf_counter() - t0) / K)
                stages = {k: 0.0 for k in smp.STAGES}
                for m in shells:
                    ms = {}
                    smp._simplify(m.vertices, m.faces, smp.target_faces(m.faces.shape[0], ratio), stage_ms=ms)
                    for k in stages:
                        stages[k] += ms[k] / K
                row = {"n": n, "field": name, "K": K, "ratio": ratio,
                       "F_in": sum(st["faces_in"] for _, st in res), "F_out": sum(st["faces_out"] for _, st in res),
                       "rounds": max(st["rounds"] for _, st in res), "stalled": any(st["stalled"] for _, st in res),
                       "ms_per_shell": round(sorted(wall)[len(wall) // 2], 2),
                       **{f"{k}_ms": round(v, 2) for k, v in stages.items()},
                       "workspace_MB": round(max(smp.workspace_bytes(m.vertices.shape[0], m.faces.shape[0])
                                                 for m in shells) / 2 ** 20, 1)}
                if name == "sphere":
                    err = 0.0
                    for (m, _), lv in zip(res, levels):
                        v = m.vertices.double()
                        err = max(err, float((torch.linalg.vector_norm(v, dim=-1) - (SPHERE_R + lv)).abs().max()))
                    row["max_radial_err_h"] = round(err / h, 4)
                if K > 1:
                    row["out_of_order"] = round(_out_of_order([m for m, _ in res]), 5)
                print(json.dumps(row), flush=True)
                out.append(row)
            del shells
        del grid
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        run_size(args.child, args.reps)
        return 0
    rows = []
    for n in (int(x) for x in args.only.split(",")):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", str(n),
               "--reps", str(args.reps)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(res.stdout)
        rows += [json.loads(x) for x in res.stdout.splitlines() if x.startswith("{")]
        if res.returncode != 0:
            print(f"n={n}: child exited with {res.returncode}; stopping", file=sys.stderr)
            return res.returncode
    print("| n | field | K | ratio | F in | F out | rounds | ms / shell | init | edges | cost | select | collapse | "
          "compact | max radial err (h) | out of order |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['field']} | {r['K']} | {r['ratio']} | {r['F_in']} | {r['F_out']} | {r['rounds']} | "
              f"{r['ms_per_shell']} | {r['init_ms']} | {r['edges_ms']} | {r['cost_ms']} | {r['select_ms']} | "
              f"{r['collapse_ms']} | {r['compact_ms']} | {r.get('max_radial_err_h', '-')} | "
              f"{r.get('out_of_order', '-')} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
