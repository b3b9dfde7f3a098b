"""Marching cubes (volsurfs_amd.isosurface, csrc/isosurface.hip): device time of the count pass (count kernel + scan +
totals, up to the host's read of the totals) and of the emit pass, from events after warm-up, for n^3 grids with
n in {256, 512, 1000}, K in {1, 5} levels, a sphere SDF and a noisy lobed SDF.  Beside each: GB/s of grid bytes
(4 n^3, one read of the grid) over the pass's time, V and F summed over the levels, `sample_grid`'s time for the
analytic field, and a RayTracer(builder="ploc") build of the K shells.

Each n runs in a child process of its own under `timeout`; the parent never opens the GPU and stops at the first
child that fails.  One JSON line per case, then a table.

    python tools/isosurface_bench.py [--reps 5] [--only 256,512,1000]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (256, 512, 1000)
STEP_TIMEOUT = 900
SPHERE_R, DELTA = 0.3, 0.01


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


def run_size(n, reps):
    import torch
    from volsurfs_amd import _lib
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.raytrace import RayTracer
    torch.cuda.init()
    out = []
    for name, fn in _fields().items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid = iso.sample_grid(fn, n, chunk=128)
        torch.cuda.synchronize()
        sample_ms = 1e3 * (time.perf_counter() - t0)
        for K in (1, 5):
            levels = [0.0] if K == 1 else [DELTA * (k - K // 2) for k in range(K)]
            ws = torch.empty(iso.workspace_bytes(grid.shape, K), dtype=torch.uint8, device="cuda")
            lv = (ctypes.c_float * K)(*levels)
            org, spc = (ctypes.c_float * 3)(-1.0, -1.0, -1.0), (ctypes.c_float * 3)(*[2.0 / (n - 1)] * 3)
            totals = (ctypes.c_longlong * (2 * K))()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

            def count():
                _lib.call("vsa_isosurface_count", grid, n, n, n, ctypes.cast(lv, ctypes.c_void_p), K, 0, ws,
                          ws.numel(), ctypes.cast(totals, ctypes.c_void_p), _lib.stream_ptr())

            count()
            verts = [torch.empty(int(totals[2 * L]), 3, device="cuda") for L in range(K)]
            faces = [torch.empty(int(totals[2 * L + 1]), 3, dtype=torch.int32, device="cuda") for L in range(K)]
            vp = (ctypes.c_void_p * K)(*[v.data_ptr() for v in verts])
            fp = (ctypes.c_void_p * K)(*[f.data_ptr() for f in faces])

            def emit():
                _lib.call("vsa_isosurface_emit", grid, n, n, n, ctypes.cast(lv, ctypes.c_void_p), K, 0,
                          ctypes.cast(org, ctypes.c_void_p), ctypes.cast(spc, ctypes.c_void_p), ws, ws.numel(),
                          ctypes.cast(totals, ctypes.c_void_p), ctypes.cast(vp, ctypes.c_void_p),
                          ctypes.cast(fp, ctypes.c_void_p), _lib.stream_ptr())

            emit()
            c_ms, e_ms = [], []
            for _ in range(reps):
                ev[0].record()
                count()
                ev[1].record()
                emit()
                ev[2].record()
                torch.cuda.synchronize()
                c_ms.append(ev[0].elapsed_time(ev[1]))
                e_ms.append(ev[1].elapsed_time(ev[2]))
            c, e = sorted(c_ms)[len(c_ms) // 2], sorted(e_ms)[len(e_ms) // 2]
            meshes = [iso._uvless(v, f) for v, f in zip(verts, faces)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            RayTracer(meshes, builder="ploc")
            torch.cuda.synchronize()
            ploc_ms = 1e3 * (time.perf_counter() - t0)
            gb = 4.0 * n ** 3 / 1e9
            row = {"n": n, "field": name, "K": K, "count_ms": round(c, 3), "emit_ms": round(e, 3),
                   "count_GBps": round(gb / (c / 1e3), 1), "emit_GBps": round(gb / (e / 1e3), 1),
                   "V": int(sum(totals[2 * L] for L in range(K))), "F": int(sum(totals[2 * L + 1] for L in range(K))),
                   "sample_grid_ms": round(sample_ms, 1), "ploc_build_ms": round(ploc_ms, 1),
                   "workspace_MB": round(ws.numel() / 2 ** 20, 1)}
            print(json.dumps(row), flush=True)
            out.append(row)
            del ws, verts, faces, meshes
        del grid
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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
    print("| n | field | K | count ms | emit ms | count GB/s | emit GB/s | V | F | sample_grid ms | ploc build ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['field']} | {r['K']} | {r['count_ms']} | {r['emit_ms']} | {r['count_GBps']} | "
              f"{r['emit_GBps']} | {r['V']} | {r['F']} | {r['sample_grid_ms']} | {r['ploc_build_ms']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
