"""Texture export and load (volsurfs_amd.texture_export, csrc/texture_io.hip) of K = 5 nested shells at the default
textures_res (2048, 1024, 512, 256) and sh_degree 3: 80 PNGs, 182 MB of raw RGBA.  Columns: bake ms (wall);
vsa_nt_export_planes ms (device events, median of --reps after a warm-up); device-to-host ms of the images (wall);
PNG encode s and bytes on disk at compress_level 1 and 6 (16 host threads); and for load_scene at each level the OBJ
read s, PNG decode s, host-to-device ms (wall) and vsa_nt_import_planes ms (device events, median of --reps).

The case runs in a child process under `timeout`; the parent never opens the GPU.  One JSON line, then a table.

    python tools/texture_export_bench.py [--reps 5] [--out DIR]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, SUBDIV, RES, SH_DEGREE = 5, 4, (2048, 1024, 512, 256), 3
LEVELS = (1, 6)
STEP_TIMEOUT = 900


def _event_ms(fn, reps):
    import torch
    fn()                                                   # warm-up
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(400000)                          # keep the queue busy: the start stamp follows the launch
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def _child(reps, out_dir):
    import ctypes
    import torch
    from volsurfs_amd import _lib
    from volsurfs_amd import texture_export as tx
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.methods import VolSurfs
    m = VolSurfs(nested_shells(K=K, subdiv=SUBDIV), max_rays=4096, textures_res=RES, sh_degree=SH_DEGREE)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        m.bank.tables.copy_((torch.rand(m.bank.tables.shape, generator=g) * 2 - 1).cuda())
    m.bank.refresh_half_params()
    m.bake()                                               # warm-up
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.bake()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    bank = m.baked
    total = tx._planes_bytes(bank)
    planes = torch.empty(total, dtype=torch.uint8, device="cuda")
    export_ms = _event_ms(lambda: _lib.call("vsa_nt_export_planes", ctypes.byref(bank.plan), bank.slot_of,
                                            bank.seg_start, bank.texels, planes, total, _lib.stream_ptr()), reps)
    row = {"K": K, "textures_res": list(RES), "sh_degree": SH_DEGREE, "raw_bytes": total,
           "bake_ms": round(statistics.median(walls), 2), "export_kernel_ms": round(export_ms, 4)}
    for level in LEVELS:
        d = os.path.join(out_dir, f"level{level}")
        shutil.rmtree(d, ignore_errors=True)
        t = {}
        tx.extract_textures(m, d, compress_level=level, timings=t)
        tex = os.path.join(d, "textures")
        row.setdefault("d2h_ms", round(t["d2h_ms"], 2))
        row[f"png_encode_s_{level}"] = round(t["png_s"], 3)
        row[f"bytes_on_disk_{level}"] = sum(os.path.getsize(os.path.join(tex, f)) for f in os.listdir(tex))
        lt = {}
        scene = tx.load_scene(d, timings=lt)
        row[f"load_meshes_s_{level}"] = round(lt["meshes_s"], 3)
        row[f"png_decode_s_{level}"] = round(lt["png_s"], 3)
        row[f"h2d_ms_{level}"] = round(lt["h2d_ms"], 2)
        if level == LEVELS[0]:
            b = scene.baked
            row["import_kernel_ms"] = round(_event_ms(lambda: _lib.call(
                "vsa_nt_import_planes", ctypes.byref(b.plan), planes, total, b.slot_of, b.seg_start, b.texels,
                _lib.stream_ptr()), reps), 4)
        del scene
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="directory for the exported scenes (default: a temporary one)")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        _child(a.reps, a.out)
        return
    out = a.out or tempfile.mkdtemp(prefix="texture_export_bench_")
    try:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child",
               "--reps", str(a.reps), "--out", out]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        rows = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
        for r in rows:
            print(json.dumps(r))
        if res.returncode != 0:
            print(f"child failed with status {res.returncode}", file=sys.stderr)
            sys.exit(res.returncode)
    finally:
        if a.out is None:
            shutil.rmtree(out, ignore_errors=True)
    keys = ["bake_ms", "export_kernel_ms", "d2h_ms"] + [f"{k}_{lv}" for lv in LEVELS for k in
                                                         ("png_encode_s", "bytes_on_disk")] + \
        ["import_kernel_ms"] + [f"{k}_{lv}" for lv in LEVELS for k in ("load_meshes_s", "png_decode_s", "h2d_ms")]
    print("| " + " | ".join(keys) + " |")
    print("|" + "---|" * len(keys))
    for r in rows:
        print("| " + " | ".join(str(r[k]) for k in keys) + " |")


if __name__ == "__main__":
    main()
