"""Loading a scene (volsurfs_amd.datasets, csrc/image_prepare.hip): the image preparation on the device
against the composition a user would write on the host, and a whole `MVDataset` load, in one process on one GPU.

Input: --views RGBA views of --size x --size made in memory (a smooth pattern behind a disc of alpha, so that the PNGs
compress as renders do), at subsample factors 1 and 2.  Timed, each --reps times after a warm-up, median (min - max) in ms:
  device          host clock around: upload of the bytes, `vsa_images_prepare`, a device synchronise;
  kernel          `vsa_images_prepare` alone, between device events (bytes already resident), with the bytes it moves
                  (read ch + written 12 + 4 per output pixel) over that time;
  host            the same rule in numpy on the host (integer sums, float32 divisions) plus the upload of the float
                  stacks and a synchronise: what a user composes without this module.  Its result is compared with the
                  device's, bit for bit;
  load            `MVDataset` of the same views written as a Blender-format scene to a temporary directory, with its
                  parse / decode / prepare host seconds apart.
Needs a GPU; writes one JSON file.

    python tools/datasets_bench.py [--out profiles/datasets.json] [--views 100] [--size 800] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _views(C, n):
    import numpy as np
    y, x = np.mgrid[0:n, 0:n].astype(np.float32) / n
    out = np.empty((C, n, n, 4), np.uint8)
    for c in range(C):
        ph = 0.37 * c
        out[c, ..., 0] = 127.5 + 127.5 * np.sin(9.0 * x + ph)
        out[c, ..., 1] = 127.5 + 127.5 * np.sin(7.0 * y - ph)
        out[c, ..., 2] = 255.0 * (0.5 * x + 0.5 * y)
        r = np.hypot(x - 0.5 - 0.1 * np.cos(ph), y - 0.5 - 0.1 * np.sin(ph))
        out[c, ..., 3] = np.clip((0.33 - r) * 40.0, 0.0, 1.0) * 255.0
    return out


def _host_rule(src, s, bg):
    import numpy as np
    C, H0, W0, ch = src.shape
    H, W, n = H0 // s, W0 // s, s * s
    b = src[:, :H * s, :W * s].reshape(C, H, s, W, s, ch)
    a = b[..., 3].astype(np.uint32)
    A = a.sum(axis=(2, 4), dtype=np.uint32)
    P = (b[..., :3].astype(np.uint32) * a[..., None]).sum(axis=(2, 4), dtype=np.uint32)
    alpha = A.astype(np.float32) / np.float32(255 * n)
    rgb = P.astype(np.float32) / np.float32(65025 * n) + (np.float32(1.0) - alpha)[..., None] * np.asarray(bg, np.float32)
    return rgb, alpha


def _stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "datasets.json"))
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("datasets_bench needs a GPU")
    from volsurfs_amd import datasets as D
    from volsurfs_amd.camera import Camera

    C, n, bg = a.views, a.size, (1.0, 1.0, 1.0)
    src = _views(C, n)
    result = {"device": torch.cuda.get_device_name(0), "views": C, "size": n, "reps": a.reps, "host_cpus": os.cpu_count(),
              "torch_threads": torch.get_num_threads()}

    def wall(fn):
        ms = []
        for i in range(a.reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i:
                ms.append(1e3 * (time.perf_counter() - t))
        return _stats(ms)

    for s in (1, 2):
        row = {}
        row["device_ms"] = wall(lambda: D.prepare_images(torch.from_numpy(src).cuda(), None, s, bg))
        src_d = torch.from_numpy(src).cuda()
        ms = []
        for i in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rgb_d, mask_d = D.prepare_images(src_d, None, s, bg)
            e1.record()
            torch.cuda.synchronize()
            if i:
                ms.append(e0.elapsed_time(e1))
        row["kernel_ms"] = _stats(ms)
        H, W = n // s, n // s
        moved = C * (H * s * W * s * 4 + H * W * 16)
        row["kernel_bytes"] = moved
        row["kernel_GBps"] = round(moved / (row["kernel_ms"]["median"] * 1e-3) / 1e9, 1)

        def host():
            rgb, alpha = _host_rule(src, s, bg)
            return torch.from_numpy(rgb).cuda(), torch.from_numpy(alpha).cuda()

        row["host_ms"] = wall(host)
        rgb_h, mask_h = host()
        row["host_equals_device"] = bool(torch.equal(rgb_h.view(torch.int32), rgb_d.view(torch.int32))
                                         and torch.equal(mask_h.view(torch.int32), mask_d.view(torch.int32)))
        row["host_over_device"] = round(row["host_ms"]["median"] / row["device_ms"]["median"], 2)
        del src_d, rgb_d, mask_d, rgb_h, mask_h
        torch.cuda.empty_cache()
        result[f"s{s}"] = row
        print(json.dumps({f"s{s}": row}), flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        cams = [Camera.look_at((4.0 * np.cos(0.1 * i), 0.5, 4.0 * np.sin(0.1 * i)), focal=1111.0, height=n, width=n,
                               device="cpu") for i in range(C)]
        t = time.perf_counter()
        D.write_blender_scene(os.path.join(tmp, "blender", "bench"), {"train": (cams, src)})
        row = {"write_s": round(time.perf_counter() - t, 3),
               "png_bytes": sum(os.path.getsize(os.path.join(tmp, "blender", "bench", "train", f))
                                for f in os.listdir(os.path.join(tmp, "blender", "bench", "train")))}
        for s in (1, 2):
            cfg = {"blender": {"white_bg": True, "subsample_factor": s}}
            total, parts = [], []
            for i in range(a.reps + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                mv = D.MVDataset("blender", "bench", tmp, splits=["train"], config=cfg)
                torch.cuda.synchronize()
                if i:
                    total.append(1e3 * (time.perf_counter() - t))
                    parts.append(mv.timings)
                del mv
            row[f"s{s}"] = {"load_ms": _stats(total),
                            **{k[:-2] + "_ms": _stats([1e3 * p[k] for p in parts]) for k in parts[0]}}
        result["load"] = row
        print(json.dumps({"load": row}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
