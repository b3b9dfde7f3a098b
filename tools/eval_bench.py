"""Held-out-view metrics (volsurfs_amd.evaluation.image_metrics, csrc/image_metrics.hip): microseconds per view and
achieved GB/s (bytes the definition must read: pred + gt once, over the kernel pair's device time) for B in {1, 16, 100}
views of 800x800, 1920x1080 and 1600x1200, fp32 pred + uint8 gt and uint8 + uint8; beside it the same metric as
torch ops on the GPU (avg_pool2d + grouped conv2d, fp32).  Then render_camera of one 800x800 view of a configs[1]-sized
method (5 nested shells, subdiv 6), so the metric's share of an evaluation is visible.

Each size runs in a child process of its own under `timeout`; the parent never opens the GPU and stops at the first
child that fails.  One JSON line per measurement, then a table.

    python tools/eval_bench.py [--reps 50] [--only 800x800,1920x1080,1600x1200,render]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"800x800": (800, 800), "1920x1080": (1080, 1920), "1600x1200": (1200, 1600)}
BATCHES = (1, 16, 100)
STEP_TIMEOUT = 600


def device_us(fn, reps, warmup=5):
    """Mean device time of fn() in microseconds between two events around `reps` back-to-back calls, after warm-up."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def torch_metric(pred, gt, f):
    """The same definition as torch ops on [B,H,W,3] (fp32 or uint8 -> u8 / 255): psnr and ssim per image."""
    import torch
    import torch.nn.functional as F
    x = pred.permute(0, 3, 1, 2).float()
    y = gt.permute(0, 3, 1, 2).float()
    if pred.dtype == torch.uint8:
        x = x / 255.0
    else:
        x = torch.trunc(x.clamp(0, 1) * 255.0) / 255.0
    if gt.dtype == torch.uint8:
        y = y / 255.0
    psnr = -10 * torch.log10(((x - y) ** 2).mean((1, 2, 3)) + 1e-8)
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    d = torch.arange(11, dtype=torch.float32, device=x.device) - 5
    g = torch.exp(-(d[None] ** 2 + d[:, None] ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).expand(3, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, g, groups=3)  # noqa: E731
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx ** 2, conv(y * y) - my ** 2, conv(x * y) - mx * my
    cs = (2 * sxy + 0.03 ** 2) / (sxx + syy + 0.03 ** 2)
    ss = (2 * mx * my + 0.01 ** 2) / (mx ** 2 + my ** 2 + 0.01 ** 2) * cs
    return psnr, ss.mean((1, 2, 3))


def run_size(name, reps):
    import torch
    from volsurfs_amd.evaluation import image_metrics, pool_factor
    H, W = SIZES[name]
    f = pool_factor(H, W)
    g = torch.Generator(device="cuda").manual_seed(0)
    top = max(BATCHES)
    pred32 = torch.rand(top, H, W, 3, device="cuda", generator=g)
    pred8 = (torch.rand(top, H, W, 3, device="cuda", generator=g) * 255).to(torch.uint8)
    gt8 = (torch.rand(top, H, W, 3, device="cuda", generator=g) * 255).to(torch.uint8)
    for kind, pred in (("f32+u8", pred32), ("u8+u8", pred8)):
        for B in BATCHES:
            p, t = pred[:B], gt8[:B]
            us = device_us(lambda: image_metrics(p, t), reps)
            t_us = device_us(lambda: torch_metric(p, t, f), max(3, reps // 10), warmup=2)
            nbytes = B * H * W * 3 * (p.element_size() + 1)
            print(json.dumps({"size": name, "inputs": kind, "B": B, "pool": f, "us": round(us, 2),
                              "us_per_view": round(us / B, 2), "GBps": round(nbytes / us / 1e3, 1),
                              "torch_us_per_view": round(t_us / B, 2)}), flush=True)


def run_render(reps):
    import torch
    from volsurfs_amd.camera import Camera
    from volsurfs_amd.evaluation import image_metrics
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.methods import VolSurfs
    m = VolSurfs(nested_shells(K=5, subdiv=6), max_rays=800 * 800)
    m.is_training = False
    cam = Camera.look_at((0.0, 0.0, -1.5), focal=1111.1, height=800, width=800)
    render_us = device_us(lambda: m.render_camera(cam), max(3, reps // 5), warmup=3)
    gt = (torch.rand(1, 800, 800, 3, device="cuda") * 255).to(torch.uint8)
    img = m.render_camera(cam)["rgb"][None].contiguous()
    metric_us = device_us(lambda: image_metrics(img, gt), reps)
    print(json.dumps({"size": "render", "render_camera_us": round(render_us, 1), "metric_us": round(metric_us, 2),
                      "metric_share": round(metric_us / render_us, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default=",".join(list(SIZES) + ["render"]))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        if args.child == "render":
            run_render(args.reps)
        else:
            run_size(args.child, args.reps)
        return
    lines = []
    for name in args.only.split(","):
        if name not in SIZES and name != "render":
            raise SystemExit(f"unknown size {name!r}")
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__),
               "--reps", str(args.reps), "--child", name]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        lines += [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
        if r.returncode != 0:
            raise SystemExit(f"{name}: exit status {r.returncode}; stopping")
    print("\n| size | inputs | B | us / view | GB/s | torch us / view |\n|---|---|---|---|---|---|")
    for d in lines:
        if d["size"] != "render":
            print(f"| {d['size']} | {d['inputs']} | {d['B']} | {d['us_per_view']} | {d['GBps']} | "
                  f"{d['torch_us_per_view']} |")
    for d in lines:
        if d["size"] == "render":
            print(f"\nrender_camera 800x800 (configs[1]-sized): {d['render_camera_us']} us; metric {d['metric_us']} us "
                  f"= {100 * d['metric_share']:.2f} %")


if __name__ == "__main__":
    main()
