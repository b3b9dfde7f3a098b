"""Teacher distillation (volsurfs_amd.camera.VirtualCameras / mixed_rays_batch, trainer.train(teacher_method=...);
csrc/hemisphere_camera.h) on one GPU, in one process.

1. The mixed batch [virtual | real] at the ray counts of `bench.py --workload train` (its first batch of 512 and the
   count its dynamic rule settles at, measured here), each --reps times after a warm-up, between device events, median
   (min - max) in ms, and the host clock around the same calls with a synchronise:
     fused      `mixed_rays_batch`: one launch into single allocations;
     composed   `VirtualCameras.get_next_rays_batch` + `TensorReel.get_next_rays_batch` + the torch.cat's of
                trainer.py:209-214 (two launches, four concatenations);
     host       the reference-shaped path: 100 `Camera.look_at` on the host (at the call's own camera centres, read
                back), a new `TensorReel` of them, a batch from it, the real batch, the torch.cat's.
   For each, whether its rays equal the fused path's (the host path's poses equal to rounding only, and its reel draws
   from its own stream: its virtual rays differ, its real half must not).
2. `trainer.train_step_from_reel` on the bench's training shells (K = 5, subdiv 6, 50 views of 800 x 800, dynamic ray
   count -> 49 152 hits) against `train_step_distilled` with a small NeRF teacher on the same shells: iterations per
   second, and the teacher's render between device events as a share of the iteration.
Every figure is recorded as it comes out.  Needs a GPU; writes one JSON file.

    python tools/distill_bench.py [--out profiles/distill.json] [--reps 20] [--steps 200] [--warmup 100]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def _timed(fn, reps, warmup=3):
    """(device ms stats, host ms stats incl. a synchronise, the last result) of fn()."""
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return _stats(dev), _stats(host), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--shells", type=int, default=5)
    ap.add_argument("--subdiv", type=int, default=6)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--target-hits", type=int, default=49152)
    a = ap.parse_args()

    import torch
    from bench import GRAD_CHAIN_GAIN, synthetic_reel
    from volsurfs_amd import camera as C
    from volsurfs_amd.background import BoundingSphere
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.nerf import NeRF, NeRFHyperParams
    from volsurfs_amd.trainer import train_step, train_step_distilled, train_step_from_reel
    from volsurfs_amd.volsurfs import _Pcg32State
    dev = "cuda"
    torch.manual_seed(42)
    reel = synthetic_reel(a.views, a.res, dev, seed=42)
    radius = float(reel.c2w[:, :, 3].norm(dim=1).mean())
    up = (1, -1)                                     # the synthetic reel's cameras look at the origin with up = -y
    out = {"device": torch.cuda.get_device_name(0),
           "config": {"shells": a.shells, "subdiv": a.subdiv, "views": a.views, "res": a.res,
                      "target_hits": a.target_hits, "reps": a.reps, "steps": a.steps, "warmup": a.warmup,
                      "virtual_cameras": 100, "radius": radius}}

    # ---- 2. the training loop with and without a teacher (first: it also finds the settled ray count)
    def loop(teacher):
        torch.manual_seed(42)
        method = VolSurfs(nested_shells(K=a.shells, subdiv=a.subdiv, device=dev), max_rays=1 << 17, nr_warmup_iters=500,
                          seed=42)
        method.init_optim()
        reel.rng.__init__()
        virtual = C.VirtualCameras(reel.intrinsics[0], reel.height, reel.width, radius, 100, *up)
        state = {"nr_rays": 512, "it": 0}
        share = []
        if teacher is not None:              # the teacher's render between device events
            inner = teacher.render

            def render(*args, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = inner(*args, **kw)
                e1.record()
                share.append((e0, e1))
                return r
            teacher.render = render

        def one():
            n = state["nr_rays"]
            method.grad_scale = GRAD_CHAIN_GAIN * float(n if teacher is None else 2 * (n // 2))
            kw = dict(jitter_pixels=True, iter_nr=state["it"], is_first_iter=state["it"] == 0,
                      target_nr_of_training_samples=a.target_hits, sync_losses=False)
            if teacher is None:
                _, nxt = train_step_from_reel(method, reel, n, **kw)
            else:
                _, nxt = train_step_distilled(method, virtual, reel, teacher, n, **kw)
            state["nr_rays"] = max(64, min(int(nxt), 4 * (1 << 17)))
            state["it"] += 1
        for _ in range(max(1, a.warmup)):
            one()
        torch.cuda.synchronize()
        share.clear()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            one()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res = {"it_per_s": round(a.steps / dt, 1), "ms_per_it": round(dt / a.steps * 1e3, 4),
               "nr_rays_settled": state["nr_rays"]}
        if teacher is not None:
            ms = [e0.elapsed_time(e1) for e0, e1 in share]
            res["teacher_render_ms"] = _stats(ms)
            res["teacher_share_of_iteration"] = round(statistics.median(ms) / (dt / a.steps * 1e3), 3)
            teacher.render = inner
        return res

    out["train_without_teacher"] = loop(None)
    torch.manual_seed(7)
    # a small teacher: a NeRF of default hyper-parameters, 100 iterations towards a grey scene on a black background,
    # so that its occupancy grid and its samples per ray are a trained model's and not an empty one's
    teacher = NeRF(True, NeRFHyperParams(nr_warmup_iters=10), None, None, BoundingSphere(0.5), bg_color=(0.0, 0.0, 0.0))
    o = torch.nn.functional.normalize(torch.randn(4096, 3, device=dev), dim=1) * 1.5
    d = torch.nn.functional.normalize(torch.rand(4096, 3, device=dev) * 0.4 - 0.2 - o, dim=1)
    grey = torch.full((4096, 3), 0.5, device=dev)
    for it in range(100):
        train_step(teacher, o, d, grey, None, iter_nr=it, is_first_iter=it == 0)
    teacher.is_training = False
    opacity = float(teacher.render(o, d)["weights_sum"].mean())
    out["train_with_nerf_teacher"] = loop(teacher)
    out["train_with_nerf_teacher"]["teacher"] = {"method": "NeRF, default hyper-parameters, 100 iterations on 4 096 rays",
                                                 "mean_opacity_of_its_training_rays": round(opacity, 3)}
    print(json.dumps({k: out[k] for k in ("train_without_teacher", "train_with_nerf_teacher")}))

    # ---- 1. the mixed batch at the training batch sizes
    out["batch"] = {}
    for n in sorted({512, int(out["train_without_teacher"]["nr_rays_settled"])}):
        h = n // 2
        virtual = C.VirtualCameras(reel.intrinsics[0], reel.height, reel.width, radius, 100, *up)
        seeds = {}

        def mark():                           # every path starts a repetition from the same two streams
            seeds["v"], seeds["r"] = (virtual.rng.state, virtual.rng.inc), (reel.rng.state, reel.rng.inc)

        def rewind():
            (virtual.rng.state, virtual.rng.inc), (reel.rng.state, reel.rng.inc) = seeds["v"], seeds["r"]
        mark()

        def fused():
            rewind()
            o, d, gt, _, _, _ = C.mixed_rays_batch(virtual, reel, h, h, True, 1)
            return o, d, gt

        def composed():
            rewind()
            _, ov, dv, _ = virtual.get_next_rays_batch(h, True)
            _, orr, dr, vals, _ = reel.get_next_rays_batch(h, True, 1)
            gt_v = torch.empty(h, 3, device=dev)                        # (the teacher's colours)
            return (torch.cat([ov, orr]), torch.cat([dv, dr]), torch.cat([gt_v, vals["rgb"]]),
                    torch.cat([torch.ones(h, 1, device=dev), torch.ones(h, 1, device=dev)]))

        focal = float(reel.intrinsics[0][0, 0])
        blank = torch.zeros(100, reel.height, reel.width, 3, device=dev)    # (not counted: the reference's reel of
        host_rng = _Pcg32State()                                             # virtual cameras holds no images)

        def host():
            rewind()
            centres = virtual.poses()[:, :, 3].cpu().tolist()           # (the reference samples them on the host)
            cams = [C.Camera.look_at(tuple(c), up=(0.0, -1.0, 0.0), focal=focal, height=reel.height, width=reel.width,
                                     device=dev) for c in centres]
            vreel = C.TensorReel(cams, blank, device=dev)
            vreel.rng = host_rng
            _, ov, dv, _, _ = vreel.get_next_rays_batch(h, True, 1)
            _, orr, dr, vals, _ = reel.get_next_rays_batch(h, True, 1)
            gt_v = torch.empty(h, 3, device=dev)
            return (torch.cat([ov, orr]), torch.cat([dv, dr]), torch.cat([gt_v, vals["rgb"]]),
                    torch.cat([torch.ones(h, 1, device=dev), torch.ones(h, 1, device=dev)]))

        e = {}
        ref = None
        for name, fn in (("fused", fused), ("composed", composed), ("host", host)):
            d_ms, h_ms, res = _timed(fn, a.reps)
            e[name] = {"device_ms": d_ms, "host_ms_with_sync": h_ms}
            if ref is None:
                ref = res
            else:
                e[name]["rays_equal_fused"] = bool(torch.equal(res[0], ref[0]) and torch.equal(res[1], ref[1]))
                e[name]["real_half_equal_fused"] = bool(torch.equal(res[0][h:], ref[0][h:]) and
                                                        torch.equal(res[1][h:], ref[1][h:]) and
                                                        torch.equal(res[2][h:], ref[2][h:]))
        out["batch"][str(n)] = e
        print(json.dumps({"nr_rays": n, **e}))

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
