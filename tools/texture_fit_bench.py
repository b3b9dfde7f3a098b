"""Texture fit (volsurfs_amd.texture_fit, csrc/texel_fit.hip) on the LOD scenes of DESIGN §40 (b): the
five lobed shells of tools/texture_transfer_bench.py with its noise-like baked source, `simplify_shells` at 0.25, atlased
and transferred with textures at 1024 / 512 / 256 / 128 and at 512 / 256 / 128 / 64 (samples 1), then `fit_textures`
against renders of the source from hemisphere cameras at the orbit's distance.  One process, one GPU; every figure is recorded as it comes out, a small or zero gain included;
no figure is a pass condition.

  quality     PSNR / SSIM against the source over the 8 orbit views of the transfer bench, which no fit sees, before and
              after the fit, per learning rate of the sweep {1e-3, 3e-3, 1e-2, 3e-2}; the loss curve of every fit.
  iteration   device ms per iteration (events around the loop) and per entry point (`_lib.kernel_events`), grouped into
              rays / trace / shade / composite + L1 / shade backward / step.
  step        the step kernel alone after one accumulated view: ms (median of --reps after a warm-up), the share of idle
              quads, the bytes it has to move (8 per idle quad, 116 per live one, 4 per texel of slot look-up) and their
              rate against the 6.29 TB/s a float4 copy reaches on this part; a step with every quad live, measured, and
              the time the same bytes take at the copy rate: what the lazy rule is judged against.

    python tools/texture_fit_bench.py [--out profiles/texture_fit.json] [--n 512] [--iterations 400] [--train-views 48]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LRS = (1e-3, 3e-3, 1e-2, 3e-2)
COPY_TBS = 6.29              # a float4 copy on this part
GROUPS = {"vsa_camera_rays": "rays", "vsa_trace": "trace", "vsa_trace_q": "trace", "vsa_trace_q_fb": "trace",
          "vsa_trace_q_narrow": "trace", "vsa_nt_mark": "shade", "vsa_nt_shade_fwd": "shade",
          "vsa_composite_dense_fwd_bwd_l1": "composite_l1", "vsa_l1_mean": "composite_l1",
          "vsa_nt_shade_bwd": "shade_bwd", "vsa_texel_fit_step": "step"}


def _train_cameras(n, size):
    """n cameras on the two z hemispheres at the orbit's distance and focal length: none of them an orbit view."""
    import torch
    from volsurfs_amd.camera import sample_cameras_on_hemisphere
    from volsurfs_amd.volsurfs import _Pcg32State
    f = 1.1 * size
    K = torch.tensor([[f, 0.0, 0.5 * size], [0.0, f, 0.5 * size], [0.0, 0.0, 1.0]])
    rng = _Pcg32State()
    return (sample_cameras_on_hemisphere(K, size, size, 1.6, (n + 1) // 2, up_sign=1, rng=rng) +
            sample_cameras_on_hemisphere(K, size, size, 1.6, n // 2, up_sign=-1, rng=rng))


def _quads(bank):
    from volsurfs_amd.neural_textures import ROW_QUADS
    return sum(bank.K * bank.tex_res[d] ** 2 * ROW_QUADS[d] for d in range(bank.D))


def _step_bytes(bank, live):
    texels = sum(bank.K * bank.tex_res[d] ** 2 for d in range(bank.D))
    return 116 * live + 8 * (_quads(bank) - live) + 4 * texels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_fit.json"))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--iterations", type=int, default=400)
    ap.add_argument("--train-views", type=int, default=48)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("texture_fit_bench needs a GPU")
    from tools.simplify_bench import _fields
    from tools.texture_transfer_bench import DELTA, K, PAD, RATIO, RES, _orbit, _quality, _spread
    from volsurfs_amd import _lib, isosurface as iso
    from volsurfs_amd import texture_transfer as TT
    from volsurfs_amd.atlas import compute_atlas
    from volsurfs_amd.camera import get_camera_rays
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.simplify import simplify_mesh, simplify_shells
    from volsurfs_amd.texture_fit import TextureFit, fit_textures

    def save(result):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    result = {"device": torch.cuda.get_device_name(0), "grid": a.n, "reps": a.reps, "views": a.views, "size": a.size,
              "iterations": a.iterations, "train_views": a.train_views, "copy_tb_s": COPY_TBS}
    full, _ = iso.extract_level_sets(_fields()["lobed_noisy"], a.n, K, delta_surfs=DELTA)
    meshes = [compute_atlas(simplify_mesh(m, RATIO), RES, PAD) for m in full]
    del full
    src = VolSurfs(meshes, max_rays=4096)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        src.bank.tables.copy_((torch.rand(src.bank.tables.shape, generator=g) * 2 - 1).cuda())
    src.bank.refresh_half_params()
    src.bake()
    res = list(src.baked.tex_res)
    eval_cams, train_cams = _orbit(a.views, a.size), _train_cameras(a.train_views, a.size)
    targets = [src.render_baked_camera(c)["rgb"].float().contiguous() for c in train_cams]
    lod_meshes, _ = simplify_shells([TensorMesh(m.vertices, m.faces, None) for m in meshes], 0.25)
    result["faces"] = [int(m.faces.shape[0]) for m in lod_meshes]
    result["cases"] = {}

    for top in (1024, 512):
        tres = [max(top >> d, 8) for d in range(len(res))]
        lod = TT.transfer_scene(src, [compute_atlas(m, top, PAD) for m in lod_meshes], tres, samples=1)
        case = result["cases"][f"res{top}"] = {"textures_res": tres, "before": _quality(src, lod, eval_cams, a.size),
                                               "sweep": {}}
        print(f"res{top} before", json.dumps(case["before"]), flush=True)
        for lr in LRS:
            fitted, rep = fit_textures(lod, train_cams, targets=targets, iterations=a.iterations, lr=lr)
            q = _quality(src, fitted, eval_cams, a.size)
            case["sweep"][f"{lr:g}"] = {
                "psnr": q["psnr"], "ssim": q["ssim"],
                "psnr_gain_db": round(q["psnr"]["median"] - case["before"]["psnr"]["median"], 3),
                "train_loss_before": rep.loss_before, "train_loss_after": rep.loss_after,
                "loss_curve_every_10": [round(x, 6) for x in rep.losses[::10]],
                "texels_touched": {f"{s}/{d}": n for (s, d), n in rep.texels_touched.items()},
                "quads_updated": rep.quads_updated, "bytes_changed": rep.bytes_changed, "nonfinite": rep.nonfinite,
                "clamped": rep.clamped}
            save(result)
            print(f"res{top} lr {lr:g}: **PSNR gain {case['sweep'][f'{lr:g}']['psnr_gain_db']:+.3f} dB** "
                  f"({case['before']['psnr']['median']:.3f} -> {q['psnr']['median']:.3f}), SSIM "
                  f"{case['before']['ssim']['median']:.3f} -> {q['ssim']['median']:.3f}, training loss "
                  f"{rep.loss_before:.5f} -> {rep.loss_after:.5f}", flush=True)
            del fitted

        # ---- what an iteration costs
        fit = TextureFit(lod)
        rays = [get_camera_rays(c) for c in train_cams[:a.reps + 1]]

        def iteration(i):
            o, d, _ = get_camera_rays(train_cams[i % len(train_cams)])
            fit.accumulate(o, d, targets[i % len(train_cams)])
            return fit.step()
        for i in range(3):
            iteration(i)
        n_it = 40
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n_it):
            iteration(i)
        e1.record()
        torch.cuda.synchronize()
        _lib.kernel_events = {}
        for i in range(n_it):
            iteration(i)
        totals = _lib.kernel_totals()
        _lib.kernel_events = None
        groups, other = {}, {}
        for name, (ms, _) in totals.items():
            into, key = (groups, GROUPS[name]) if name in GROUPS else (other, name)
            into[key] = round(into.get(key, 0.0) + ms / n_it, 4)
        case["iteration"] = {"device_ms": round(e0.elapsed_time(e1) / n_it, 4), "entry_points_ms": groups,
                             "other_entry_points_ms": other}
        print(f"res{top} iteration", json.dumps(case["iteration"]), flush=True)

        # ---- the step kernel alone
        ms, live = [], []
        for i in range(a.reps + 1):
            o, d, _ = rays[i]
            fit.accumulate(o, d, targets[i])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            stats = fit.step()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            live.append(int(stats[0]))
        ms, live = ms[1:], live[1:]
        bank = fit.scene.baked
        total = _quads(bank)
        med, live_med = statistics.median(ms), int(statistics.median(live))
        moved = _step_bytes(bank, live_med)
        dense_ms = []
        for i in range(a.reps + 1):
            fit.grad_rows.fill_(1.0)
            fit._scale = 1.0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dense_stats = fit.step()
            e1.record()
            torch.cuda.synchronize()
            dense_ms.append(e0.elapsed_time(e1))
        dense_bytes = _step_bytes(bank, total)
        case["step"] = {
            "ms": _spread(ms), "quads": total, "live_quads": live_med, "idle_share": round(1 - live_med / total, 4),
            "bytes": moved, "tb_s": round(moved / med / 1e9, 3), "share_of_copy_rate": round(moved / med / 1e9 / COPY_TBS, 3),
            "dense_step_ms_measured": _spread(dense_ms[1:]), "dense_step_live_quads": int(dense_stats[0]),
            "dense_step_bytes": dense_bytes,
            "dense_step_tb_s_measured": round(dense_bytes / statistics.median(dense_ms[1:]) / 1e9, 3),
            "dense_step_ms_at_copy_rate": round(dense_bytes / (COPY_TBS * 1e9), 4)}
        save(result)
        print(f"res{top} step", json.dumps(case["step"]), flush=True)
        del fit, lod
    print("wrote", a.out)


if __name__ == "__main__":
    main()
