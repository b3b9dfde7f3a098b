"""Mesh smoothing (volsurfs_amd.mesh_smooth, csrc/mesh_smooth.hip) on the shells the atlas and untangle
figures come from: K = 5 level sets of the noisy lobed SDF of tools/simplify_bench.py on an n^3 grid at the reference's
delta_surfs = 0.0025, in one process on one GPU.  Four measurements, each recorded as it comes out, including where
the stage loses; nothing here tunes the rule (tests/mesh_smooth_restated.py fixes it).

  one_shell   the middle shell, 10 unguarded iterations.  Device events around the 20 vsa_mesh_smooth_step launches
              alone (min / median / max over --reps after a warm-up), and around the whole `_smooth` (prepare, steps,
              statistics read).  Bytes per half-step are counted from the shapes: `needed` = every array once (P read
              and written, ring ranges and flags, the ring's faces, the faces) = 36 V + 24 F; `requested` = what the
              lanes ask for (a face row and two neighbour positions per corner slot) = 36 V + 120 F.  Both over the
              median step time, against the HBM rate of a float4 copy on this GPU (6.29 TB/s).
  stack       `smooth_shells` of the five shells, guarded: wall ms, reverted vertices, guard rounds, crossings in and
              out; then the entry points alone under device events (`_lib.kernel_events`, a run of its own) and the
              share of their total that is vsa_mesh_smooth_guard.
  baselines   the same rule on the middle shell as torch ops on the same GPU (`index_add_` over the corner list: its
              sum order is the scheduler's) and as the numpy restatement on the host (half-steps only); ms, and whether
              the vertices equal the stage's bit for bit, with the largest difference.
  atlas       the reason for the stage: `simplify_mesh` at 0.025 then `compute_atlas` at 1024 / 4 of the five shells,
              with and without `smooth_shells` in front: charts, split rounds, utilization, pack ms, and
              `simplification_error` of both against the unsmoothed extraction.
No speed threshold is a pass condition.  Needs a GPU; writes one JSON file.

    python tools/mesh_smooth_bench.py [--out profiles/mesh_smooth.json] [--n 512] [--reps 5] [--skip-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, DELTA, RATIO, RES, PAD = 5, 0.0025, 0.025, 1024, 4
ITERATIONS, LAM, MU = 10, 0.5, -0.53
HBM_COPY_TBS = 6.29                     # MI355X, float4 copy (8.0 TB/s by the data sheet)


def _spread(ms):
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def _events(fn, reps):
    """Device ms of fn() per repetition, after one warm-up call."""
    import torch
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _steps_alone(v, f):
    """A closure that issues the 2 x ITERATIONS half-step launches on buffers of its own, and its last output."""
    import torch
    from volsurfs_amd import _lib, mesh_smooth as MS
    V, F = v.shape[0], f.shape[0]
    nbytes = MS.workspace_bytes(V, F)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=v.device)
    state = torch.zeros(1, dtype=torch.int64, device=v.device)
    st = _lib.stream_ptr()
    _lib.call("vsa_mesh_smooth_prepare", f, V, F, ws, nbytes, st)
    bufs = [torch.empty_like(v) for _ in range(3)]

    def run():
        cur, q, r = v, bufs[1], bufs[2]                            # (v is only ever read)
        for _ in range(ITERATIONS):
            _lib.call("vsa_mesh_smooth_step", cur, q, f, V, F, 0, LAM, 1, ws, nbytes, state, st)
            _lib.call("vsa_mesh_smooth_step", q, r, f, V, F, 1, MU, 1, ws, nbytes, state, st)
            cur, r = r, (bufs[0] if cur is v else cur)
        return cur
    return run, bufs


def _torch_rule(v, f):
    """The rule as torch ops: (prepare(), smooth(prepared)).  The ring sum is one index_add_ of P[a] + P[b] over the
    corner list: float atomics, in the scheduler's order."""
    import torch
    V = v.shape[0]

    def prepare():
        fl = f.long()
        corner, a, b = fl.reshape(-1), fl[:, [1, 2, 0]].reshape(-1), fl[:, [2, 0, 1]].reshape(-1)
        slots = torch.bincount(corner, minlength=V)
        keys = torch.minimum(corner, a) << 32 | torch.maximum(corner, a)
        uniq, count = torch.unique(keys, return_counts=True)
        once = uniq[count == 1]
        boundary = torch.zeros(V, dtype=torch.bool, device=v.device)
        boundary[once >> 32] = True
        boundary[once & 0xFFFFFFFF] = True
        return corner, a, b, (slots > 0) & ~boundary, (2 * slots).float()[:, None]

    def smooth(prepared):
        corner, a, b, free, n = prepared
        P = v
        for _ in range(ITERATIONS):
            for w in (LAM, MU):
                acc = torch.zeros_like(P).index_add_(0, corner, P[a] + P[b])
                new = P + w * (acc / n - P)
                P = torch.where((free & torch.isfinite(new).all(1))[:, None], new, P)
        return P
    return prepare, smooth


def _host_rule(v, f):
    import mesh_smooth_restated as M
    topo = M.topology(f, len(v))
    cur = v
    for _ in range(ITERATIONS):
        cur, _ = M.half_step(cur, topo, LAM)
        cur, _ = M.half_step(cur, topo, MU)
    return cur


def _compare(ref, other):
    import torch
    return {"equal_bits": bool(torch.equal(ref.view(torch.int32), other.view(torch.int32))),
            "max_abs_difference": float((ref.double() - other.double()).abs().max())}


def _atlas_case(originals, shells):
    """simplify at RATIO, atlas at RES / PAD: the figures of tools/atlas_bench.py, and the error against `originals`."""
    from volsurfs_amd import atlas
    from volsurfs_amd.mesh_distance import simplification_error
    from volsurfs_amd.simplify import simplify_mesh
    simp = [simplify_mesh(m, RATIO) for m in shells]
    for m in simp:                                                 # warm-up
        atlas.compute_atlas(m, RES, PAD)
    stats, pack = [], []
    for m in simp:
        ms = {}
        stats.append(atlas.compute_atlas(m, RES, PAD, return_stats=True)[1])
        atlas.compute_atlas(m, RES, PAD, stage_ms=ms)
        pack.append(ms["pack"])
    err = [simplification_error(o, s) for o, s in zip(originals, simp)]
    return {"faces": [int(m.faces.shape[0]) for m in simp], "charts": [s["charts"] for s in stats],
            "charts_sum": sum(s["charts"] for s in stats), "split_rounds": [s["split_rounds"] for s in stats],
            "utilization": [round(s["utilization"], 4) for s in stats],
            "utilization_mean": round(sum(s["utilization"] for s in stats) / len(stats), 4),
            "pack_ms": [round(x, 3) for x in pack], "pack_ms_sum": round(sum(pack), 3),
            "chamfer_rel": [e["chamfer_rel"] for e in err], "hausdorff_rel": [e["hausdorff_rel"] for e in err]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth.json"))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true", help="leave the numpy restatement out")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("mesh_smooth_bench needs a GPU")
    from tools.simplify_bench import _fields
    from volsurfs_amd import _lib, isosurface as iso, mesh_smooth as MS

    def save(result):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    result = {"device": torch.cuda.get_device_name(0), "grid": a.n, "reps": a.reps, "delta_surfs": DELTA,
              "iterations": ITERATIONS, "lam": LAM, "mu": MU}
    meshes, _ = iso.extract_level_sets(_fields()["lobed_noisy"], a.n, K, delta_surfs=DELTA)
    result["vertices"] = [int(m.vertices.shape[0]) for m in meshes]
    result["faces"] = [int(m.faces.shape[0]) for m in meshes]

    # ---- one shell, unguarded
    mid = meshes[K // 2]
    v, f = MS._check_mesh(mid, "bench")
    V, F = v.shape[0], f.shape[0]
    run, _ = _steps_alone(v, f)
    steps_ms = _events(run, a.reps)
    whole_ms = _events(lambda: MS._smooth(v, f, ITERATIONS, LAM, MU, True, None), a.reps)
    out, st = MS._smooth(v, f, ITERATIONS, LAM, MU, True, None)
    per_step = statistics.median(steps_ms) / (2 * ITERATIONS)
    needed, requested = 36 * V + 24 * F, 36 * V + 120 * F
    result["one_shell"] = {
        "vertices": V, "faces": F, "report": st, "steps_ms": _spread(steps_ms), "smooth_ms": _spread(whole_ms),
        "ms_per_half_step": round(per_step, 4), "bytes_needed_per_half_step": needed,
        "bytes_requested_per_half_step": requested,
        "needed_TB_per_s": round(needed / per_step / 1e9, 3), "requested_TB_per_s": round(requested / per_step / 1e9, 3),
        "hbm_copy_TB_per_s": HBM_COPY_TBS, "needed_over_hbm_copy": round(needed / per_step / 1e9 / HBM_COPY_TBS, 3),
        "steps_equal_smooth": bool(torch.equal(run().view(torch.int32), out.view(torch.int32)))}
    save(result)
    print("one_shell", json.dumps(result["one_shell"]), flush=True)

    # ---- the same rule as torch ops and on the host
    prepare, smooth = _torch_rule(v, f)
    prepared = prepare()
    base = {"torch_prepare_ms": _spread(_events(prepare, a.reps)),
            "torch_steps_ms": _spread(_events(lambda: smooth(prepared), a.reps)),
            "torch_vs_stage": _compare(out, smooth(prepared))}
    base["torch_steps_over_stage_steps"] = round(base["torch_steps_ms"]["median"] / statistics.median(steps_ms), 2)
    if not a.skip_host:
        hv, hf = v.cpu().numpy(), f.cpu().numpy()
        t0 = time.perf_counter()
        host = _host_rule(hv, hf)
        base["host_numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        base["host_vs_stage"] = _compare(out, torch.from_numpy(host).to(out.device))
    result["baselines"] = base
    save(result)
    print("baselines", json.dumps(base), flush=True)
    del prepared

    # ---- the stack, guarded
    MS.smooth_shells(meshes[:2], iterations=1)                     # warm-up of the guard's kernels and the builders
    walls = []
    for _ in range(max(1, a.reps // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        smoothed, reports = MS.smooth_shells(meshes)
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    _lib.kernel_events = {}
    again, _ = MS.smooth_shells(meshes)
    totals = _lib.kernel_totals()
    _lib.kernel_events = None
    own = {n: t for n, t in totals.items() if n.startswith("vsa_mesh_smooth")}
    total = sum(t for t, _ in own.values())
    result["stack"] = {
        "smooth_shells_ms": _spread(walls), "reports": [r._asdict() for r in reports],
        "crossings_in": reports.crossings_in, "crossings_out": reports.crossings_out, "nested": reports.nested,
        "same_bytes_on_a_second_call": all(torch.equal(x.vertices.view(torch.int32), y.vertices.view(torch.int32))
                                           for x, y in zip(smoothed, again)),
        "entry_points_ms": {n: {"total": round(t, 3), "calls": c} for n, (t, c) in sorted(own.items())},
        "guard_share_of_entry_points": round(own["vsa_mesh_smooth_guard"][0] / total, 4)}
    save(result)
    print("stack", json.dumps(result["stack"]), flush=True)

    # ---- the reason: atlases with and without the stage in front
    result["atlas"] = {"simplify_ratio": RATIO, "resolution": RES, "padding": PAD,
                       "plain": _atlas_case(meshes, meshes), "smoothed": _atlas_case(meshes, smoothed)}
    result["atlas"]["charts_smoothed_over_plain"] = round(
        result["atlas"]["smoothed"]["charts_sum"] / result["atlas"]["plain"]["charts_sum"], 4)
    save(result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
