"""Shell untangling (volsurfs_amd.shell_untangle, csrc/shell_untangle.hip) on the stack the README's
crossing figures come from: K = 5 level sets of the noisy lobed SDF of tools/simplify_bench.py on an n^3 grid at the
reference's delta_surfs = 0.0025, each simplified to 0.025 of its faces (the shells of tools/mesh_intersect_bench.py),
in one process on one GPU.

Recorded: per shell the rounds, the highest level, the moved vertices, the largest displacement as a fraction of the
shell spacing and the round log (moved, stuck, max |t|, crossing pairs); crossings and self-crossings before and after;
`converged`; `shells_nested` after.  If the stack does not converge or comes out with self-crossings, that is what the
file says: the rule is fixed by the restatement (tests/shell_untangle_restated.py), nothing here tunes it.

Timed --reps times after a warm-up, host clock around calls that end in a device synchronise, min / median / max in ms:
  untangle_shells   the whole call on a tracer built (untimed) from the input meshes for every repetition.
  baseline          the same rule with what the library had before this stage: `RayTracer.signed_distance`, torch ops for
                    the residual, the test and the move, the crossing count pass as `crossing_stats` runs it, torch for
                    the levels; the same refits.  Whether its vertices equal the stage's bit for bit is recorded, with
                    the largest difference.
  project kernel    device events around vsa_shell_untangle_project alone (`_lib.kernel_events`), in a run of its own:
                    the total over all rounds of all shells, the calls, and the median per call.
No speed threshold is a pass condition.  Needs a GPU; writes one JSON file.

    python tools/shell_untangle_bench.py [--out profiles/shell_untangle.json] [--n 512] [--reps 5] [--margin 2.5e-4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, DELTA, RATIO = 5, 0.0025, 0.025


def _spread(ms):
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def _baseline_pair(tracer, mesh_id, against, side, margin, max_rounds, max_level):
    """One pair by the rule, with the library's older entry points and torch.  Returns (vertices, rounds, converged)."""
    import torch
    from volsurfs_amd import mesh_intersect as MI
    from volsurfs_amd.mesh import TensorMesh
    dev = tracer.device
    mesh = tracer._meshes[mesh_id]
    v = mesh.vertices.detach().to(dev, torch.float32).clone()
    f = mesh.faces.detach().to(dev, torch.int32).contiguous()
    level = torch.zeros(v.shape[0], dtype=torch.int64, device=dev)
    tree = MI.tree_of((tracer, against), "baseline")
    order = MI.leaf_order(tracer, mesh_id)
    s, m0 = torch.tensor(float(side), device=dev), torch.tensor(margin, dtype=torch.float32, device=dev)
    rounds, converged = 0, False
    for _ in range(max_rounds):
        q = tracer.signed_distance(v, against)
        dist, slot, bary = q["dist"], q["slot"].long().clamp_min(0), q["bary"]
        rec = tracer.tris[slot]
        a = v - rec[:, 0:3]
        r = (a - bary[:, 0:1] * rec[:, 4:7]) - bary[:, 1:2] * rec[:, 8:11]
        m = m0 * torch.bitwise_left_shift(torch.ones_like(level), level.clamp_max(max_level)).float()
        violated = (s * dist < m) & (q["slot"] >= 0)
        t = s * (1.25 * m) - dist
        ad = dist.abs()
        if bool(((ad == 0) & violated).any()):
            raise RuntimeError("baseline: a vertex on the fixed surface (the region code is not returned)")
        g = r / ad[:, None]
        g = torch.where((dist < 0)[:, None], -g, g)
        moved = violated & torch.isfinite(g).all(1)
        v = torch.where(moved[:, None], v + t[:, None] * g, v).contiguous()
        _, count_q, _, _, total = MI.cross_passes(tree, (v, f, order), False, False, False)
        crossing = f[count_q > 0].flatten().long().unique()
        level[crossing] += 1
        rounds += 1
        nr_moved, pairs = torch.stack([moved.sum(), total[0]]).cpu().tolist()          # the round's blocking read
        if nr_moved == 0 and pairs == 0:
            converged = True
            break
    meshes = list(tracer._meshes)
    meshes[mesh_id] = TensorMesh(v, mesh.faces, mesh.faces_uvs, device=dev)
    tracer.refit(meshes)
    return v, rounds, converged


def _baseline(tracer, margin, max_rounds, max_level):
    anchor = K // 2
    out = {}
    for k, against, side in ([(k, k - 1, 1) for k in range(anchor + 1, K)] +
                             [(k, k + 1, -1) for k in range(anchor - 1, -1, -1)]):
        out[k] = _baseline_pair(tracer, k, against, side, margin, max_rounds, max_level)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shell_untangle.json"))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--margin", type=float, default=0.1 * DELTA)
    ap.add_argument("--max-rounds", type=int, default=16)
    ap.add_argument("--max-level", type=int, default=6)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("shell_untangle_bench needs a GPU")
    from tools.simplify_bench import _fields
    from volsurfs_amd import _lib, isosurface as iso, mesh_intersect as MI
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.shell_stack import self_crossing_count
    from volsurfs_amd.shell_untangle import untangle_shells
    from volsurfs_amd.simplify import simplify_mesh

    kw = dict(margin=a.margin, max_rounds=a.max_rounds, max_level=a.max_level)
    result = {"device": torch.cuda.get_device_name(0), "grid": a.n, "reps": a.reps, "delta_surfs": DELTA,
              "simplify_ratio": RATIO, **kw}
    meshes, _ = iso.extract_level_sets(_fields()["lobed_noisy"], a.n, K, delta_surfs=DELTA)
    meshes = [simplify_mesh(m, RATIO) for m in meshes]
    result["faces"] = [int(m.faces.shape[0]) for m in meshes]
    result["vertices"] = [int(m.vertices.shape[0]) for m in meshes]

    def fresh():
        return RayTracer(meshes, builder="device")

    tracer = fresh()
    result["tree_depth"] = tracer.max_depth
    result["before"] = {"crossings": [e["pairs"] for e in MI.shell_crossings(tracer)],
                        "self_crossings": [int(self_crossing_count(tracer, k).item()) for k in range(K)],
                        "nested": MI.shells_nested(tracer)}
    log = {}
    out, reports = untangle_shells(tracer, log=log, **kw)
    result["shells"] = [{"shell": r.shell, "side": r.side, "against": r.against, "rounds": r.rounds,
                         "max_level": r.max_level, "moved_vertices": r.moved_vertices, "stuck": r.stuck,
                         "max_displacement": r.max_displacement,
                         "max_displacement_over_spacing": round(r.max_displacement / DELTA, 4),
                         "crossings_before": r.crossings_before, "crossings_after": r.crossings_after,
                         "self_crossings_after": r.self_crossings_after, "converged": r.converged,
                         "round_log": [list(x) for x in log.get(r.shell, [])]} for r in reports]
    result["converged"] = all(r.converged for r in reports)
    result["after"] = {"crossings": [e["pairs"] for e in MI.shell_crossings(tracer)],
                       "self_crossings": [r.self_crossings_after for r in reports],
                       "nested": MI.shells_nested(tracer)}
    for m0, m1 in zip(meshes, out):
        assert torch.equal(m0.faces, m1.faces) and m0.vertices.shape == m1.vertices.shape

    # ---- the same bytes again, and the baseline's
    again, _ = untangle_shells(fresh(), **kw)
    result["same_bytes_on_a_second_call"] = all(
        torch.equal(x.vertices.view(torch.int32), y.vertices.view(torch.int32)) for x, y in zip(out, again))
    base = _baseline(fresh(), **kw)
    result["baseline_equal_vertices"] = all(
        torch.equal(base[k][0].view(torch.int32), out[k].vertices.view(torch.int32)) for k in base)
    result["baseline_rounds"] = {str(k): base[k][1] for k in sorted(base)}
    result["baseline_max_abs_difference"] = max(float((base[k][0] - out[k].vertices).abs().max()) for k in base)

    # ---- times: alternating, each repetition on a tracer of its own
    stage_ms, base_ms = [], []
    for _ in range(a.reps):
        for fn, ms in ((lambda t: untangle_shells(t, **kw), stage_ms), (lambda t: _baseline(t, **kw), base_ms)):
            t = fresh()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(t)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
    result["untangle_shells_ms"] = _spread(stage_ms)
    result["baseline_ms"] = _spread(base_ms)
    result["baseline_over_stage"] = round(result["baseline_ms"]["median"] / result["untangle_shells_ms"]["median"], 2)

    # ---- the entry points alone: device events, a run of its own
    t = fresh()
    torch.cuda.synchronize()
    _lib.kernel_events = {}
    untangle_shells(t, **kw)
    totals, medians = _lib.kernel_totals(), _lib.kernel_ms()
    _lib.kernel_events = None
    result["entry_points_ms"] = {name: {"total": round(total, 3), "calls": calls, "median_per_call": round(medians[name], 4)}
                                 for name, (total, calls) in sorted(totals.items())
                                 if name.startswith(("vsa_shell_untangle", "vsa_mesh_cross_count"))}

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
