"""Guarded shell simplification (volsurfs_amd.simplify.simplify_shells, csrc/simplify.hip: smp_guard) on the
stack the README's crossing figures come from: K = 5 level sets of the noisy lobed SDF of tools/simplify_bench.py on an
n^3 grid at the reference's delta_surfs = 0.0025, at ratio 0.025, in one process on one GPU.

Recorded: per shell faces_out / target / stalled / guard_rejected / rounds / collapses / self-crossings; the crossing
pairs of every consecutive pair of the inputs and of the outputs, `shells_nested`; whether a second call gives the same
bytes.  Beside it, in the same run, what the library did before: `simplify_mesh` per shell (its crossings), and that
followed by `untangle_shells` with its defaults (its crossings, self-crossings, convergence).  If the guarded stack
stalls above its targets or keeps crossings, that is what the file says: nothing here tunes the rule.

Timed --reps times after a warm-up, host clock around calls that end in a device synchronise, min / median / max in ms:
  simplify_shells       the whole call: guard trees, K guarded simplifications, the crossing counts of the report.
  guarded_only          the K vsa_simplify_guarded calls with their guard trees, without the report's counts.
  plain                 simplify_mesh per shell.
  plain_then_untangle   simplify_mesh per shell, then untangle_shells.
and the seven stage times per shell (device events, one stream synchronisation per stage, in a run of their own) next
to the six of the plain path.  No speed threshold is a pass condition.  Needs a GPU; writes one JSON file.

    python tools/simplify_shells_bench.py [--out profiles/simplify_shells.json] [--n 512] [--reps 3] [--ratio 0.025]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, DELTA = 5, 0.0025


def _spread(ms):
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def _guarded_stack(meshes, ratio, stage_ms=None):
    """`simplify_shells`' K guarded calls alone (no report): the outputs; stage_ms (a list) takes one dict per shell."""
    from volsurfs_amd import simplify as smp
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.shell_stack import guard_block
    inputs = RayTracer(meshes, builder="device")
    done, out = [None] * K, [None] * K
    for k, names in smp.stack_order(K, K // 2):
        guards = [(inputs, g) if which == "in" else (done[g], 0) for which, g in names]
        V, F, r = smp._check(meshes[k], ratio)
        ms = {} if stage_ms is not None else None
        v, f, _ = smp._simplify_guarded(V, F, smp.target_faces(F.shape[0], r), guard_block(guards, "bench"), ms)
        out[k] = smp._uvless(v, f)
        done[k] = RayTracer([out[k]], builder="device")
        if stage_ms is not None:
            stage_ms.append({"shell": k, **{s: round(t, 3) for s, t in ms.items()}})
    return out


def _plain_stages(meshes, ratio):
    from volsurfs_amd import simplify as smp
    rows = []
    for k, m in enumerate(meshes):
        V, F, r = smp._check(m, ratio)
        ms = {}
        smp._simplify(V, F, smp.target_faces(F.shape[0], r), ms)
        rows.append({"shell": k, **{s: round(t, 3) for s, t in ms.items()}})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_shells.json"))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.025)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("simplify_shells_bench needs a GPU")
    from tools.simplify_bench import _fields
    from volsurfs_amd import isosurface as iso, mesh_intersect as MI
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.shell_stack import self_crossing_count
    from volsurfs_amd.shell_untangle import untangle_shells
    from volsurfs_amd.simplify import simplify_mesh, simplify_shells

    result = {"device": torch.cuda.get_device_name(0), "grid": a.n, "reps": a.reps, "delta_surfs": DELTA,
              "ratio": a.ratio}
    meshes, _ = iso.extract_level_sets(_fields()["lobed_noisy"], a.n, K, delta_surfs=DELTA)
    result["faces_in"] = [int(m.faces.shape[0]) for m in meshes]

    def pairs(ms):
        return [e["pairs"] for e in MI.shell_crossings(ms)]

    def selfs(ms):
        t = RayTracer(ms, builder="device")
        return [int(self_crossing_count(t, k).item()) for k in range(K)]

    def note(what):
        print(f"[simplify_shells_bench] {what}", file=sys.stderr, flush=True)

    # ---- the guarded stack
    note(f"faces in {result['faces_in']}")
    out, reports = simplify_shells(meshes, a.ratio)
    note(f"guarded: {[tuple(r) for r in reports]} crossings {reports.crossings_in} -> {reports.crossings_out}")
    result["tree_depth_inputs"] = RayTracer(meshes, builder="device").max_depth
    result["shells"] = [dict(r._asdict(), guards=[list(g) for g in r.guards]) for r in reports]
    result["crossings_in"], result["crossings_out"] = reports.crossings_in, reports.crossings_out
    result["nested_out"] = reports.nested
    result["faces_out_over_target"] = [round(r.faces_out / max(r.target, 1), 4) for r in reports]
    again, _ = simplify_shells(meshes, a.ratio)
    result["same_bytes_on_a_second_call"] = all(
        torch.equal(x.faces, y.faces) and torch.equal(x.vertices.view(torch.int32), y.vertices.view(torch.int32))
        for x, y in zip(out, again))

    # ---- the parent's path: each shell on its own, then untangled
    plain, plain_stats = zip(*[simplify_mesh(m, a.ratio, return_stats=True) for m in meshes])
    plain = list(plain)
    result["plain"] = {"faces_out": [s["faces_out"] for s in plain_stats], "rounds": [s["rounds"] for s in plain_stats],
                       "stalled": [s["stalled"] for s in plain_stats], "crossings": pairs(plain),
                       "self_crossings": selfs(plain), "nested": MI.shells_nested(plain)}
    unt, ureports = untangle_shells(plain)
    result["plain_then_untangle"] = {"crossings": pairs(unt), "self_crossings": [r.self_crossings_after for r in ureports],
                                     "converged": [r.converged for r in ureports],
                                     "rounds": [r.rounds for r in ureports],
                                     "max_displacement_over_spacing": [round(r.max_displacement / DELTA, 4)
                                                                       for r in ureports],
                                     "nested": MI.shells_nested(unt)}

    note(f"plain {result['plain']['crossings']}, untangled {result['plain_then_untangle']['crossings']}")
    # ---- times: alternating
    cases = {"simplify_shells": lambda: simplify_shells(meshes, a.ratio),
             "guarded_only": lambda: _guarded_stack(meshes, a.ratio),
             "plain": lambda: [simplify_mesh(m, a.ratio) for m in meshes],
             "plain_then_untangle": lambda: untangle_shells([simplify_mesh(m, a.ratio) for m in meshes])}
    times = {name: [] for name in cases}
    for _ in range(a.reps):
        for name, fn in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
            note(f"{name} {times[name][-1]:.1f} ms")
    result["ms"] = {name: _spread(ms) for name, ms in times.items()}
    result["guarded_over_plain"] = round(result["ms"]["guarded_only"]["median"] / result["ms"]["plain"]["median"], 2)

    # ---- stage times: a run of their own
    stage_ms = []
    _guarded_stack(meshes, a.ratio, stage_ms)
    result["guarded_stage_ms"] = sorted(stage_ms, key=lambda r: r["shell"])
    result["plain_stage_ms"] = _plain_stages(meshes, a.ratio)
    result["guard_stage_share"] = round(sum(r["guard"] for r in stage_ms) /
                                        sum(sum(v for s, v in r.items() if s != "shell") for r in stage_ms), 4)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
