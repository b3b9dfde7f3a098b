"""Texture bake of field appearance models (volsurfs_amd/texture_bake.py, csrc/texture_bake.hip) on the
shells §15 / §16 measure: K = 5 level sets of the noisy lobed SDF on a 1000^3 grid (delta_surfs = 0.0025), simplified to
0.025 and atlased at 1024 / padding 4, each with a ColorSH rgb model (27 coefficients) and a ColorSH alpha model (9) on
the permutohedral encoder and the fused MLP (128, 128, 64), baked at R = 2048, S = 12 and dilated by 5 iterations.

Per stage the device ms from events, summed over the 5 shells (two bakes per shell: alpha, rgb), median (min - max) of
--reps runs after a warm-up: sample pass (vsa_tb_samples + vsa_tb_emit), model evaluation, resolve, dilation.  One JSON
line.  `--profile RATIO` bakes shell 0 simplified to RATIO once after a warm-up and nothing else: the run that
`rocprofv3 --kernel-trace --stats` wraps (two ratios give two face counts: the tb_* launch counts must not differ).

    python tools/texture_bake_bench.py [--reps 10] [--res 2048] [--samples 12] [--n 1000]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, DELTA, ATLAS_RES, PAD = 5, 0.0025, 1024, 4


def _shells(n, ratio, only=None):
    from tools.simplify_bench import _fields
    from volsurfs_amd import atlas, isosurface as iso
    from volsurfs_amd.simplify import simplify_mesh
    meshes, _ = iso.extract_level_sets(_fields()["lobed_noisy"], n, K, delta_surfs=DELTA)
    if only is not None:
        meshes = [meshes[only]]
    return [atlas.compute_atlas(simplify_mesh(m, ratio), ATLAS_RES, PAD) for m in meshes]


def _models():
    import torch
    from volsurfs_amd.models import ColorSH
    torch.manual_seed(7)
    kw = dict(in_channels=3, mlp_layers_dims=[128, 128, 64], pos_encoder_type="permutohash", sh_deg=2, bb_sides=2.0)
    return ColorSH(out_channels=1, **kw), ColorSH(out_channels=3, **kw)


def _bake_shell(mesh, models, R, S, ms):
    import torch
    from volsurfs_amd.texture_bake import bake_field_texture, dilate_texture
    parts = []
    for model in models:
        st = {}
        parts.append(bake_field_texture(lambda p, n: model(p, samples_dirs=None, normals=n), mesh, R, S, stage_ms=st))
        for k in ("samples", "model", "resolve"):
            ms[k] += st[k]
        ms["rows"] += st["rows"]
        ms["chunks"] += st["chunks"]
    tex = torch.cat(parts[::-1], 2)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = dilate_texture(tex, 5)
    b.record()
    torch.cuda.synchronize()
    ms["dilation"] += a.elapsed_time(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--profile", type=float, default=0.0)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "texture_bake_bench needs a GPU"
    models = _models()
    zero = lambda: {"samples": 0.0, "model": 0.0, "resolve": 0.0, "dilation": 0.0, "rows": 0, "chunks": 0}
    if a.profile:
        mesh = _shells(a.n, a.profile, only=0)[0]
        _bake_shell(mesh, models, 256, a.samples, zero())          # warm-up: code objects, allocator
        ms = zero()
        _bake_shell(mesh, models, a.res, a.samples, ms)
        print(json.dumps({"profile_ratio": a.profile, "faces": int(mesh.faces.shape[0]),
                          **{k: round(v, 3) for k, v in ms.items()}}), flush=True)
        return
    shells = _shells(a.n, 0.025)
    runs = []
    for rep in range(a.reps + 1):
        ms = zero()
        covered = 0
        for mesh in shells:
            tex = _bake_shell(mesh, models, a.res, a.samples, ms)
            covered += int((tex != 0).all(2).sum()) if rep == 0 else 0
            del tex
        if rep:
            runs.append(ms)
        else:
            covered0 = covered
    med = lambda k: [round(f(r[k] for r in runs), 2) for f in (statistics.median, min, max)]
    print(json.dumps({"n": a.n, "K": K, "faces": sum(int(m.faces.shape[0]) for m in shells), "res": a.res,
                      "samples": a.samples, "reps": a.reps, "rows": runs[0]["rows"], "chunks": runs[0]["chunks"],
                      "texels_full_after_dilation": covered0,
                      "ms_median_min_max": {k: med(k) for k in ("samples", "model", "resolve", "dilation")}}),
          flush=True)


if __name__ == "__main__":
    main()
