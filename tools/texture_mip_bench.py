"""Texture mips (volsurfs_amd.texture_mip, csrc/texture_mip.hip) on the scenes of DESIGN §40: the five lobed
shells of tools/texture_transfer_bench.py (16 k faces each, atlases at 1024, textures at 2048 / 1024 / 512 / 256, a
noise-like baked appearance) and their `make_lod` copies.  One process, one GPU; every figure is recorded as it comes
out, a loss included; no figure is a pass condition.

  chain      the L = 4 chain of the source (`mip_planes`, four launches) with and without a coverage mask, against a
             device copy that reads and writes the same number of bytes, alternated with it in the same run: ms (median
             and range of --reps after a warm-up) and the fraction of the copy's rate, for `mip_planes` whole (with the
             allocation of the level buffers) and for the four launches alone (`_lib.kernel_events`).  `build_mips`
             whole (export, owners, chain, density, the one read), wall clock.
  frame      an 800 x 800 `render_baked_camera` at three distances whose mean level (finest degree, hits only) is about
             0, 1.5 and 3: filter="bilinear" (the parent commit's code path), filter="mip", and bilinear at supersample 2;
             device ms per frame, the three alternated; the shade entry points alone (`_lib.kernel_events`).
  quality    PSNR / SSIM (evaluation.py) against the 8 x 8 supersampled bilinear frame at the same three distances, of
             bilinear 1 spp, mip 1 spp and bilinear 2 x 2, for the source and for every LOD scene; the mip frame with
             coverage="owners" and with coverage=None (the bleeding of the texels outside the charts).
  coverage   covered texels per level and degree of shell 0, and per level the texels that two or more charts share and
             the distinct chart pairs that meet in one: where the atlas's padding stops separating the charts.

    python tools/texture_mip_bench.py [--out profiles/texture_mip.json] [--n 512] [--size 800] [--reps 7]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = 4
TARGET_LEVELS = (0.0, 1.5, 3.0)
LOD_RATIOS = (0.25, 0.0625)


def _camera(radius, size):
    from volsurfs_amd.camera import Camera
    a = 0.7
    return Camera.look_at((radius * math.cos(a), 0.3 * radius, radius * math.sin(a)), focal=1.1 * size, height=size,
                          width=size)


def _image(out, size):
    return out["rgb"].float().reshape(1, size, size, 3).permute(0, 3, 1, 2).contiguous().clamp(0, 1)


def _chart_pairs(TT, mesh, chart_of_face, res, levels):
    """Per degree and level l: the texels of level l that hold readable texels (an owner within 1.5 texels) of two or
    more charts, and the distinct chart pairs that meet in such a texel -- charts closer than 2^l texels of level 0
    along an axis.  At level 0 a shared texel is one whose owner's neighbourhood is ambiguous by construction: none."""
    import torch
    out = {}
    nr_charts = int(chart_of_face.max()) + 1
    for d, R in enumerate(res):
        face, _, _ = TT.texel_owners(mesh, R, reach=1.5)
        chart = torch.where(face >= 0, chart_of_face.long()[face.clamp(min=0).long()], torch.full_like(face, -1).long())
        rows = {}
        for l in range(levels + 1):
            b, n = 1 << l, R >> l
            blocks = chart.reshape(n, b, n, b).permute(0, 2, 1, 3).reshape(n * n, b * b)
            key = torch.unique(torch.arange(n * n, device=chart.device)[:, None] * (nr_charts + 1) + blocks + 1)
            key = key[key % (nr_charts + 1) != 0]                                   # drop the unowned entries
            blk, ch = key // (nr_charts + 1), key % (nr_charts + 1) - 1
            counts = torch.bincount(blk, minlength=n * n)
            shared = counts >= 2
            pairs = set()
            if bool(shared.any()):
                sel = shared[blk]
                bs, cs = blk[sel].tolist(), ch[sel].tolist()
                per = {}
                for x, c in zip(bs, cs):
                    per.setdefault(x, []).append(c)
                for cl in per.values():
                    pairs.update((p, q) for i, p in enumerate(cl) for q in cl[i + 1:])
            rows[f"level{l}"] = {"texels": n * n, "shared_texels": int(shared.sum()), "chart_pairs": len(pairs)}
        out[f"degree{d}"] = {"resolution": R, "charts": nr_charts, **rows}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_mip.json"))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=800)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("texture_mip_bench needs a GPU")
    from tools.simplify_bench import _fields
    from tools.texture_transfer_bench import DELTA, K, PAD, RATIO, RES, _spread, _wall
    from volsurfs_amd import _lib, isosurface as iso
    from volsurfs_amd import texture_mip as TMIP
    from volsurfs_amd import texture_transfer as TT
    from volsurfs_amd.atlas import compute_atlas
    from volsurfs_amd.evaluation import psnr, ssim
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.simplify import simplify_mesh
    from volsurfs_amd.texture_export import _export_flat

    def save(result):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    def alternate(fns, reps):
        """Device ms per call of every fn, the fns taking turns inside each repetition, after one warm-up round."""
        for fn in fns.values():
            fn()
        ms = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return {k: _spread(v) for k, v in ms.items()}

    result = {"device": torch.cuda.get_device_name(0), "grid": a.n, "reps": a.reps, "size": a.size, "levels": LEVELS}
    full, _ = iso.extract_level_sets(_fields()["lobed_noisy"], a.n, K, delta_surfs=DELTA)
    atlased = [compute_atlas(simplify_mesh(m, RATIO), RES, PAD, return_charts=True) for m in full]
    meshes, charts = [m for m, _ in atlased], [c for _, c in atlased]
    del full, atlased
    src = VolSurfs(meshes, max_rays=4096)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        src.bank.tables.copy_((torch.rand(src.bank.tables.shape, generator=g) * 2 - 1).cuda())
    src.bank.refresh_half_params()
    src.bake()
    bank = src.baked
    res = [int(r) for r in bank.tex_res[:bank.D]]
    result["source"] = {"faces": [int(m.faces.shape[0]) for m in meshes], "textures_res": res}

    # ---- chain
    planes, _ = _export_flat(bank)
    cover = TMIP._owner_cover(src, res, bank.K, bank.D)
    total, ctotal = planes.numel(), cover.numel()
    moved = sum((total >> (2 * l)) + (total >> (2 * l + 2)) for l in range(LEVELS))          # read + written
    moved_c = moved + sum((ctotal >> (2 * l)) + (ctotal >> (2 * l + 2)) for l in range(LEVELS))
    a_buf, b_buf = (torch.empty(moved_c // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
    t = alternate({"chain": lambda: TMIP.mip_planes(planes, res, bank.K, bank.D, LEVELS),
                   "copy": lambda: b_buf[:moved // 2].copy_(a_buf[:moved // 2]),
                   "chain_masked": lambda: TMIP.mip_planes(planes, res, bank.K, bank.D, LEVELS, cover),
                   "copy_masked": lambda: b_buf.copy_(a_buf)}, a.reps)
    # the four launches alone (the alternated figure above includes the allocation of the level buffers)
    launches = {}
    for key, cv in (("chain", None), ("chain_masked", cover)):
        _lib.kernel_events = {}
        for _ in range(a.reps + 1):
            TMIP.mip_planes(planes, res, bank.K, bank.D, LEVELS, cv)
        torch.cuda.synchronize()
        ev = _lib.kernel_events["vsa_texmip_reduce"][LEVELS:]                    # (the first round is the warm-up)
        _lib.kernel_events = None
        per_call = [sum(e0.elapsed_time(e1) for e0, e1 in ev[i:i + LEVELS]) for i in range(0, len(ev), LEVELS)]
        launches[key] = _spread(per_call)
    _, build_ms = _wall(lambda: src.build_mips(levels=LEVELS))
    result["chain"] = {
        "plane_bytes_level0": total, "bytes_moved": moved, "bytes_moved_masked": moved_c, "ms": t,
        "gb_s": {k: round((moved_c if "masked" in k else moved) / t[k]["median"] / 1e6, 1) for k in t},
        "fraction_of_copy_rate": round(t["copy"]["median"] / t["chain"]["median"], 3),
        "fraction_of_copy_rate_masked": round(t["copy_masked"]["median"] / t["chain_masked"]["median"], 3),
        "launches_ms": launches,
        "launches_fraction_of_copy_rate": round(t["copy"]["median"] / launches["chain"]["median"], 3),
        "launches_fraction_of_copy_rate_masked": round(t["copy_masked"]["median"] / launches["chain_masked"]["median"], 3),
        "note": "ms.chain = mip_planes whole: four vsa_texmip_reduce launches and the allocation of the level buffers; "
                "launches_ms = the sum of the four launches' own events; the copy moves the same bytes (half read, half "
                "written) in one launch",
        "build_mips_wall_ms": round(build_ms, 1)}
    result["coverage_shell0"] = {f"level{l}": {f"degree{d}": [src.mips.covered[l][d], (res[d] >> l) ** 2]
                                               for d in range(bank.D)} for l in range(LEVELS + 1)}
    result["chart_pairs_shell0"] = _chart_pairs(TT, meshes[0], charts[0], res, LEVELS)
    save(result)
    print("chain", json.dumps(result["chain"]), flush=True)
    print("chart_pairs", json.dumps(result["chart_pairs_shell0"]), flush=True)

    # ---- the three distances
    def mean_level(scene, cam):
        lod = TMIP.hit_lod(scene, cam)[..., 0]
        return float(lod[~torch.isnan(lod)].mean())
    radii = [1.2 * 2 ** (k / 4) for k in range(0, 25)]
    levels_at = [mean_level(src, _camera(r, a.size)) for r in radii]
    picks = [min(range(len(radii)), key=lambda i: abs(levels_at[i] - tl)) for tl in TARGET_LEVELS]
    result["distances"] = [{"radius": round(radii[i], 3), "mean_level_degree0": round(levels_at[i], 3)} for i in picks]
    cams = [_camera(radii[i], a.size) for i in picks]

    # ---- frame time
    result["frame"] = []
    for cam, dist in zip(cams, result["distances"]):
        t = alternate({"bilinear": lambda: src.render_baked_camera(cam),
                       "mip": lambda: src.render_baked_camera(cam, filter="mip"),
                       "bilinear_2x2": lambda: src.render_baked_camera(cam, supersample=2),
                       "bilinear_raster": lambda: src.render_baked_camera(cam, hits="raster"),
                       "mip_raster": lambda: src.render_baked_camera(cam, hits="raster", filter="mip")}, a.reps)
        _lib.kernel_events = {}
        for _ in range(a.reps):
            src.render_baked_camera(cam)
            src.render_baked_camera(cam, filter="mip")
        shade = {k: round(v, 4) for k, v in _lib.kernel_ms().items() if "shade" in k}
        _lib.kernel_events = None
        result["frame"].append({**dist, "frame_ms": t, "shade_kernel_ms_median": shade})
        print("frame", json.dumps(result["frame"][-1]), flush=True)
    save(result)

    # ---- quality, source and LODs
    scenes = {"source": src}
    for ratio in LOD_RATIOS:
        scenes[f"lod_{ratio:g}"], _ = TT.make_lod(src, ratio)
    result["quality"] = {}
    for name, scene in scenes.items():
        rows = []
        owners = scene.build_mips(levels=LEVELS, coverage="owners")
        everything = scene.build_mips(levels=LEVELS, coverage=None)
        for cam, dist in zip(cams, result["distances"]):
            target = _image(scene.render_baked_camera(cam, supersample=8), a.size)
            row = dict(dist)
            scene.mips = owners
            frames = {"bilinear_1spp": scene.render_baked_camera(cam), "mip_1spp": scene.render_baked_camera(cam, filter="mip"),
                      "bilinear_2x2": scene.render_baked_camera(cam, supersample=2)}
            scene.mips = everything
            frames["mip_1spp_coverage_none"] = scene.render_baked_camera(cam, filter="mip")
            for k, f in frames.items():
                img = _image(f, a.size)
                row[k] = {"psnr": round(float(psnr(img, target)), 3), "ssim": round(float(ssim(img, target)), 4)}
            rows.append(row)
            print("quality", name, json.dumps(row), flush=True)
        result["quality"][name] = {"faces": [int(m.faces.shape[0]) for m in scene.tensor_meshes], "views": rows}
        save(result)
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
