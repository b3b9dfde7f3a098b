"""Texture transfer (volsurfs_amd.texture_transfer, csrc/texture_transfer.hip) on the shells the other mesh
benches use: K = 5 level sets of the noisy lobed SDF of tools/simplify_bench.py on an n^3 grid, simplified at 0.025 and
atlased at 1024 / 4, with a baked bank at the default resolutions (an untrained VolSurfs with random hash tables: the
appearance is noise-like, which is the hard case for a resampler).  One process, one GPU; every figure is recorded as it
comes out, including where the stage loses; no figure is a pass condition.

  reatlas     (a) the same meshes re-atlased at 512: device ms per entry point (owners, transfer, export of the source
              planes, import into the new bank: `_lib.kernel_events`, totals per call over --reps), the whole
              `transfer_planes` under device events, and the composition available without the stage --
              `rasterize_atlas` + `RayTracer.closest` + torch gathers and lerps for the covered texels -- under device
              events on the same GPU, with the share of owned texels it leaves unwritten and the share of its bytes that
              equal the stage's.
  lod         (b) `make_lod` at ratio 0.25 with textures at 1024 and at 512 (halving per degree), samples 1 and 2: wall ms
              of simplify, atlas and transfer + import, the faces, the reports' distances.
  quality     PSNR / SSIM (`evaluation.psnr` / `ssim`) of `render_baked_camera` of (a) and of every LOD against the
              source's over a fixed orbit of --views views at --size^2, with the face counts and the ms per frame.

    python tools/texture_transfer_bench.py [--out profiles/texture_transfer.json] [--n 512] [--reps 5] [--views 8]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, DELTA, RATIO, RES, PAD = 5, 0.0025, 0.025, 1024, 4


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


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def _lut(lo, span, dev):
    import torch
    q = torch.arange(256, dtype=torch.float32, device=dev)
    o = (q / 255.0).half().float()
    return (lo + (span * o).half().float()).half().float()


def _composition(src, src_planes, dst_meshes, res):
    """What the parent commit offers: per (shell, degree) `rasterize_atlas` for the covered texels, their points by
    torch, `RayTracer.closest`, torch gathers and lerps of the source planes, the nearest byte by bucketize.  Texels the
    rasterizer does not cover stay zero (no reach)."""
    import torch
    from volsurfs_amd.atlas import rasterize_atlas
    bank, tracer = src.baked, src.raytracer
    out = {}
    for s, m in enumerate(dst_meshes):
        V, F, UV = m.vertices, m.faces.long(), m.faces_uvs
        for d, R in enumerate(res):
            fid, _ = rasterize_atlas(m, R)
            r, c = torch.nonzero(fid >= 0, as_tuple=True)
            f = fid[r, c].long()
            t = UV[f] * R
            q = torch.stack([c + 0.5, r + 0.5], 1).float()
            e1, e2, a = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], q - t[:, 0]
            det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            u = (a[:, 0] * e2[:, 1] - a[:, 1] * e2[:, 0]) / det
            v = (e1[:, 0] * a[:, 1] - e1[:, 1] * a[:, 0]) / det
            v0, v1, v2 = V[F[f, 0]], V[F[f, 1]], V[F[f, 2]]
            p = (v0 + u[:, None] * (v1 - v0) + v[:, None] * (v2 - v0)).contiguous()
            hit = tracer.closest(p, s)
            fuv = src.face_uvs[hit["slot"].long()]
            bu, bv = hit["bary"][:, 0], hit["bary"][:, 1]
            b0 = 1.0 - bu - bv
            su = b0 * fuv[:, 0] + bu * fuv[:, 2] + bv * fuv[:, 4]
            sv = b0 * fuv[:, 1] + bu * fuv[:, 3] + bv * fuv[:, 5]
            Rs = bank.tex_res[d]
            ap, bp = Rs - sv * Rs, su * Rs
            flx, fly = torch.floor(ap - 0.5), torch.floor(bp - 0.5)
            fx, fy = ap - (flx + 0.5), bp - (fly + 0.5)
            i0, j0 = flx.long(), fly.long()
            plane = src_planes[(s, d)]
            lut = _lut(float(bank.plan.sh_lo[d]), float(bank.plan.sh_span[d]), V.device)
            acc = torch.zeros(plane.shape[0], f.shape[0], 4, device=V.device)
            for ky in (0, 1):
                for kx in (0, 1):
                    ix, iy = (i0 + kx).clamp(0, Rs - 1), (j0 + ky).clamp(0, Rs - 1)
                    w = (fx if kx else 1.0 - fx) * (fy if ky else 1.0 - fy)
                    acc = acc + lut[plane[:, Rs - 1 - ix, iy, :].long()] * w[None, :, None]
            coef = acc.half().float()
            q8 = torch.bucketize(coef, ((lut[1:] + lut[:-1]) * 0.5).contiguous()).to(torch.uint8)
            img = torch.zeros(plane.shape[0], R, R, 4, dtype=torch.uint8, device=V.device)
            img[:, r, c, :] = q8
            out[(s, d)] = img
    return out


def _orbit(views, size):
    from volsurfs_amd.camera import Camera
    cams = []
    for i in range(views):
        a = 2.0 * math.pi * i / views
        cams.append(Camera.look_at((1.6 * math.cos(a), 0.5 * math.sin(2 * a), 1.6 * math.sin(a)), focal=1.1 * size,
                                   height=size, width=size))
    return cams


def _quality(src, scene, cams, size):
    import torch
    from volsurfs_amd.evaluation import psnr, ssim
    ps, ss, ms = [], [], []
    for cam in cams:
        ref = src.render_baked_camera(cam)["rgb"].reshape(1, size, size, 3).permute(0, 3, 1, 2).contiguous()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        img = scene.render_baked_camera(cam)["rgb"]
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
        img = img.reshape(1, size, size, 3).permute(0, 3, 1, 2).contiguous()
        ps.append(float(psnr(img.clamp(0, 1), ref.clamp(0, 1))))
        ss.append(float(ssim(img.clamp(0, 1), ref.clamp(0, 1))))
    return {"faces": [int(m.faces.shape[0]) for m in scene.tensor_meshes], "psnr": _spread(ps), "ssim": _spread(ss),
            "frame_ms": _spread(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_transfer.json"))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=800)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("texture_transfer_bench needs a GPU")
    from tools.simplify_bench import _fields
    from volsurfs_amd import _lib, isosurface as iso
    from volsurfs_amd import texture_transfer as TT
    from volsurfs_amd.atlas import compute_atlas
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.simplify import simplify_mesh
    from volsurfs_amd.texture_export import export_planes

    def save(result):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")

    result = {"device": torch.cuda.get_device_name(0), "grid": a.n, "reps": a.reps, "views": a.views, "size": a.size}
    full, _ = iso.extract_level_sets(_fields()["lobed_noisy"], a.n, K, delta_surfs=DELTA)
    simple = [simplify_mesh(m, RATIO) for m in full]
    del full
    meshes = [compute_atlas(m, RES, PAD) for m in simple]
    src = VolSurfs(meshes, max_rays=4096)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        src.bank.tables.copy_((torch.rand(src.bank.tables.shape, generator=g) * 2 - 1).cuda())
    src.bank.refresh_half_params()
    src.bake()
    res = list(src.baked.tex_res)
    result["source"] = {"faces": [int(m.faces.shape[0]) for m in meshes], "textures_res": res,
                        "appearance": "untrained VolSurfs, hash tables U(-1, 1)"}
    cams = _orbit(a.views, a.size)

    # ---- (a) the same meshes, another atlas
    other = [compute_atlas(TensorMesh(m.vertices, m.faces, None), 512, PAD) for m in meshes]
    whole = _events(lambda: TT.transfer_planes(src, other), a.reps)
    _lib.kernel_events = {}
    for _ in range(a.reps):
        scene = TT.transfer_scene(src, other)
    totals = _lib.kernel_totals()
    _lib.kernel_events = None
    stages = {name: round(ms / a.reps, 3) for name, (ms, _) in totals.items()
              if name.startswith("vsa_textransfer") or name in ("vsa_nt_export_planes", "vsa_nt_import_planes")}
    src_planes = export_planes(src.baked)
    comp_ms = _events(lambda: _composition(src, src_planes, other, res), a.reps)
    comp = _composition(src, src_planes, other, res)
    planes, reports = TT.transfer_planes(src, other)
    same = sum(int(((comp[k] == planes[k]).all(-1) & (comp[k] != 0).any(-1)).sum()) for k in planes)
    written = sum(int((comp[k] != 0).any(-1).sum()) for k in planes)
    owned = sum(r["owned"] * (2 * d + 1) for (_, d), r in reports.items())
    transfer_ms = stages.get("vsa_textransfer_owners", 0.0) + stages.get("vsa_textransfer_planes", 0.0)
    result["reatlas"] = {
        "dst_atlas": 512, "transfer_planes_ms": _spread(whole), "entry_points_ms_per_call": stages,
        "owners_plus_transfer_ms": round(transfer_ms, 3), "composition_ms": _spread(comp_ms),
        "composition_over_stage": round(statistics.median(comp_ms) / statistics.median(whole), 2),
        "owned_pixels": owned, "composition_written_pixels": written,
        "composition_unwritten_share_of_owned": round(1.0 - written / owned, 4),
        "composition_pixels_equal_stage_share_of_written": round(same / max(written, 1), 4),
        "rms_distance_max": max(r["rms_distance"] for r in reports.values()),
        "max_distance": max(r["max_distance"] for r in reports.values())}
    save(result)
    print("reatlas", json.dumps(result["reatlas"]), flush=True)
    result["quality"] = {"reatlas_512": _quality(src, scene, cams, a.size)}
    save(result)
    print("quality reatlas", json.dumps(result["quality"]["reatlas_512"]), flush=True)
    del scene, comp, planes, src_planes

    # ---- (b) levels of detail
    from volsurfs_amd.simplify import simplify_shells
    bare = [TensorMesh(m.vertices, m.faces, None) for m in meshes]
    (lod_meshes, _), simplify_ms = _wall(lambda: simplify_shells(bare, 0.25))
    result["lod"] = {"ratio": 0.25, "simplify_ms": round(simplify_ms, 1),
                     "faces": [int(m.faces.shape[0]) for m in lod_meshes], "cases": {}}
    for top in (1024, 512):
        tres = [max(top >> d, 8) for d in range(len(res))]
        atlased, atlas_ms = _wall(lambda: [compute_atlas(m, top, PAD) for m in lod_meshes])
        for samples in (1, 2):
            TT.transfer_scene(src, atlased, tres, samples=samples)                      # warm-up
            (scene, reports), ms = _wall(lambda: TT.transfer_scene(src, atlased, tres, samples=samples,
                                                                     return_reports=True))
            name = f"res{top}_s{samples}"
            result["lod"]["cases"][name] = {
                "textures_res": tres, "samples": samples, "atlas_ms": round(atlas_ms, 1),
                "transfer_and_import_ms": round(ms, 1),
                "rms_distance_max": max(r["rms_distance"] for r in reports.values()),
                "max_distance": max(r["max_distance"] for r in reports.values())}
            result["quality"][name] = _quality(src, scene, cams, a.size)
            save(result)
            print(name, json.dumps(result["lod"]["cases"][name]), json.dumps(result["quality"][name]), flush=True)
    result["quality"]["source_frame_ms"] = _quality(src, src, cams, a.size)["frame_ms"]
    save(result)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
