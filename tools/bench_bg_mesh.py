"""TSDF fusion of the background mesh (volsurfs_amd/bg_mesh.py, csrc/tsdf_fuse.hip) at the size the baker
stage runs at: 100 views of 800 x 800 fused on the 256^3 and 512^3 lattices.

The scene is synthetic and built on the device: a ball of radius 0.5 inside a shell of radius 0.95 whose far wall
every other pixel sees, so that every pixel carries a depth, seen from Fibonacci points of the sphere of radius 2.2.
Per resolution, device ms from events, median (min - max) of --reps runs after a warm-up, in one process:
  * `fused`      vsa_tsdf_fuse_lattice, one launch;
  * `per_view`   the reference's formulation on the same GPU: tests/bg_mesh_restated.py's per-view torch loop over the
                 lattice in chunks of 256^3 points (the chunk of the reference's `evaluate`);
  * `colours`    vsa_tsdf_fuse_points with colours at the extracted mesh's vertices;
  * `extract`    the whole extract_mesh_unbounded (fusion, marching cubes, vertex step, colours).
Traffic of the fused kernel: `tap_bytes` = 16 B per (point, view) pair inside the frustum, what the lanes ask for;
`footprint_bytes` = 4 B per DISTINCT texel a 4 x 4 x 4 brick touches in a view, summed over bricks and views (counted
exactly on --footprint-views views spread over the set and scaled to all): the depth maps once per wave footprint;
plus 4 B per point written.  `GB_per_s` = (footprint_bytes + 4 n^3) / fused time.

    python tools/bench_bg_mesh.py [--reps 5] [--views 100] [--size 800] [--res 256 512] [--out profiles/bg_mesh.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BALL_R, SHELL_R, EYE_R = 0.5, 0.95, 2.2


def scene(nr_views, size, focal, device="cuda"):
    """-> (depthmaps, rgbmaps, c2ws, intrinsics) as MeshExtractor takes them, the maps on the device."""
    import numpy as np
    import torch
    import bg_mesh_restated as BG
    K = np.array([[focal, 0, 0.5 * size], [0, focal, 0.5 * size], [0, 0, 1]], np.float64)
    px = torch.arange(size, device=device, dtype=torch.float64) * size / (size - 1)
    dy, dx = torch.meshgrid((px - K[1, 2]) / focal, (px - K[0, 2]) / focal, indexing="ij")
    d_cam = torch.stack([dx, dy, torch.ones_like(dx)], -1)
    depths, rgbs, c2ws, ixts = [], [], [], []
    for eye in BG.fibonacci_sphere(nr_views, EYE_R):
        c2w = BG.look_at_pose(eye)
        R, o = torch.from_numpy(c2w[:3, :3]).to(device), torch.from_numpy(c2w[:3, 3]).to(device)
        d = d_cam @ R.T
        A, B = (d * d).sum(-1), 2.0 * (d @ o)
        root = lambda r, sign: (-B + sign * torch.sqrt((B * B - 4.0 * A * (o @ o - r * r)).clamp_min(0.0))) / (2.0 * A)
        hit = B * B - 4.0 * A * (o @ o - BALL_R ** 2) > 0
        in_shell = B * B - 4.0 * A * (o @ o - SHELL_R ** 2) > 0
        t = torch.where(hit, root(BALL_R, -1.0), torch.where(in_shell, root(SHELL_R, 1.0), torch.zeros_like(A)))
        p = o + t[..., None] * d
        rgb = 0.5 + 0.5 * p / p.norm(dim=-1, keepdim=True).clamp_min(1e-9)
        depths.append(t[None].float())
        rgbs.append(rgb.permute(2, 0, 1).float().contiguous())
        c2ws.append(c2w.astype(np.float32))
        ixts.append(K.astype(np.float32))
    return depths, rgbs, c2ws, ixts


def timed(fn, reps):
    import torch
    fn()                                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
        del out
    return [round(f(ms), 3) for f in (statistics.median, min, max)]


def per_view_lattice(ex, n, trunc):
    """The reference's formulation: the per-view torch loop over the lattice, 256^3 points at a time."""
    import torch
    import bg_mesh_restated as BG
    ax = torch.linspace(-1.0, 1.0, n, dtype=torch.float32).cuda()
    out = torch.empty(n, n, n, device="cuda")
    step = max(1, 256 ** 3 // (n * n))                     # i-slabs of 256^3 points
    for i0 in range(0, n, step):
        pts = torch.stack(torch.meshgrid(ax[i0:i0 + step], ax, ax, indexing="ij"), -1).reshape(-1, 3)
        out[i0:i0 + step] = BG.fuse_restated(pts, ex.depthmaps, ex.rgbmaps, ex.full_proj_transform, trunc)[0] \
            .reshape(-1, n, n)
    return out


def traffic(ex, n, views):
    """(pairs inside the frustum, distinct texels per brick summed over bricks) over `views`, exactly, in torch."""
    import torch
    assert n % 4 == 0
    ax = torch.linspace(-1.0, 1.0, n, dtype=torch.float32).cuda()
    H, W = ex.height, ex.width
    pairs = distinct = 0
    step = max(4, (128 ** 3 // (n * n)) // 4 * 4)
    for v in views:
        P = ex.full_proj_transform[v]
        for i0 in range(0, n, step):
            xs = ax[i0:i0 + step]
            pts = torch.stack(torch.meshgrid(xs, ax, ax, indexing="ij"), -1)
            h = pts @ P[:, :3].T + P[:, 3]
            z = h[..., 3]
            u, w = h[..., 0] / z, h[..., 1] / z
            m = (u > -1) & (u < 1) & (w > -1) & (w < 1) & (z > 0)
            x0 = (((u + 1) / 2) * (W - 1)).clamp(0, W - 1).floor().long()
            y0 = (((w + 1) / 2) * (H - 1)).clamp(0, H - 1).floor().long()
            ni = xs.shape[0]
            ii, jj, kk = torch.meshgrid(torch.arange(ni, device="cuda") // 4, torch.arange(n, device="cuda") // 4,
                                        torch.arange(n, device="cuda") // 4, indexing="ij")
            brick = ((ii * (n // 4) + jj) * (n // 4) + kk)[m]
            x0, y0 = x0[m], y0[m]
            pairs += int(m.sum())
            keys = torch.cat([brick * (H * W) + (y0 + a).clamp_max(H - 1) * W + (x0 + b).clamp_max(W - 1)
                              for a in (0, 1) for b in (0, 1)])
            distinct += int(torch.unique(keys).numel())
            del keys, brick, pts, h
    return pairs, distinct


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--focal", type=float, default=700.0)
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--footprint-views", type=int, default=5)
    ap.add_argument("--skip-per-view", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from volsurfs_amd.bg_mesh import MeshExtractor
    assert torch.cuda.is_available(), "bench_bg_mesh needs a GPU"
    ex = MeshExtractor(*scene(a.views, a.size, a.focal), with_vertex_colors=True)
    rows = []
    for n in a.res:
        trunc = ex.truncation(n)[1]
        row = {"resolution": n, "views": a.views, "size": a.size, "reps": a.reps}
        row["fused_ms"] = timed(lambda: ex.fuse_lattice(n), a.reps)
        if not a.skip_per_view:
            row["per_view_ms"] = timed(lambda: per_view_lattice(ex, n, trunc), max(1, a.reps // 2))
            row["ratio"] = round(row["per_view_ms"][0] / row["fused_ms"][0], 2)
            gap = (per_view_lattice(ex, n, trunc) - ex.fuse_lattice(n)).abs()
            row["max_gap_to_per_view"] = float(gap.max())
            row["share_beyond_1e-3"] = float((gap > 1e-3).float().mean())
            del gap
        mesh, _ = ex.extract_mesh_unbounded(resolution=n)
        row["vertices"], row["faces"] = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
        verts = mesh.vertices
        row["colours_ms"] = timed(lambda: ex.fuse_points(verts, return_rgb=True, resolution=n), a.reps)
        row["extract_ms"] = timed(lambda: ex.extract_mesh_unbounded(resolution=n), a.reps)
        del mesh, verts
        views = sorted({int(round(i * (a.views - 1) / max(1, a.footprint_views - 1))) for i in range(a.footprint_views)})
        pairs, distinct = traffic(ex, n, views)
        scale = a.views / len(views)
        row["tap_bytes"] = int(16 * pairs * scale)
        row["footprint_bytes"] = int(4 * distinct * scale)
        row["out_bytes"] = 4 * n ** 3
        row["pairs_in_frustum_share"] = round(pairs * scale / (n ** 3 * a.views), 4)
        sec = row["fused_ms"][0] * 1e-3
        row["GB_per_s"] = round((row["footprint_bytes"] + row["out_bytes"]) / sec / 1e9, 1)
        row["tap_GB_per_s"] = round(row["tap_bytes"] / sec / 1e9, 1)
        row["Gpairs_per_s"] = round(n ** 3 * a.views / sec / 1e9, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
