"""The reference's sphere tracing loop (volsurfs_py/utils/sphere_tracing.py:9-163) restated in torch for any device,
written from its behaviour: the baseline that tests/test_sphere_trace.py and tools/sphere_trace_bench.py hold
volsurfs_amd.sphere_trace against.  Also what the fixture tests/golden/sphere_trace.npz was recorded with besides the
reference's own loop: the torch bounding sphere, the pinhole rays and the analytic fields.  Not collected by pytest."""
import torch


class TorchBoundingSphere:
    """An origin-centred sphere in torch, any device: `intersect` in vsa_intersect_primitive's fp32 operation order
    (a miss reports t = 0 and its points at the ray origin), `check_points_inside` as background.BoundingSphere."""

    def __init__(self, radius=0.5):
        self.radius = float(radius)

    def get_radius(self):
        return self.radius

    def check_points_inside(self, points):
        return torch.linalg.vector_norm(points, dim=-1) <= self.radius

    def intersect(self, rays_o, rays_d):
        o, d = rays_o, rays_d
        a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        b = 2.0 * ((o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]) + o[:, 2] * d[:, 2])
        c = ((o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2]) - self.radius * self.radius
        disc = b * b - (4.0 * a) * c
        sq = torch.sqrt(torch.clamp(disc, min=0.0))
        tn, tf = (-b - sq) / (2.0 * a), (-b + sq) / (2.0 * a)
        hit = (disc >= 0.0) & (tf > 0.0)
        zero = torch.zeros_like(tn)
        tn = torch.where(hit, torch.clamp(tn, min=0.0), zero)
        tf = torch.where(hit, tf, zero)
        return hit, tn, tf, o + tn.unsqueeze(-1) * d, o + tf.unsqueeze(-1) * d


def fixture_rays(res=48, eye=(0.3, 0.4, 1.2), extent=0.6, dtype=torch.float32):
    """A pinhole view: one ray per cell centre of a res x res grid on [-extent, extent]^2 of the plane z = 0."""
    c = (torch.arange(res, dtype=torch.float64) + 0.5) / res * (2 * extent) - extent
    v, u = torch.meshgrid(c, c, indexing="ij")
    tgt = torch.stack([u, v, torch.zeros_like(u)], -1).reshape(-1, 3)
    o = torch.tensor(eye, dtype=torch.float64).expand_as(tgt)
    d = torch.nn.functional.normalize(tgt - o, dim=-1)
    return o.to(dtype).contiguous(), d.to(dtype).contiguous()


# ---- analytic fields ([M, 3] -> [M, C]), plain elementwise torch
def _norm3(p):
    return torch.sqrt((p[:, 0:1] * p[:, 0:1] + p[:, 1:2] * p[:, 1:2]) + p[:, 2:3] * p[:, 2:3])


def sdf_torus(p, R=0.25, r=0.1):
    q = torch.sqrt(p[:, 0:1] * p[:, 0:1] + p[:, 1:2] * p[:, 1:2]) - R
    return torch.sqrt(q * q + p[:, 2:3] * p[:, 2:3]) - r


def sdf_two_balls(p):
    c = torch.tensor([0.15, 0.0, 0.0], dtype=p.dtype, device=p.device)
    return torch.minimum(_norm3(p - c) - 0.22, _norm3(p + c) - 0.22)


def sdf_two_balls_half(p):
    return sdf_two_balls(p) * 0.5


def sdf_three_columns(p):
    s = sdf_two_balls(p)
    return torch.cat([s + 0.02, s, s - 0.02], 1)


# name -> (field, surf_idx as passed to the reference)
FIXTURE_FIELDS = {"torus": (sdf_torus, None), "two_balls": (sdf_two_balls, None),
                  "two_balls_half": (sdf_two_balls_half, None), "three_col1": (sdf_three_columns, [1]),
                  "three_col2": (sdf_three_columns, [2])}
# (nr_sphere_traces, sdf_converged_tresh): the render's setting, and one that leaves many rays unconverged
FIXTURE_SETTINGS = {"r100": (100, 1e-3), "r12": (12, 1e-4)}
FIXTURE_RADIUS = 0.5


@torch.no_grad()
def sphere_trace_restated(sdf_fn, rays_o, rays_d, bounding_primitive, nr_sphere_traces=30, sdf_converged_tresh=1e-4,
                          sdf_multiplier=1.0, iter_nr=None, surf_idx=None, unconverged_are_hits=False, stats=None):
    """-> (points [N,3], z [N,1], hit [N] bool).  Every round selects the rays that are not done with a boolean
    mask, steps them by the SDF of their points, and writes points and flags back through the mask.  `surf_idx`: None,
    an int (the column kept as [M,1]) or a one-element list.  `stats` (a dict) counts "rounds", "rows" (SDF rows
    evaluated) and "masked_ops" (boolean-mask gathers / writes: on a GPU each is a nonzero whose size the host
    waits for)."""
    _, _, _, p_near, _ = bounding_primitive.intersect(rays_o, rays_d)
    pts = p_near.clone()
    N = pts.shape[0]
    hit = torch.zeros(N, dtype=torch.bool, device=pts.device)
    done = torch.zeros(N, dtype=torch.bool, device=pts.device)
    z = torch.zeros(N, 1, dtype=pts.dtype, device=pts.device)
    if isinstance(surf_idx, int):
        surf_idx = [surf_idx]
    count = (lambda k, v=1: stats.__setitem__(k, stats.get(k, 0) + v)) if stats is not None else (lambda k, v=1: None)
    if N == 0:
        return pts, z, hit
    for _ in range(int(nr_sphere_traces)):
        live = torch.logical_not(done)
        p, d = pts[live, :], rays_d[live, :]
        count("masked_ops", 2)
        if p.shape[0] == 0:
            break
        pred = sdf_fn(p, iter_nr) if iter_nr is not None else sdf_fn(p)
        sdf = pred[0] if isinstance(pred, tuple) else pred
        count("rounds")
        count("rows", p.shape[0])
        if surf_idx is not None:
            sdf = sdf[:, surf_idx]
        sdf = sdf.reshape(p.shape[0], 1)
        p = p + d * (sdf * sdf_multiplier)
        newly = (sdf.abs() < sdf_converged_tresh)[:, 0]
        hit[live] = torch.logical_or(hit[live], newly)
        done[live] = torch.logical_or(done[live], newly)
        inside = bounding_primitive.check_points_inside(p)
        done[live] = torch.logical_or(done[live], torch.logical_not(inside))
        pts[live] = p
        count("masked_ops", 7)
        z = (pts - rays_o).norm(dim=-1, keepdim=True)
    if unconverged_are_hits:
        hit[~done] = True
    return pts, z, hit


def blend_restated(surfs_rgb, surfs_alpha):
    """methods/offsets_surfs.py:810-858 as torch expressions: surfs_rgb [N,K,3], surfs_alpha [N,K,1] (inner to outer)
    -> (surfs_transmittance, surfs_blending_weights [N,K,1], rgb_fg [N,3], bg_transmittance [N,1])."""
    K = surfs_rgb.shape[1]
    rgb, alpha = surfs_rgb.flip(1), surfs_alpha.flip(1)
    T = torch.cumprod(1 - alpha, dim=1)
    if K == 1:
        surfs_T, bg_T = torch.ones_like(T), T.squeeze(-1)
    else:
        surfs_T = torch.cat([torch.ones_like(T[:, :1]), T[:, :-1]], dim=1)
        bg_T = T[:, -1:].squeeze(-1)
    w = surfs_T * alpha
    rgb_fg = (rgb * w).sum(dim=1)
    return surfs_T.flip(1), w.flip(1), rgb_fg, bg_T
