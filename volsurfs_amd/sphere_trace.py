"""Sphere tracing of a signed distance field (volsurfs_py/utils/sphere_tracing.py) with the round bookkeeping on
the device (csrc/sphere_trace.hip): the SDF stays a Python callable (`sdf_fn`, the encoder and MLP launches), and
everything around it — advancing the points, the hit / done flags, the ordered compaction of the live rays into the
next round's dense rows — is two launches per round with no read-back that the host waits for.

An *item* is one (ray, column) pair: `sphere_trace` traces one item per ray, `sphere_trace_columns` K per ray as one
batch, each item stepping by its own column of the SDF block.

The host needs a row count to call `sdf_fn`.  The live count never grows, so an old count is a valid upper bound:
every round copies its count to pinned memory asynchronously, and round r is launched with the count that round
r - COUNT_LAG started with.  Rows past the real count hold copies of points that were live earlier; their SDF is
evaluated and ignored.  The loop ends when a count that has arrived is 0, or after `nr_sphere_traces` rounds.

Two quirks of the reference are kept / resolved:
  * it sets `occupancy_grid = None` on entry: every ray starts at the bounding primitive's near point, and a ray
    that misses the primitive starts at its origin (`vsa_intersect_primitive`'s near point of a miss).  The
    `occupancy_grid` argument is accepted and ignored, as there;
  * with an int `surf_idx` its `sdf[:, surf_idx]` of an [M, C] block is 1-D and the next line raises for any batch
    that is not 3 rows.  The meaning taken here is the selected column kept as [M, 1] (`surf_idx=[k]` there)."""
import torch

from . import _lib
from .background import BoundingBox, BoundingSphere, intersect_bounding_primitive
from .volsurfs import RaySampler

COUNT_LAG = 2      # rounds between a live count and the launch it bounds (0: wait for every round's own count)
_BLOCK = 256       # csrc/sphere_trace.hip ST_BLOCK

last_stats = None  # the last trace's counters (tools/sphere_trace_bench.py): see _trace


class TraceResult:
    """points [S, N, 3], z [S, N], hit [S, N] bool for S columns over N rays; hit_items [H] int32: the hit items
    (slot * N + ray) in ascending order; hit_count: the device's count of them (int32 [1])."""

    def __init__(self, points, z, hit, hit_items, hit_count, nr_rays, nr_slots):
        self.points, self.z, self.hit = points, z, hit
        self.hit_items, self.hit_count = hit_items, hit_count
        self.nr_rays, self.nr_slots = nr_rays, nr_slots

    def hits_per_slot(self):
        """[S] Python ints (one blocking read)."""
        if self.nr_rays == 0:
            return [0] * self.nr_slots
        return [int(c) for c in self.hit.sum(1).tolist()]


def _primitive_kind(bounding_primitive):
    if isinstance(bounding_primitive, BoundingBox):
        return 0, bounding_primitive.half
    if isinstance(bounding_primitive, BoundingSphere):
        return 1, bounding_primitive.radius
    raise _lib.VolsurfsHipError(f"sphere tracing needs a BoundingBox or BoundingSphere, got {type(bounding_primitive)}")


def _sdf_rows(sdf_fn, points, iter_nr):
    pred = sdf_fn(points, iter_nr) if iter_nr is not None else sdf_fn(points)
    sdf = pred[0] if isinstance(pred, tuple) else pred
    if sdf.shape[0] != points.shape[0]:
        raise _lib.VolsurfsHipError(f"sdf_fn returned {sdf.shape[0]} rows for {points.shape[0]} points")
    return _lib.check_f32(sdf.detach().reshape(points.shape[0], -1).contiguous())


@torch.no_grad()
def _trace(sdf_fn, rays_o, rays_d, points_near, bounding_primitive, columns, nr_sphere_traces, sdf_converged_tresh,
           sdf_multiplier, iter_nr, unconverged_are_hits):
    """The traced items of `columns` (a list of column indices, None = the field's only column) -> TraceResult.
    Fills `last_stats`: rounds run, the bound of every round (rows evaluated), blocking host waits, and — after
    the result has been read — the live items per round."""
    global last_stats
    N, S = rays_o.shape[0], len(columns)
    dev = rays_o.device
    if N == 0 or S == 0:
        last_stats = {"rounds": 0, "rows": [], "waits": 0, "counts": None}
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
        return TraceResult(e(S, 0, 3), e(S, 0), e(S, 0, dt=torch.bool), e(0, dt=torch.int32),
                           torch.zeros(1, dtype=torch.int32, device=dev), N, S)
    kind, size = _primitive_kind(bounding_primitive)
    rays_o = _lib.check_f32(rays_o.contiguous(), N, 3)
    rays_d = _lib.check_f32(rays_d.contiguous(), N, 3)
    points_near = _lib.check_f32(points_near.contiguous(), N, 3)
    M = N * S
    R = int(nr_sphere_traces)
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=dev)
    pts, flags, keep = f32(M, 3), u8(M), u8(M)
    live, dense = (i32(M), i32(M)), (f32(M, 3), f32(M, 3))
    block_counts = i32((M + _BLOCK - 1) // _BLOCK)
    counts = i32(R + 2)                                  # [r]: live at the start of round r; [R + 1]: hits
    counts_host = torch.empty(R + 1, dtype=torch.int32).pin_memory()
    slot_cols = torch.tensor([0 if c is None else int(c) for c in columns], dtype=torch.int32, device=dev)
    max_col = max(0 if c is None else int(c) for c in columns)
    stream = _lib.stream_ptr()
    _lib.call("vsa_st_begin", points_near, N, S, pts, flags, live[0], dense[0], counts, stream)
    events, rows, waits, rounds = [None] * (R + 1), [], 0, 0
    for r in range(R):
        q = r - COUNT_LAG
        bound = M
        if q >= 1:
            if not events[q].query():
                waits += 1
                events[q].synchronize()
            bound = int(counts_host[q])
        if bound == 0:
            break
        a, b = r & 1, (r + 1) & 1
        sdf = _sdf_rows(sdf_fn, dense[a][:bound], iter_nr)
        C = sdf.shape[1]
        if max_col >= C or (C > 1 and any(c is None for c in columns)):
            raise _lib.VolsurfsHipError(f"sphere_trace: columns {columns} of an SDF block with {C} column(s)")
        _lib.call("vsa_st_step", live[a], counts[r:], sdf, C, slot_cols, N, rays_d, float(sdf_multiplier),
                  float(sdf_converged_tresh), kind, float(size), pts, flags, keep, block_counts, dense[a], live[b],
                  dense[b], counts[r + 1:], bound, stream)
        counts_host[r + 1:r + 2].copy_(counts[r + 1:r + 2], non_blocking=True)
        events[r + 1] = torch.cuda.Event()
        events[r + 1].record()
        rows.append(bound)
        rounds += 1
    z, hit, hit_items = f32(M), u8(M), i32(M)
    _lib.call("vsa_st_finish", pts, rays_o, N, S, flags, bool(unconverged_are_hits), z, hit, keep, block_counts,
              hit_items, counts[R + 1:], stream)
    last_stats = {"rounds": rounds, "rows": rows, "waits": waits, "counts": counts_host, "nr_items": M}
    return TraceResult(pts.view(S, N, 3), z.view(S, N), hit.view(S, N).bool(), hit_items, counts[R + 1:R + 2], N, S)


def stats_summary():
    """`last_stats` as plain numbers; call after the device has finished the trace (the live counts per round sit
    in pinned memory): rounds, live items per round, rows evaluated, padded rows, blocking host waits."""
    s = last_stats
    if not s or not s["rounds"]:
        return {"rounds": 0, "live": [], "rows": 0, "padded_rows": 0, "waits": 0}
    live = [s["nr_items"]] + [int(c) for c in s["counts"][1:s["rounds"]].tolist()]
    return {"rounds": s["rounds"], "live": live, "rows": sum(s["rows"]), "padded_rows": sum(s["rows"]) - sum(live),
            "waits": s["waits"]}


def _column(surf_idx):
    if surf_idx is None:
        return None
    if isinstance(surf_idx, (list, tuple)):
        if len(surf_idx) != 1:
            raise _lib.VolsurfsHipError("sphere_trace: surf_idx selects one column (sphere_trace_columns takes several)")
        return int(surf_idx[0])
    return int(surf_idx)


def _pack(points_near, rays_d, points, z):
    pack = RaySampler.init_with_one_sample_per_ray(points_near, rays_d)
    pack.samples_3d, pack.samples_z = points, z.unsqueeze(-1)
    return pack


@torch.no_grad()
def sphere_trace(sdf_fn, rays_o, rays_d, bounding_primitive, nr_sphere_traces=30, sdf_converged_tresh=1e-4,
                 sdf_multiplier=1.0, occupancy_grid=None, iter_nr=None, surf_idx=None, unconverged_are_hits=False):
    """utils/sphere_tracing.py:9-163 -> (RaySamplesPacked with one sample per ray, samples_3d [N,3] = the final
    points and samples_z [N,1] = their distance from the ray origins; ray_hit_flag [N] bool).  `sdf_fn(points)` or
    `sdf_fn(points, iter_nr)` returns a tensor or a tuple whose first element is taken, [M,1] or [M,C]; `surf_idx`
    (an int or a one-element list) selects the column.  See the module docstring for the two reference quirks:
    `occupancy_grid` is ignored, and an int `surf_idx` means that column kept as [M,1]."""
    raycast = intersect_bounding_primitive(bounding_primitive, rays_o, rays_d)
    res = _trace(sdf_fn, rays_o, rays_d, raycast["points_near"], bounding_primitive, [_column(surf_idx)],
                 nr_sphere_traces, sdf_converged_tresh, sdf_multiplier, iter_nr, unconverged_are_hits)
    return _pack(raycast["points_near"], rays_d, res.points[0], res.z[0]), res.hit[0]


@torch.no_grad()
def sphere_trace_columns(sdf_fn, rays_o, rays_d, bounding_primitive, columns, nr_sphere_traces=30,
                         sdf_converged_tresh=1e-4, sdf_multiplier=1.0, iter_nr=None, unconverged_are_hits=False):
    """`columns` of one SDF block traced as one batch of N x len(columns) items, every item stepping by its own
    column -> [(pack, ray_hit_flag)] per column, each equal to the bytes of `sphere_trace(..., surf_idx=column)`
    (an item's arithmetic reads its own row only): K surfaces cost one loop of rounds, not K."""
    raycast = intersect_bounding_primitive(bounding_primitive, rays_o, rays_d)
    res = _trace(sdf_fn, rays_o, rays_d, raycast["points_near"], bounding_primitive, [int(c) for c in columns],
                 nr_sphere_traces, sdf_converged_tresh, sdf_multiplier, iter_nr, unconverged_are_hits)
    return [(_pack(raycast["points_near"], rays_d, res.points[s], res.z[s]), res.hit[s])
            for s in range(len(columns))]


def scatter_rows(hit_items, nr_hits, rows, nr_rays, nr_slots=1):
    """[H, C] rows of the hit items -> a zero [N, C] (one slot) or [N, S, C] tensor with the rows at their rays."""
    rows = _lib.check_f32(rows.contiguous())
    C = rows.shape[1]
    out = torch.zeros((nr_rays, C) if nr_slots == 1 else (nr_rays, nr_slots, C), device=rows.device)
    if nr_hits and nr_rays:
        _lib.call("vsa_st_scatter", hit_items, int(nr_hits), rows, C, nr_rays, nr_slots, out, _lib.stream_ptr())
    return out


def blend_surfaces(surfs_rgb, surfs_alpha):
    """methods/offsets_surfs.py:810-858 for surfs_rgb [N,K,3] and surfs_alpha [N,K,1] (surfaces inner to outer) ->
    (surfs_transmittance [N,K,1], surfs_blending_weights [N,K,1], rgb_fg [N,3], bg_transmittance [N,1]) in one
    launch; bit-identical to the reference's flip / cumprod / sum expression as torch evaluates it on the device."""
    N, K = surfs_rgb.shape[0], surfs_rgb.shape[1]
    surfs_rgb = _lib.check_f32(surfs_rgb.contiguous(), N, K, 3)
    surfs_alpha = _lib.check_f32(surfs_alpha.contiguous(), N, K, 1)
    dev = surfs_rgb.device
    T, w = torch.empty(N, K, 1, device=dev), torch.empty(N, K, 1, device=dev)
    rgb_fg, bg_T = torch.empty(N, 3, device=dev), torch.empty(N, 1, device=dev)
    _lib.call("vsa_st_blend", surfs_rgb, surfs_alpha, N, K, T, w, rgb_fg, bg_T, _lib.stream_ptr())
    return T, w, rgb_fg, bg_T
