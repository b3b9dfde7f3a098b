// Camera hits of K shells by screen-space bins instead of K BVH walks per ray.  (The reference deploys its shells
// through a rasterizer outside its tree; the bin rule is this library's own -- include/volsurfs_hip.h "Shell
// rasterization", DESIGN §35: restated in tests/rasterize_restated.py, unpinned.)
//
// The rays of a whole frame share their origin, and the samples of an 8 x 8 tile see the same handful of triangles.
// tri_test (trace_walk.h) has a total order on hits (smallest t, ties to the smallest original face id, a hit iff
// t > t_min), so the closest hit over a list of triangles does not depend on the order of the list: the same tri_test
// on the same pinhole_ray (pinhole.h) over any list that holds every triangle the ray's walk would accept gives
// vsa_trace_q's hit record bit for bit.
//
// vsa_shell_raster_setup: one lane per triangle slot.  The lane moves the three vertices into camera space, classifies
//   the face (dropped / behind / straddling / in front), boxes an in-front face in 8 x 8-sample tiles with the
//   one-pixel margin and adds 1 to the counter of every (shell, tile) the box touches; a straddling face is appended
//   to its shell's list, which every tile of the shell walks.  Then a scan of the counters and one blocking read of the
//   four statistics: the caller sizes the pair list from them.
// vsa_shell_raster_draw: the fill pass (one lane per slot, the box the setup pass stored, one integer atomic per pair:
//   the order inside a tile's list is whatever the schedule makes it, and does not matter), then the raster pass: one
//   wave per (shell, tile), one lane per sample, the ray made in registers, every lane on the same triangle -- the
//   list entry and the three float4 of its record are wave-uniform loads -- and write_hit.  No stack, no LDS.
// Integer atomics only: the same inputs give the same bytes.
#include "mesh_topology.h"
#include "pinhole.h"
#include "trace_walk.h"

namespace {

constexpr long long MAX_I32 = 0x7fffffffll;
constexpr int SETUP_BLOCK = 256;
constexpr int RASTER_TILE = 8;                 // samples per tile side: one wave per tile

enum { FACE_DROPPED = 0, FACE_BEHIND = 1, FACE_STRADDLING = 2, FACE_FRONT = 3 };
enum { STAT_BEHIND = 0, STAT_STRADDLING = 1, STAT_BINNED = 2, STAT_PAIRS = 3 };

struct SlotRanges {
  int first[VSA_MAX_SHELLS], count[VSA_MAX_SHELLS];
};

struct TileBox {
  int x0, y0, x1, y1;      // tiles, inclusive; x0 > x1: the face is in no tile's list
};

struct RasterGrid {
  int tiles_x, tiles;      // per shell
  int samples_h, samples_w, supersample, width;
};

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

// p = R^T (v - t), c2w = [R | t].
__device__ __forceinline__ void to_camera(const float* __restrict__ c2w, float vx, float vy, float vz, float& x, float& y,
                                          float& z) {
  const float wx = vx - c2w[3], wy = vy - c2w[7], wz = vz - c2w[11];
  x = (c2w[0] * wx + c2w[4] * wy) + c2w[8] * wz;
  y = (c2w[1] * wx + c2w[5] * wy) + c2w[9] * wz;
  z = (c2w[2] * wx + c2w[6] * wy) + c2w[10] * wz;
}

// The bin rule (include/volsurfs_hip.h "Shell rasterization"), fp32 in the order written.  Returns the class; `box` is
// set for FACE_FRONT (x0 > x1 when the expanded box misses the image).
__device__ __forceinline__ int classify(const float4 v0, const float4 e1, const float4 e2, const float* __restrict__ c2w,
                                        const float* __restrict__ k, const RasterGrid g, TileBox& box) {
  box = TileBox{1, 1, 0, 0};
  const float ax = v0.x, ay = v0.y, az = v0.z;
  const float bx = v0.x + e1.x, by = v0.y + e1.y, bz = v0.z + e1.z;
  const float cx = v0.x + e2.x, cy = v0.y + e2.y, cz = v0.z + e2.z;
  if (!(finite3(ax, ay, az) && finite3(bx, by, bz) && finite3(cx, cy, cz))) return FACE_DROPPED;
  float px[3], py[3], pz[3];
  to_camera(c2w, ax, ay, az, px[0], py[0], pz[0]);
  to_camera(c2w, bx, by, bz, px[1], py[1], pz[1]);
  to_camera(c2w, cx, cy, cz, px[2], py[2], pz[2]);
  const float zg = 1e-4f * fmaxf(1.0f, fmaxf(fmaxf(fabsf(c2w[3]), fabsf(c2w[7])), fabsf(c2w[11])));
  if (pz[0] < -zg && pz[1] < -zg && pz[2] < -zg) return FACE_BEHIND;
  if (!(pz[0] > zg && pz[1] > zg && pz[2] > zg)) return FACE_STRADDLING;
  float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float hx = (k[0] * px[i] + k[1] * py[i]) + k[2] * pz[i];
    const float hy = (k[3] * px[i] + k[4] * py[i]) + k[5] * pz[i];
    const float hw = (k[6] * px[i] + k[7] * py[i]) + k[8] * pz[i];
    if (!(hw > 0.0f)) return FACE_STRADDLING;
    const float u = hx / hw, v = hy / hw;
    if (!(fabsf(u) < INFINITY && fabsf(v) < INFINITY)) return FACE_STRADDLING;
    lo_x = fminf(lo_x, u), hi_x = fmaxf(hi_x, u);
    lo_y = fminf(lo_y, v), hi_y = fmaxf(hi_y, v);
  }
  // pixels -> samples, one pixel of margin on every side; clamped in float before the conversion
  const float s = (float)g.supersample;
  const float x0 = floorf((lo_x - 1.0f) * s), x1 = floorf((hi_x + 1.0f) * s);
  const float y0 = floorf((lo_y - 1.0f) * s), y1 = floorf((hi_y + 1.0f) * s);
  const float max_x = (float)(g.samples_w - 1), max_y = (float)(g.samples_h - 1);
  if (x1 < 0.0f || y1 < 0.0f || x0 > max_x || y0 > max_y) return FACE_FRONT;      // off the image: no tile
  // (the integer min: (float)(samples - 1) rounds up past 2^24 samples a side; it never binds below that)
  const int last_x = g.tiles_x - 1, last_y = g.tiles / g.tiles_x - 1;
  box.x0 = min((int)fmaxf(x0, 0.0f) / RASTER_TILE, last_x);
  box.x1 = min((int)fminf(x1, max_x) / RASTER_TILE, last_x);
  box.y0 = min((int)fmaxf(y0, 0.0f) / RASTER_TILE, last_y);
  box.y1 = min((int)fminf(y1, max_y) / RASTER_TILE, last_y);
  return FACE_FRONT;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) v += (unsigned long long)__shfl_xor((long long)v, w);
  return v;
}

__global__ __launch_bounds__(SETUP_BLOCK) void raster_setup_kernel(
    const float4* __restrict__ tris, SlotRanges ranges, const float* __restrict__ c2w, const float* __restrict__ k,
    RasterGrid g, TileBox* __restrict__ boxes, int* __restrict__ tile_count, int* __restrict__ strad_list,
    int* __restrict__ strad_count, unsigned long long* __restrict__ stats) {
  const int mesh = blockIdx.y;
  const long long i = (long long)blockIdx.x * SETUP_BLOCK + threadIdx.x;
  const bool alive = i < ranges.count[mesh];
  int cls = FACE_DROPPED;
  unsigned long long pairs = 0;
  if (alive) {
    const long long slot = ranges.first[mesh] + i;
    TileBox box;
    cls = classify(tris[3 * slot], tris[3 * slot + 1], tris[3 * slot + 2], c2w, k, g, box);
    boxes[slot] = box;
    if (cls == FACE_STRADDLING) {
      const int pos = atomicAdd(strad_count + mesh, 1);
      strad_list[ranges.first[mesh] + pos] = (int)slot;         // (pos < count[mesh]: one append per slot)
    }
    if (box.x0 <= box.x1) {
      int* const counts = tile_count + (long long)mesh * g.tiles;
      for (int ty = box.y0; ty <= box.y1; ++ty)
        for (int tx = box.x0; tx <= box.x1; ++tx) atomicAdd(counts + (long long)ty * g.tiles_x + tx, 1);
      pairs = (unsigned long long)(box.x1 - box.x0 + 1) * (unsigned long long)(box.y1 - box.y0 + 1);
    }
  }
  const int nr_behind = __popcll(__builtin_amdgcn_ballot_w64(cls == FACE_BEHIND));
  const int nr_strad = __popcll(__builtin_amdgcn_ballot_w64(cls == FACE_STRADDLING));
  const int nr_binned = __popcll(__builtin_amdgcn_ballot_w64(pairs != 0));
  pairs = wave_sum(pairs);
  if ((threadIdx.x & 63) == 0) {
    if (nr_behind) atomicAdd(stats + STAT_BEHIND, (unsigned long long)nr_behind);
    if (nr_strad) atomicAdd(stats + STAT_STRADDLING, (unsigned long long)nr_strad);
    if (nr_binned) atomicAdd(stats + STAT_BINNED, (unsigned long long)nr_binned);
    if (pairs) atomicAdd(stats + STAT_PAIRS, pairs);
  }
}

__global__ __launch_bounds__(SETUP_BLOCK) void raster_fill_kernel(SlotRanges ranges, RasterGrid g,
                                                                  const TileBox* __restrict__ boxes,
                                                                  const int* __restrict__ tile_start,
                                                                  int* __restrict__ cursor, long long nr_pairs,
                                                                  int* __restrict__ pairs) {
  const int mesh = blockIdx.y;
  const long long i = (long long)blockIdx.x * SETUP_BLOCK + threadIdx.x;
  if (i >= ranges.count[mesh]) return;
  const long long slot = ranges.first[mesh] + i;
  TileBox box = boxes[slot];
  // (no-ops on the setup pass's boxes: a workspace that is not this frame's must not move an atomic off the counters)
  box.x0 = max(box.x0, 0), box.y0 = max(box.y0, 0);
  box.x1 = min(box.x1, g.tiles_x - 1), box.y1 = min(box.y1, g.tiles / g.tiles_x - 1);
  const long long base = (long long)mesh * g.tiles;
  for (int ty = box.y0; ty <= box.y1; ++ty)
    for (int tx = box.x0; tx <= box.x1; ++tx) {
      const long long t = base + (long long)ty * g.tiles_x + tx;
      const long long at = (long long)tile_start[t] + atomicAdd(cursor + t, 1);
      if (at >= 0 && at < nr_pairs) pairs[at] = (int)slot;      // (always, for the setup pass's counts)
    }
}

// One wave per (shell, tile); lane = sample (lane & 7, lane >> 3) of the tile.
template <bool DIRS>
__global__ __launch_bounds__(TRACE_BLOCK) void raster_kernel(
    const float4* __restrict__ tris, long long nr_slots, SlotRanges ranges, const float* __restrict__ c2w,
    const float* __restrict__ kinv, RasterGrid g, const int* __restrict__ tile_start, long long nr_pairs,
    const int* __restrict__ pairs, const int* __restrict__ strad_list, const int* __restrict__ strad_count, float t_min,
    long long nr_samples, float* __restrict__ hit_t, int* __restrict__ hit_slot, float* __restrict__ hit_uv,
    float* __restrict__ rays_d) {
  const int lane = threadIdx.x;
  const int mesh = blockIdx.y;
  const int tile = blockIdx.x;
  const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
  const int X = tx * RASTER_TILE + (lane & 7), Y = ty * RASTER_TILE + (lane >> 3);
  const bool alive = X < g.samples_w && Y < g.samples_h;        // edge tiles: the lanes outside the image sit out
  const int ss = g.supersample;
  const int col = X / ss, row = Y / ss;
  const int si = X - col * ss, sj = Y - row * ss;
  const float s = (float)ss;
  const float x = (float)col + ((float)si + 0.5f) / s;
  const float y = (float)row + ((float)sj + 0.5f) / s;
  const RayOut r = pinhole_ray(c2w, kinv, x, y);
  const float ox = r.ox, oy = r.oy, oz = r.oz, dx = r.dx, dy = r.dy, dz = r.dz;

  Hit best = no_hit();
  // two lists, both wave-uniform: the tile's pairs, then the shell's straddling faces
  const long long t = (long long)mesh * g.tiles + tile;
  const long long begin = min(max((long long)tile_start[t], 0ll), nr_pairs);
  const long long end = min((long long)tile_start[t + 1], nr_pairs);
#pragma unroll 1
  for (int which = 0; which < 2; ++which) {
    const int* const list = which == 0 ? pairs + begin : strad_list + ranges.first[mesh];
    const int n = which == 0 ? (int)max(end - begin, 0ll) : min(strad_count[mesh], ranges.count[mesh]);
    for (int p0 = 0; p0 < n; p0 += 4) {
      float4 tv[4][3];
      int sl[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sl[i] = list[min(p0 + i, n - 1)];
        const long long q = min(max((long long)sl[i], 0ll), nr_slots - 1);
        tv[i][0] = tris[3 * q];
        tv[i][1] = tris[3 * q + 1];
        tv[i][2] = tris[3 * q + 2];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (p0 + i < n) tri_test(tv[i][0], tv[i][1], tv[i][2], ox, oy, oz, dx, dy, dz, t_min, sl[i], best);
    }
  }
  if (!alive) return;
  // pixel-major, a pixel's s^2 samples consecutive, j outer, i inner
  const long long o = ((long long)row * g.width + col) * (ss * ss) + sj * ss + si;
  write_hit(best, (long long)mesh * nr_samples + o, hit_t, hit_slot, hit_uv);
  if (DIRS && mesh == 0) rays_d[3 * o] = dx, rays_d[3 * o + 1] = dy, rays_d[3 * o + 2] = dz;
}

struct Layout {
  size_t stats, strad_count, tile_count, tile_start, cursor, boxes, strad_list, fixed, tmp, tmp_bytes, total;
  long long tiles_x, tiles;
};

// Status of the image arguments (before any HIP call) and the tile grid.
int raster_grid(int nr_meshes, int height, int width, int supersample, RasterGrid* g) {
  if (nr_meshes < 1 || nr_meshes > VSA_MAX_SHELLS || height < 1 || width < 1 || supersample < 1 || supersample > 8)
    return VSA_ERR_ARG;
  long long samples = (long long)height * width;             // (each factor checked before the next product)
  if (samples >= (1ll << 31)) return VSA_ERR_ARG;
  samples *= supersample * supersample;
  if (samples >= (1ll << 31)) return VSA_ERR_ARG;
  const long long sh = (long long)height * supersample, sw = (long long)width * supersample;
  const long long tiles_x = (sw + RASTER_TILE - 1) / RASTER_TILE, tiles_y = (sh + RASTER_TILE - 1) / RASTER_TILE;
  const long long tiles = tiles_x * tiles_y;                 // <= samples
  if (tiles * nr_meshes + 1 > MAX_I32) return VSA_ERR_UNSUPPORTED;
  *g = RasterGrid{(int)tiles_x, (int)tiles, (int)sh, (int)sw, supersample, width};
  return VSA_OK;
}

int raster_layout(long long nr_slots, int nr_meshes, const RasterGrid& g, Layout* L, bool with_scan = true) {
  const size_t cells = (size_t)g.tiles * nr_meshes + 1;      // (+ 1: the scan's last entry is the pair count)
  mt::Bump b;
  L->stats = b.take(4 * sizeof(long long));
  L->strad_count = b.take(4 * VSA_MAX_SHELLS);
  L->tile_count = b.take(4 * cells);
  L->tile_start = b.take(4 * cells);
  L->cursor = b.take(4 * cells);
  L->boxes = b.take(sizeof(TileBox) * (size_t)nr_slots);
  L->strad_list = b.take(4 * (size_t)nr_slots);
  L->fixed = b.o;                                            // (what the scan's storage comes on top of)
  if (!with_scan) return VSA_OK;
  mt::TmpCounts n = {};
  n.xscan32 = cells;
  MT_TRY(mt::tmp_bytes(n, &L->tmp_bytes));
  L->tmp = b.take(L->tmp_bytes);
  L->total = b.o;
  return VSA_OK;
}

// The layout, and VSA_ERR_ARG for a workspace smaller than it.  The size of the scan's storage is a query of the scan
// library: a workspace that cannot even hold the rest is refused before that query, i.e. before any HIP call.
int checked_layout(long long nr_slots, int nr_meshes, const RasterGrid& g, long long workspace_bytes, Layout* L) {
  MT_TRY(raster_layout(nr_slots, nr_meshes, g, L, false));
  if (workspace_bytes < (long long)L->fixed) return VSA_ERR_ARG;
  MT_TRY(mt::abi_status(raster_layout(nr_slots, nr_meshes, g, L)));
  return workspace_bytes < (long long)L->total ? VSA_ERR_ARG : VSA_OK;
}

// The slot ranges of the shells: inside [0, nr_slots), none negative.
int slot_ranges(const int32_t* mesh_tri_offset, const int32_t* mesh_nr_tris, int nr_meshes, long long nr_slots,
                SlotRanges* r) {
  for (int i = 0; i < VSA_MAX_SHELLS; ++i) {
    r->first[i] = i < nr_meshes ? mesh_tri_offset[i] : 0;
    r->count[i] = i < nr_meshes ? mesh_nr_tris[i] : 0;
    if (r->first[i] < 0 || r->count[i] < 0 || (long long)r->first[i] + r->count[i] > nr_slots) return VSA_ERR_ARG;
  }
  return VSA_OK;
}

int max_count(const SlotRanges& r) {
  int m = 1;
  for (int i = 0; i < VSA_MAX_SHELLS; ++i) m = r.count[i] > m ? r.count[i] : m;
  return m;
}

// What setup and draw check alike, before any HIP call.
int check_raster_args(const float* tris, long long nr_slots, const int32_t* mesh_tri_offset, const int32_t* mesh_nr_tris,
                      int nr_meshes, const float* c2w, const float* intrinsics, const float* intrinsics_inv, int height,
                      int width, int supersample, float t_min, const void* workspace, RasterGrid* g, SlotRanges* r) {
  if (!tris || !mesh_tri_offset || !mesh_nr_tris || !c2w || !intrinsics || !intrinsics_inv || !workspace)
    return VSA_ERR_ARG;
  if (nr_slots < 1 || !(t_min >= 0.0f) || !(t_min < INFINITY)) return VSA_ERR_ARG;
  MT_TRY(raster_grid(nr_meshes, height, width, supersample, g));
  if (nr_slots > MAX_I32) return VSA_ERR_UNSUPPORTED;
  return slot_ranges(mesh_tri_offset, mesh_nr_tris, nr_meshes, nr_slots, r);
}

}  // namespace

extern "C" long long vsa_shell_raster_workspace_bytes(long long nr_slots, int nr_meshes, int height, int width,
                                                      int supersample) {
  RasterGrid g;
  if (nr_slots < 1) return VSA_ERR_ARG;
  if (const int rc = raster_grid(nr_meshes, height, width, supersample, &g)) return rc;
  if (nr_slots > MAX_I32) return VSA_ERR_UNSUPPORTED;
  Layout L;
  if (const int rc = raster_layout(nr_slots, nr_meshes, g, &L)) return mt::abi_status(rc);
  return (long long)L.total;
}

extern "C" int vsa_shell_raster_setup(const float* tris, long long nr_slots, const int32_t* mesh_tri_offset,
                                      const int32_t* mesh_nr_tris, int nr_meshes, const float* c2w,
                                      const float* intrinsics, const float* intrinsics_inv, int height, int width,
                                      int supersample, float t_min, void* workspace, long long workspace_bytes,
                                      long long* stats, void* stream) {
  RasterGrid g;
  SlotRanges r;
  MT_TRY(check_raster_args(tris, nr_slots, mesh_tri_offset, mesh_nr_tris, nr_meshes, c2w, intrinsics, intrinsics_inv,
                           height, width, supersample, t_min, workspace, &g, &r));
  if (!stats) return VSA_ERR_ARG;
  Layout L;
  MT_TRY(checked_layout(nr_slots, nr_meshes, g, workspace_bytes, &L));
  const hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  const size_t cells = (size_t)g.tiles * nr_meshes + 1;
  // stats, the straddler counts and the tile counters lie in front of the workspace, one after the other
  VSA_HIP_TRY(hipMemsetAsync(ws + L.stats, 0, L.tile_count + 4 * cells - L.stats, st));
  const dim3 grid((unsigned)vsa_div_up(max_count(r), SETUP_BLOCK), nr_meshes), block(SETUP_BLOCK);
  hipLaunchKernelGGL(raster_setup_kernel, grid, block, 0, st, reinterpret_cast<const float4*>(tris), r, c2w, intrinsics, g,
                     mt::at<TileBox>(ws, L.boxes), mt::at<int>(ws, L.tile_count), mt::at<int>(ws, L.strad_list),
                     mt::at<int>(ws, L.strad_count), mt::at<unsigned long long>(ws, L.stats));
  MT_LAUNCHED();
  MT_TRY(mt::exclusive_scan({ws + L.tmp, L.tmp_bytes}, mt::at<int32_t>(ws, L.tile_count),
                            mt::at<int32_t>(ws, L.tile_start), cells, st));
  MT_TRY(mt::read_counters(st, mt::at<long long>(ws, L.stats), stats, 4));
  // (the 32-bit scan has wrapped by then; nothing reads it)
  return stats[STAT_PAIRS] > MAX_I32 ? VSA_ERR_UNSUPPORTED : VSA_OK;
}

extern "C" int vsa_shell_raster_draw(const float* tris, long long nr_slots, const int32_t* mesh_tri_offset,
                                     const int32_t* mesh_nr_tris, int nr_meshes, const float* c2w,
                                     const float* intrinsics, const float* intrinsics_inv, int height, int width,
                                     int supersample, float t_min, const void* workspace, long long workspace_bytes,
                                     long long nr_pairs, int32_t* pairs, float* hit_t, int32_t* hit_slot, float* hit_uv,
                                     float* rays_d, float* stage_ms, void* stream) {
  RasterGrid g;
  SlotRanges r;
  MT_TRY(check_raster_args(tris, nr_slots, mesh_tri_offset, mesh_nr_tris, nr_meshes, c2w, intrinsics, intrinsics_inv,
                           height, width, supersample, t_min, workspace, &g, &r));
  if (!hit_t || !hit_slot || !hit_uv || nr_pairs < 0 || (nr_pairs > 0 && !pairs)) return VSA_ERR_ARG;
  if (nr_pairs > MAX_I32) return VSA_ERR_UNSUPPORTED;
  Layout L;
  MT_TRY(checked_layout(nr_slots, nr_meshes, g, workspace_bytes, &L));
  const hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(const_cast<void*>(workspace));   // (the cursors are this call's own)
  const size_t cells = (size_t)g.tiles * nr_meshes + 1;
  mt::StageTimer timer;
  MT_TRY(timer.create(stage_ms, 2, st));
  MT_TRY(timer.open());
  if (nr_pairs > 0) {
    VSA_HIP_TRY(hipMemsetAsync(ws + L.cursor, 0, 4 * cells, st));
    const dim3 grid((unsigned)vsa_div_up(max_count(r), SETUP_BLOCK), nr_meshes), block(SETUP_BLOCK);
    hipLaunchKernelGGL(raster_fill_kernel, grid, block, 0, st, r, g, mt::at<TileBox>(ws, L.boxes),
                       mt::at<int>(ws, L.tile_start), mt::at<int>(ws, L.cursor), nr_pairs, pairs);
    MT_LAUNCHED();
  }
  MT_TRY(timer.close(0));
  MT_TRY(timer.open());
  const long long nr_samples = (long long)g.samples_h * g.samples_w;
  const dim3 grid((unsigned)g.tiles, nr_meshes), block(TRACE_BLOCK);
  with_flag(rays_d != nullptr, [&](auto dirs) {
    hipLaunchKernelGGL((raster_kernel<decltype(dirs)::value>), grid, block, 0, st, reinterpret_cast<const float4*>(tris),
                       nr_slots, r, c2w, intrinsics_inv, g, mt::at<int>(ws, L.tile_start), nr_pairs, pairs,
                       mt::at<int>(ws, L.strad_list), mt::at<int>(ws, L.strad_count), t_min, nr_samples, hit_t, hit_slot,
                       hit_uv, rays_d);
  });
  MT_LAUNCHED();
  MT_TRY(timer.close(1));
  timer.destroy();
  return VSA_OK;
}
