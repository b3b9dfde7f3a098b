// How far is one mesh from another?  (The reference has no such stage: the rule is this library's own —
// include/volsurfs_hip.h "Mesh distance", DESIGN §27: restated in tests/mesh_distance_restated.py, unpinned.)
//
// vsa_closest_point_q: N points x K shells -> distance, triangle slot and barycentric weights of the closest point of
// each shell, by the closest-point walk of the q16 nodes (closest_walk.h), one query per lane, one launch (grid.y =
// mesh).  The result is that of brute force over every triangle record, bit for bit.
// vsa_surface_area_prefix / vsa_surface_sample: an area-weighted, stratified sampler of the leaf-ordered records with
// integer weights (an exact prefix, whatever the scan's shape).
// vsa_surface_distance: the two fused.  A wave makes 64 samples of the source shell in registers, walks the
// destination shell and reduces: no sample and no per-sample distance reaches memory.  min / max / counts by integer
// atomics, the sums as one fp64 pair per wave added in a fixed order: exact or fixed-order, the same for every schedule.
#include "closest_walk.h"
#include "mesh_topology.h"
#include "ordered_sum.h"

namespace {

template <int STACK, bool BOUNDS, bool COUNT>
__global__ __launch_bounds__(TRACE_BLOCK) void closest_point_kernel(
    const uint4* __restrict__ qnodes, const float4* __restrict__ tris, Roots roots, Frames frames,
    const float* __restrict__ points, long long nr_points, float* __restrict__ dist, int* __restrict__ slot,
    float* __restrict__ bary, unsigned long long* __restrict__ counters) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  __shared__ float s_bound[BOUNDS ? STACK : 1][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const int mesh = blockIdx.y;
  const long long i = (long long)blockIdx.x * TRACE_BLOCK + lane;
  const bool alive = i < nr_points;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (alive) px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
  const QPoint q = closest_qpoint(frames.f[mesh], px, py, pz);
  Closest best = no_closest();
  int visits = 0, tests = 0;
  closest_walk<STACK, BOUNDS, COUNT>(qnodes, tris, q, px, py, pz, alive ? roots.root[mesh] : TRACE_EMPTY, best, s_node, s_bound,
                             lane, &visits, &tests);
  if constexpr (COUNT) {
    atomicAdd(&counters[0], (unsigned long long)visits);
    atomicAdd(&counters[1], (unsigned long long)tests);
    if (alive) atomicAdd(&counters[2], 1ull);
    return;
  }
  if (!alive) return;
  const long long o = (long long)mesh * nr_points + i;
  dist[o] = sqrtf(best.d2);
  slot[o] = best.slot;
  if (bary) {
    bary[2 * o] = best.u;
    bary[2 * o + 1] = best.v;
  }
}

// ---- sampler

// The largest finite fp64 area of the records, as the bits of the (non-negative) double: an integer maximum.
__global__ __launch_bounds__(MT_BLOCK) void area_max_kernel(const float4* __restrict__ tris, long long first_slot,
                                                            long long nr_slots, unsigned long long* __restrict__ amax) {
  const long long i = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= nr_slots) return;
  const long long s = first_slot + i;
  const double a = record_area(tris[3 * s + 1], tris[3 * s + 2]);
  // (the word only grows: a lane that does not exceed the value it reads, however stale, has nothing to add -- without
  // the check every record's atomic queues on the one word)
  const unsigned long long bits = (unsigned long long)__double_as_longlong(a);
  if (a > 0.0 && a < INFINITY && bits > __hip_atomic_load(amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(amax, bits);
}

// weight = floor(area 2^k), 2^k the power of two that puts the largest area into [2^30, 2^31): a step of at most
// 2^-30 of the largest area, a total below nr_slots 2^31.  No positive finite area at all: every record weighs 1.
__global__ __launch_bounds__(MT_BLOCK) void area_weight_kernel(const float4* __restrict__ tris, long long first_slot,
                                                               long long nr_slots,
                                                               const unsigned long long* __restrict__ amax,
                                                               long long* __restrict__ weight) {
  const long long i = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= nr_slots) return;
  const double largest = __longlong_as_double((long long)*amax);
  if (!(largest > 0.0)) {
    weight[i] = 1;
    return;
  }
  int e;
  (void)frexp(largest, &e);                       // largest = m 2^e, m in [0.5, 1)
  const long long s = first_slot + i;
  const double a = record_area(tris[3 * s + 1], tris[3 * s + 2]);
  weight[i] = (a > 0.0 && a < INFINITY) ? (long long)floor(ldexp(a, 31 - e)) : 0;
}

__global__ __launch_bounds__(MT_BLOCK) void surface_sample_kernel(const float4* __restrict__ tris, long long first_slot,
                                                                  long long nr_slots,
                                                                  const long long* __restrict__ prefix, long long n,
                                                                  unsigned long long seed, float* __restrict__ points,
                                                                  int* __restrict__ slot, float* __restrict__ bary) {
  const long long i = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const SurfaceSample s = surface_sample(tris, first_slot, nr_slots, prefix, i, n, seed);
  points[3 * i] = s.x, points[3 * i + 1] = s.y, points[3 * i + 2] = s.z;
  if (slot) slot[i] = s.slot;
  if (bary) bary[2 * i] = s.u, bary[2 * i + 1] = s.v;
}

// ---- fused

// stats: 12 64-bit words: the bits of min d and of max d (fp32, zero-extended), sum d and sum d^2 (fp64), within[8].
enum { ST_MIN = 0, ST_MAX = 1, ST_SUM = 2, ST_SUM2 = 3, ST_WITHIN = 4, ST_WORDS = 12 };

struct Thresholds {
  float tau[8];
};

__global__ void distance_init_kernel(unsigned long long* __restrict__ stats) {
  const int t = threadIdx.x;
  if (t < ST_WORDS) stats[t] = t == ST_MIN ? 0x7f800000ull : 0ull;
}

template <int STACK, bool BOUNDS>
__global__ __launch_bounds__(TRACE_BLOCK) void surface_distance_kernel(
    const float4* __restrict__ src_tris, long long src_first, long long src_slots,
    const long long* __restrict__ src_prefix, const uint4* __restrict__ qnodes, const float4* __restrict__ tris,
    Roots roots, Frames frames, long long n, unsigned long long seed, Thresholds th, int nr_thresholds,
    unsigned long long* __restrict__ stats, double* __restrict__ partials) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  __shared__ float s_bound[BOUNDS ? STACK : 1][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const long long i = (long long)blockIdx.x * TRACE_BLOCK + lane;
  const bool alive = i < n;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (alive) {
    const SurfaceSample s = surface_sample(src_tris, src_first, src_slots, src_prefix, i, n, seed);
    px = s.x, py = s.y, pz = s.z;
  }
  const QPoint q = closest_qpoint(frames.f[0], px, py, pz);
  Closest best = no_closest();
  closest_walk<STACK, BOUNDS>(qnodes, tris, q, px, py, pz, alive ? roots.root[0] : TRACE_EMPTY, best, s_node, s_bound, lane);
  const float d = sqrtf(best.d2);

  // the wave's minimum and maximum of the distance bits (d >= 0: the order of the bits is the order of the values)
  unsigned lo = alive ? __float_as_uint(d) : 0xffffffffu, hi = alive ? __float_as_uint(d) : 0u;
  double s1 = alive ? (double)d : 0.0, s2 = alive ? (double)d * (double)d : 0.0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {            // a fixed tree: the pair of a wave does not depend on the schedule
    lo = min(lo, (unsigned)__shfl_xor((int)lo, m));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, m));
    s1 += __shfl_xor(s1, m);
    s2 += __shfl_xor(s2, m);
  }
  for (int j = 0; j < nr_thresholds; ++j) {
    const unsigned long long in = __builtin_amdgcn_ballot_w64(alive && d <= th.tau[j]);
    if (lane == 0 && in) atomicAdd(&stats[ST_WITHIN + j], (unsigned long long)__builtin_popcountll(in));
  }
  if (lane == 0) {
    // (every wave's atomic on the same two words would queue at the L2: the words only ever move one way, so a wave
    // that does not improve on the value it reads -- however stale -- has nothing to add)
    if (lo < __hip_atomic_load(&stats[ST_MIN], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(&stats[ST_MIN], (unsigned long long)lo);
    if (hi > __hip_atomic_load(&stats[ST_MAX], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(&stats[ST_MAX], (unsigned long long)hi);
    partials[2 * (long long)blockIdx.x] = s1;
    partials[2 * (long long)blockIdx.x + 1] = s2;
  }
}

// The waves' fp64 pairs (sum of d, sum of d^2) added in ordered_sum.h's fixed order.
__global__ __launch_bounds__(ORDERED_SUM_BLOCK) void distance_sum_kernel(const double2* __restrict__ partials,
                                                                         long long nr_waves,
                                                                         unsigned long long* __restrict__ stats) {
  double total[2];
  if (!ordered_sum<2, 4>(reinterpret_cast<const double*>(partials), nr_waves, total)) return;
  stats[ST_SUM] = (unsigned long long)__double_as_longlong(total[0]);
  stats[ST_SUM2] = (unsigned long long)__double_as_longlong(total[1]);
}

// rocPRIM's temporary storage for the scan of n weights, after the weights [n] and the maximum (one aligned word)
int prefix_layout(long long n, size_t* o_weight, size_t* o_amax, size_t* o_tmp, size_t* tmp_bytes, size_t* total) {
  mt::TmpCounts c = {};
  c.iscan64 = (size_t)n;
  MT_TRY(mt::tmp_bytes(c, tmp_bytes));
  mt::Bump b;
  *o_weight = b.take(8 * (size_t)n);
  *o_amax = b.take(8);
  *o_tmp = b.take(*tmp_bytes);
  *total = b.o;
  return VSA_OK;
}

constexpr long long MAX_GRID = 0x7fffffffll;

// process-wide: does a stack entry carry its bound (vsa_closest_walk_config): 0 never, 1 with the 24-entry stack, 2 always
int& walk_mode() {
  static int mode = 1;
  return mode;
}

}  // namespace

bool closest_walk_bounds(int max_depth) { return walk_mode() == 2 || (walk_mode() == 1 && max_depth < 24); }

static int closest_point_launch(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                                const float* mesh_frames, int nr_meshes, int max_depth, const float* points,
                                long long nr_points, float* dist, int32_t* slot, float* bary, long long* counters,
                                void* stream) {
  if (const int rc = check_qtree(qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth, VSA_ERR_ARG)) return rc;
  if (!points || nr_points < 1) return VSA_ERR_ARG;
  if (counters ? false : (!dist || !slot)) return VSA_ERR_ARG;
  const long long waves = (nr_points + TRACE_BLOCK - 1) / TRACE_BLOCK;
  if (waves > MAX_GRID) return VSA_ERR_UNSUPPORTED;
  const QTree t = make_qtree(qnodes, tris, mesh_roots, mesh_frames, nr_meshes);
  const dim3 grid((unsigned)waves, nr_meshes), block(TRACE_BLOCK);
  unsigned long long* ct = reinterpret_cast<unsigned long long*>(counters);
  if (counters) VSA_HIP_TRY(hipMemsetAsync(counters, 0, 3 * sizeof(long long), (hipStream_t)stream));
  // (the stack never exceeds the tree depth: 24 entries for the usual shallow trees, as vsa_trace_q)
  with_stack(max_depth, [&](auto st) {
    with_flag(closest_walk_bounds(max_depth), [&](auto bd) {
      with_flag(counters != nullptr, [&](auto cn) {
        hipLaunchKernelGGL((closest_point_kernel<decltype(st)::value, decltype(bd)::value, decltype(cn)::value>), grid,
                           block, 0, (hipStream_t)stream, t.qnodes, t.tris, t.roots, t.frames, points, nr_points, dist,
                           slot, bary, ct);
      });
    });
  });
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_closest_walk_config(int keep_bounds) {
  if (keep_bounds < 0 || keep_bounds > 2) return VSA_ERR_ARG;
  walk_mode() = keep_bounds;
  return VSA_OK;
}

extern "C" int vsa_closest_point_q(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                                   const float* mesh_frames, int nr_meshes, int max_depth, const float* points,
                                   long long nr_points, float* dist, int32_t* slot, float* bary, void* stream) {
  return closest_point_launch(qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth, points, nr_points, dist,
                              slot, bary, nullptr, stream);
}

extern "C" int vsa_closest_point_q_stats(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                                         const float* mesh_frames, int nr_meshes, int max_depth, const float* points,
                                         long long nr_points, long long* counters, void* stream) {
  if (!counters) return VSA_ERR_ARG;
  return closest_point_launch(qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth, points, nr_points, nullptr,
                              nullptr, nullptr, counters, stream);
}

extern "C" long long vsa_surface_area_prefix_workspace_bytes(long long nr_slots) {
  if (nr_slots < 1) return VSA_ERR_ARG;
  if (nr_slots > 0x7fffffffll) return VSA_ERR_UNSUPPORTED;
  size_t ow, oa, ot, tb, total;
  const int rc = prefix_layout(nr_slots, &ow, &oa, &ot, &tb, &total);
  if (rc != VSA_OK) return mt::abi_status(rc);
  return (long long)total;
}

extern "C" int vsa_surface_area_prefix(const float* tris, long long first_slot, long long nr_slots, void* workspace,
                                       long long workspace_bytes, long long* area_prefix, void* stream) {
  if (!tris || !workspace || !area_prefix || first_slot < 0 || nr_slots < 1) return VSA_ERR_ARG;
  if (nr_slots > 0x7fffffffll || first_slot > 0x7fffffffll - nr_slots) return VSA_ERR_UNSUPPORTED;
  size_t ow, oa, ot, tb, total;
  MT_TRY(mt::abi_status(prefix_layout(nr_slots, &ow, &oa, &ot, &tb, &total)));
  if (workspace_bytes < (long long)total) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  long long* weight = mt::at<long long>(ws, ow);
  unsigned long long* amax = mt::at<unsigned long long>(ws, oa);
  const float4* tr = reinterpret_cast<const float4*>(tris);
  VSA_HIP_TRY(hipMemsetAsync(amax, 0, 8, st));
  hipLaunchKernelGGL(area_max_kernel, mt::grid(nr_slots), dim3(MT_BLOCK), 0, st, tr, first_slot, nr_slots, amax);
  MT_LAUNCHED();
  hipLaunchKernelGGL(area_weight_kernel, mt::grid(nr_slots), dim3(MT_BLOCK), 0, st, tr, first_slot, nr_slots, amax,
                     weight);
  MT_LAUNCHED();
  return mt::inclusive_scan({ws + ot, tb}, weight, area_prefix, (size_t)nr_slots, st);
}

extern "C" int vsa_surface_sample(const float* tris, long long first_slot, long long nr_slots,
                                  const long long* area_prefix, long long nr_samples, unsigned long long seed,
                                  float* points, int32_t* slot, float* bary, void* stream) {
  if (!tris || !area_prefix || !points || first_slot < 0 || nr_slots < 1 || nr_samples < 1) return VSA_ERR_ARG;
  if (nr_slots > 0x7fffffffll || first_slot > 0x7fffffffll - nr_slots || nr_samples > MAX_GRID * MT_BLOCK)
    return VSA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(surface_sample_kernel, mt::grid(nr_samples), dim3(MT_BLOCK), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(tris), first_slot, nr_slots, area_prefix, nr_samples, seed, points,
                     slot, bary);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_surface_distance(const float* src_tris, long long src_first_slot, long long src_nr_slots,
                                    const long long* src_area_prefix, const uint32_t* dst_qnodes, const float* dst_tris,
                                    int dst_root, const float* dst_frame, int dst_max_depth, long long nr_samples,
                                    unsigned long long seed, const float* thresholds, int nr_thresholds,
                                    unsigned long long* stats, double* partials, void* stream) {
  if (const int rc = check_qtree(dst_qnodes, dst_tris, &dst_root, dst_frame, 1, dst_max_depth, VSA_ERR_ARG)) return rc;
  if (!src_tris || !src_area_prefix || !stats || !partials) return VSA_ERR_ARG;
  if (src_first_slot < 0 || src_nr_slots < 1 || nr_samples < 1 || dst_root < 0) return VSA_ERR_ARG;
  if (nr_thresholds < 0 || nr_thresholds > 8 || (nr_thresholds > 0 && !thresholds)) return VSA_ERR_ARG;
  Thresholds th = {};
  for (int j = 0; j < nr_thresholds; ++j) {
    if (!(thresholds[j] >= 0.0f)) return VSA_ERR_ARG;      // negative or NaN
    th.tau[j] = thresholds[j];
  }
  const long long waves = (nr_samples + TRACE_BLOCK - 1) / TRACE_BLOCK;
  if (src_nr_slots > 0x7fffffffll || src_first_slot > 0x7fffffffll - src_nr_slots || waves > MAX_GRID)
    return VSA_ERR_UNSUPPORTED;
  const QTree t = make_qtree(dst_qnodes, dst_tris, &dst_root, dst_frame, 1);
  const hipStream_t st = (hipStream_t)stream;
  const float4* sr = reinterpret_cast<const float4*>(src_tris);
  hipLaunchKernelGGL(distance_init_kernel, dim3(1), dim3(64), 0, st, stats);
  with_stack(dst_max_depth, [&](auto sk) {
    with_flag(closest_walk_bounds(dst_max_depth), [&](auto bd) {
      hipLaunchKernelGGL((surface_distance_kernel<decltype(sk)::value, decltype(bd)::value>), dim3((unsigned)waves),
                         dim3(TRACE_BLOCK), 0, st, sr, src_first_slot, src_nr_slots, src_area_prefix, t.qnodes, t.tris,
                         t.roots, t.frames, nr_samples, seed, th, nr_thresholds, stats, partials);
    });
  });
  hipLaunchKernelGGL(distance_sum_kernel, dim3(1), dim3(ORDERED_SUM_BLOCK), 0, st, reinterpret_cast<const double2*>(partials), waves,
                     stats);
  VSA_RETURN_LAUNCH_STATUS();
}
