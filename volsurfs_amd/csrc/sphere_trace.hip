// Sphere tracing (utils/sphere_tracing.py:112-152): the round bookkeeping around an SDF that stays a Python
// callable (encoder + MLP launches).  An ITEM is one (ray, column) pair, item = slot * N + ray: one slot for a
// single SDF, K slots for K offset surfaces; each slot reads its own column of the [rows, C] SDF block.
//
// Per round the host evaluates the SDF on the DENSE point rows of the live items and calls vsa_st_step:
//   st_step_kernel     live row j -> its item: advance the point, set the flags, keep[j] = still live; a
//                      block's survivors are counted into block_counts[b]
//   st_compact_kernel  ORDERED compaction of the survivors (ascending item index): a block's offset is the sum
//                      of the counts of the blocks before it (an integer sum, so every block finds the same
//                      values whatever the order blocks run in), a wave's from an LDS scan of the 4 wave totals,
//                      a lane's from ballot + popcount.  Writes the next round's live list, dense point rows and
//                      live count.  No atomics: two runs give the same bytes.
// Rows from the live count up to the launch bound (the host launches with an OLD count, which is an upper
// bound: the count never grows) carry a copy of the same row of the round before, a point that was live once;
// their SDF is never read.
//
// fp32, no contraction (-ffp-contract=off), the reference's order: p += d * (sdf * multiplier);
// newly = |sdf| < thresh; hit |= newly; done |= newly; done |= !inside(p).
#include "common.h"

namespace {

constexpr int ST_BLOCK = 256;
constexpr int ST_WAVES = ST_BLOCK / VSA_WAVE;
constexpr unsigned char ST_HIT = 1, ST_DONE = 2;

// background.BoundingBox / BoundingSphere .check_points_inside (closed), kind as in vsa_intersect_primitive
__device__ __forceinline__ bool st_inside(int kind, float size, float x, float y, float z) {
  if (kind == 0) return fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z)) <= size;
  return sqrtf((x * x + y * y) + z * z) <= size;
}

// keep -> this block's count (thread 0 writes it)
__device__ __forceinline__ void st_block_count(bool keep, int32_t* __restrict__ block_counts) {
  __shared__ int wave_total[ST_WAVES];
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & (VSA_WAVE - 1)) == 0) wave_total[threadIdx.x / VSA_WAVE] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < ST_WAVES; ++w) t += wave_total[w];
    block_counts[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(ST_BLOCK)
st_begin_kernel(const float* __restrict__ points_near, int N, long long M, float* __restrict__ pts,
                unsigned char* __restrict__ flags, int32_t* __restrict__ live, float* __restrict__ dense,
                int32_t* __restrict__ count) {
  const long long i = (long long)blockIdx.x * ST_BLOCK + threadIdx.x;
  if (i == 0) *count = (int32_t)M;
  if (i >= M) return;
  const long long ray = i % N;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = points_near[3 * ray + c];
    pts[3 * i + c] = v;
    dense[3 * i + c] = v;
  }
  flags[i] = 0;
  live[i] = (int32_t)i;
}

__global__ void __launch_bounds__(ST_BLOCK)
st_step_kernel(const int32_t* __restrict__ live_in, const int32_t* __restrict__ count_in,
               const float* __restrict__ sdf, int C, const int32_t* __restrict__ slot_cols, int N,
               const float* __restrict__ rays_d, float multiplier, float thresh, int kind, float size,
               float* __restrict__ pts, unsigned char* __restrict__ flags, unsigned char* __restrict__ keep,
               int32_t* __restrict__ block_counts, int bound) {
  const int j = blockIdx.x * ST_BLOCK + threadIdx.x;
  const int count = *count_in;          // <= bound (the host's bound is an older count)
  bool alive = false;
  if (j < count && j < bound) {
    const int item = live_in[j];
    const int slot = item / N, ray = item - slot * N;
    const float s = sdf[(long long)j * C + slot_cols[slot]];
    const float step = s * multiplier;
    const float x = pts[3ll * item] + rays_d[3ll * ray] * step;
    const float y = pts[3ll * item + 1] + rays_d[3ll * ray + 1] * step;
    const float z = pts[3ll * item + 2] + rays_d[3ll * ray + 2] * step;
    pts[3ll * item] = x;
    pts[3ll * item + 1] = y;
    pts[3ll * item + 2] = z;
    unsigned char f = flags[item];
    if (fabsf(s) < thresh) f |= ST_HIT | ST_DONE;
    if (!st_inside(kind, size, x, y, z)) f |= ST_DONE;
    flags[item] = f;
    alive = !(f & ST_DONE);
  }
  if (j < bound) keep[j] = alive ? 1 : 0;
  st_block_count(alive, block_counts);
}

// Per item: z = ||p - o||, the hit flag (unconverged items too when asked), keep = hit.
__global__ void __launch_bounds__(ST_BLOCK)
st_finish_kernel(const float* __restrict__ pts, const float* __restrict__ rays_o, int N, int M,
                 const unsigned char* __restrict__ flags, int unconverged_are_hits, float* __restrict__ z,
                 unsigned char* __restrict__ hit, unsigned char* __restrict__ keep,
                 int32_t* __restrict__ block_counts) {
  const int i = blockIdx.x * ST_BLOCK + threadIdx.x;
  bool h = false;
  if (i < M) {
    const int ray = i % N;
    const float dx = pts[3ll * i] - rays_o[3ll * ray];
    const float dy = pts[3ll * i + 1] - rays_o[3ll * ray + 1];
    const float dz = pts[3ll * i + 2] - rays_o[3ll * ray + 2];
    z[i] = sqrtf((dx * dx + dy * dy) + dz * dz);
    const unsigned char f = flags[i];
    h = (f & ST_HIT) || (unconverged_are_hits && !(f & ST_DONE));
    hit[i] = h ? 1 : 0;
    keep[i] = h ? 1 : 0;
  }
  st_block_count(h, block_counts);
}

// Ordered compaction of the rows j < bound with keep[j]: ids_out[rank] = ids_in[j] (j itself without
// ids_in), dense_out[rank] = pts[that item] (when given), *count_out = the total.  Rows total <= j < bound of
// dense_out take dense_in's row j.  The grid is the one that wrote keep / block_counts.
__global__ void __launch_bounds__(ST_BLOCK)
st_compact_kernel(const unsigned char* __restrict__ keep, const int32_t* __restrict__ ids_in,
                  const int32_t* __restrict__ block_counts, const float* __restrict__ pts,
                  const float* __restrict__ dense_in, int32_t* __restrict__ ids_out,
                  float* __restrict__ dense_out, int32_t* __restrict__ count_out, int bound) {
  __shared__ int red[2][ST_WAVES];
  __shared__ int wave_total[ST_WAVES];
  const int lane = threadIdx.x & (VSA_WAVE - 1), wave = threadIdx.x / VSA_WAVE;
  // this block's offset and the total: integer sums of the per-block counts
  int before = 0, all = 0;
  for (int b = threadIdx.x; b < (int)gridDim.x; b += ST_BLOCK) {
    const int c = block_counts[b];
    all += c;
    if (b < (int)blockIdx.x) before += c;
  }
#pragma unroll
  for (int off = VSA_WAVE / 2; off > 0; off >>= 1) {
    before += __shfl_xor(before, off);
    all += __shfl_xor(all, off);
  }
  if (lane == 0) red[0][wave] = before, red[1][wave] = all;
  const int j = blockIdx.x * ST_BLOCK + threadIdx.x;
  const bool k = j < bound && keep[j];
  const unsigned long long m = __ballot(k);
  if (lane == 0) wave_total[wave] = __popcll(m);
  __syncthreads();
  int offset = 0, total = 0, wave_off = 0;
#pragma unroll
  for (int w = 0; w < ST_WAVES; ++w) {
    offset += red[0][w];
    total += red[1][w];
    if (w < wave) wave_off += wave_total[w];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *count_out = total;
  if (k) {
    const int dst = offset + wave_off + __popcll(m & ((1ull << lane) - 1ull));
    const int item = ids_in ? ids_in[j] : j;
    ids_out[dst] = item;
    if (dense_out) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dense_out[3ll * dst + c] = pts[3ll * item + c];
    }
  }
  if (dense_out && j >= total && j < bound) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dense_out[3ll * j + c] = dense_in[3ll * j + c];
  }
}

// dst[(item % N) * S + item / N, :] = src[h, :] for the first H entries of `ids`
__global__ void __launch_bounds__(ST_BLOCK)
st_scatter_kernel(const int32_t* __restrict__ ids, long long H, const float* __restrict__ src, int C, int N,
                  int S, float* __restrict__ dst) {
  const long long t = (long long)blockIdx.x * ST_BLOCK + threadIdx.x;
  if (t >= H * C) return;
  const long long h = t / C;
  const int c = (int)(t - h * C);
  const int item = ids[h];
  const int slot = item / N, ray = item - slot * N;
  dst[((long long)ray * S + slot) * C + c] = src[t];
}

// methods/offsets_surfs.py:810-858, one thread per ray, bit for bit what the torch expression gives on the
// device: the K products taken one after the other from the outer shell (k = K - 1) inwards, which is cumprod's
// order over the flipped alphas, and the sum over the surfaces as torch's reduction takes it: term j (outer
// shell first) into partial sum j mod 4, the four partial sums added in order at the end.
__global__ void __launch_bounds__(ST_BLOCK)
st_blend_kernel(const float* __restrict__ surfs_rgb, const float* __restrict__ surfs_alpha, int N, int K,
                float* __restrict__ transmittance, float* __restrict__ weights, float* __restrict__ rgb_fg,
                float* __restrict__ bg_transmittance) {
  const int n = blockIdx.x * ST_BLOCK + threadIdx.x;
  if (n >= N) return;
  float T = 1.0f, acc[4][3];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 0.0f;
  for (int k0 = K - 1; k0 >= 0; k0 -= 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 - q;
      if (k < 0) break;
      const long long r = (long long)n * K + k;
      const float a = surfs_alpha[r];
      const float w = T * a;
      transmittance[r] = T;
      weights[r] = w;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[q][c] = acc[q][c] + surfs_rgb[3 * r + c] * w;
      T = T * (1.0f - a);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb_fg[3ll * n + c] = ((acc[0][c] + acc[1][c]) + acc[2][c]) + acc[3][c];
  bg_transmittance[n] = T;
}

}  // namespace

extern "C" int vsa_st_begin(const float* points_near, int nr_rays, int nr_slots, float* pts, uint8_t* flags,
                            int32_t* live, float* dense, int32_t* count, void* stream) {
  if (nr_rays < 1 || nr_slots < 1 || (long long)nr_rays * nr_slots > 0x7FFFFFFFll - ST_BLOCK) return VSA_ERR_ARG;
  if (!points_near || !pts || !flags || !live || !dense || !count) return VSA_ERR_ARG;
  const long long M = (long long)nr_rays * nr_slots;
  hipLaunchKernelGGL(st_begin_kernel, dim3(vsa_div_up(M, ST_BLOCK)), dim3(ST_BLOCK), 0, (hipStream_t)stream,
                     points_near, nr_rays, M, pts, flags, live, dense, count);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_st_step(const int32_t* live_in, const int32_t* count_in, const float* sdf, int nr_columns,
                           const int32_t* slot_cols, int nr_rays, const float* rays_d, float sdf_multiplier,
                           float thresh, int kind, float size, float* pts, uint8_t* flags, uint8_t* keep,
                           int32_t* block_counts, const float* dense_in, int32_t* live_out, float* dense_out,
                           int32_t* count_out, int bound, void* stream) {
  if (bound < 0 || nr_columns < 1 || nr_rays < 1 || (kind != 0 && kind != 1) || !(size > 0.0f)) return VSA_ERR_ARG;
  if (bound == 0) return VSA_OK;
  if (!live_in || !count_in || !sdf || !slot_cols || !rays_d || !pts || !flags || !keep || !block_counts ||
      !dense_in || !live_out || !dense_out || !count_out || live_in == live_out || dense_in == dense_out)
    return VSA_ERR_ARG;
  const dim3 grid(vsa_div_up(bound, ST_BLOCK));
  hipLaunchKernelGGL(st_step_kernel, grid, dim3(ST_BLOCK), 0, (hipStream_t)stream, live_in, count_in, sdf,
                     nr_columns, slot_cols, nr_rays, rays_d, sdf_multiplier, thresh, kind, size, pts, flags, keep,
                     block_counts, bound);
  hipLaunchKernelGGL(st_compact_kernel, grid, dim3(ST_BLOCK), 0, (hipStream_t)stream, keep, live_in, block_counts,
                     pts, dense_in, live_out, dense_out, count_out, bound);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_st_finish(const float* pts, const float* rays_o, int nr_rays, int nr_slots, const uint8_t* flags,
                             int unconverged_are_hits, float* z, uint8_t* hit, uint8_t* keep, int32_t* block_counts,
                             int32_t* hit_list, int32_t* hit_count, void* stream) {
  if (nr_rays < 1 || nr_slots < 1 || (long long)nr_rays * nr_slots > 0x7FFFFFFFll - ST_BLOCK) return VSA_ERR_ARG;
  if (!pts || !rays_o || !flags || !z || !hit || !keep || !block_counts || !hit_list || !hit_count)
    return VSA_ERR_ARG;
  const int M = nr_rays * nr_slots;
  const dim3 grid(vsa_div_up(M, ST_BLOCK));
  hipLaunchKernelGGL(st_finish_kernel, grid, dim3(ST_BLOCK), 0, (hipStream_t)stream, pts, rays_o, nr_rays, M, flags,
                     unconverged_are_hits, z, hit, keep, block_counts);
  hipLaunchKernelGGL(st_compact_kernel, grid, dim3(ST_BLOCK), 0, (hipStream_t)stream, keep, (const int32_t*)nullptr,
                     block_counts, (const float*)nullptr, (const float*)nullptr, hit_list, (float*)nullptr,
                     hit_count, M);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_st_scatter(const int32_t* ids, long long nr_ids, const float* src, int nr_channels, int nr_rays,
                              int nr_slots, float* dst, void* stream) {
  if (nr_ids < 0 || nr_channels < 1 || nr_rays < 1 || nr_slots < 1 ||
      nr_ids > (long long)nr_rays * nr_slots || nr_ids * nr_channels > 0x7FFFFFFFll * ST_BLOCK)
    return VSA_ERR_ARG;
  if (nr_ids == 0) return VSA_OK;
  if (!ids || !src || !dst) return VSA_ERR_ARG;
  hipLaunchKernelGGL(st_scatter_kernel, dim3(vsa_div_up(nr_ids * nr_channels, ST_BLOCK)), dim3(ST_BLOCK), 0,
                     (hipStream_t)stream, ids, nr_ids, src, nr_channels, nr_rays, nr_slots, dst);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_st_blend(const float* surfs_rgb, const float* surfs_alpha, int nr_rays, int nr_surfs,
                            float* surfs_transmittance, float* surfs_blending_weights, float* rgb_fg,
                            float* bg_transmittance, void* stream) {
  if (nr_rays < 0 || nr_surfs < 1) return VSA_ERR_ARG;
  if (nr_rays == 0) return VSA_OK;
  if (!surfs_rgb || !surfs_alpha || !surfs_transmittance || !surfs_blending_weights || !rgb_fg || !bg_transmittance)
    return VSA_ERR_ARG;
  hipLaunchKernelGGL(st_blend_kernel, dim3(vsa_div_up(nr_rays, ST_BLOCK)), dim3(ST_BLOCK), 0, (hipStream_t)stream,
                     surfs_rgb, surfs_alpha, nr_rays, nr_surfs, surfs_transmittance, surfs_blending_weights, rgb_fg,
                     bg_transmittance);
  VSA_RETURN_LAUNCH_STATUS();
}
