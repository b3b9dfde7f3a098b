// Per-ray building blocks of the packed (ragged) sample kernels: packed.hip and the fused sweeps
// of ray_sweep.h include this one copy, so that a fused kernel performs exactly the fp32
// operations, in exactly the order, of the single-op kernel it replaces.
//
// Layout: a ray is owned by a 32-lane half-wave, lanes = consecutive samples (coalesced rows),
// segmented scans / reductions by shuffles, chunks of 32 samples with a carried running value for
// longer rays.  The build has -ffp-contract=off.
#pragma once
#include "common.h"

// The half-wave of a BLOCK-thread block that owns ray `ray`: lane l, the ray's samples [i0, i1)
#define VSA_RAY_PROLOGUE(BLOCK)                                                  \
  const int l = threadIdx.x & (vsa_ray::SUB - 1);                                \
  const long long ray = ((long long)blockIdx.x * (BLOCK) + threadIdx.x) / vsa_ray::SUB; \
  if (ray >= N) return;                                                          \
  const int i0 = start_end[2 * ray], i1 = start_end[2 * ray + 1];                \
  const int n = i1 - i0;

namespace vsa_ray {

constexpr int SUB = 32;  // lanes per ray

// inclusive shuffle scans / butterfly reduction over the 32 lanes (fixed partner order -> fixed bits)
__device__ __forceinline__ float sub_scan_mul(float v, int l) {
#pragma unroll
  for (int off = 1; off < SUB; off <<= 1) {
    const float u = __shfl_up(v, off, SUB);
    if (l >= off) v *= u;
  }
  return v;
}
__device__ __forceinline__ float sub_scan_add(float v, int l) {
#pragma unroll
  for (int off = 1; off < SUB; off <<= 1) {
    const float u = __shfl_up(v, off, SUB);
    if (l >= off) v += u;
  }
  return v;
}
__device__ __forceinline__ float sub_reduce_add(float v) {
#pragma unroll
  for (int off = SUB / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, SUB);
  return v;
}

// One chunk step of T = cumprod(a1) (exclusive, carried across chunks) for the sample of lane l,
// as cumprod_fwd_kernel computes it; returns T and advances `carry`.  a1 = (1 - alpha) + 1e-6 in
// the render chains; lanes past the ray's end pass in = false.
__device__ __forceinline__ float transmittance_step(float a1, bool in, int l, float& carry) {
  const float incl = sub_scan_mul(in ? a1 : 1.0f, l);
  float excl = __shfl_up(incl, 1, SUB);
  if (l == 0) excl = 1.0f;
  const float T = carry * excl;
  carry *= __shfl(incl, SUB - 1, SUB);
  return T;
}

// integrate_bwd_kernel<3>'s weight gradient of one sample: (g_0 v_0 + g_1 v_1) + g_2 v_c with
// c = 1 under bug_compat (VolumeRenderingGPU.cuh:1021), else 2.
__device__ __forceinline__ float integrate3_grad_w(const float g[3], const float* v, int bug_compat) {
  float gw = 0.f;
#pragma unroll
  for (int d = 0; d < 3; ++d) gw += g[d] * v[(bug_compat && d == 2) ? 1 : d];
  return gw;
}

// One chunk step of the backward of T = cumprod(a1) over the REVERSED ray (lane l holds the
// sample n - 1 - (c + l)): the suffix sums of lv in cumsum_kernel(inverse)'s order, carried in
// `csum`; returns the suffix sum of the samples after this one (cumsumLV[i + 1] of
// cumprod_bwd_kernel; the caller drops it for the ray's last sample).
__device__ __forceinline__ float cumprod_bwd_suffix_step(float lv, bool in, int l, float& csum) {
  const float incl = sub_scan_add(in ? lv : 0.0f, l);
  const float cs = csum + incl;
  float cs_next = __shfl_up(cs, 1, SUB);
  if (l == 0) cs_next = csum;
  csum += __shfl(incl, SUB - 1, SUB);
  return cs_next;
}

// VolumeRenderingGPU.cuh:185-244: the NeuS alpha of sample i from the SDF at i and i + 1.  The
// reference mixes float variables with double literals, so several intermediate results are formed
// in double and rounded to float on assignment; reproduced operation by operation.
__device__ __forceinline__ float sigmoid_ref(float x) {   // :179-183: float res = 1.0 / (1.0 + exp(-x))
  return (float)(1.0 / (1.0 + (double)expf(-x)));
}
__device__ __forceinline__ float sdf2alpha_sample(float prev, float next, float d, float b) {
  const float mid = (float)((double)(prev + next) * 0.5);
  float cosv = (float)((double)(next - prev) / ((double)d + 1e-6));
  cosv = fminf(fmaxf(cosv, -1e3f), 0.0f);
  const float prev_esti = (float)((double)mid - (double)(cosv * d) * 0.5);
  const float next_esti = (float)((double)mid + (double)(cosv * d) * 0.5);
  const float prev_cdf = sigmoid_ref(prev_esti * b), next_cdf = sigmoid_ref(next_esti * b);
  return (float)(((double)(prev_cdf - next_cdf) + 1e-6) / ((double)prev_cdf + 1e-6));
}

}  // namespace vsa_ray
