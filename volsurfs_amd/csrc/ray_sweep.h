// The per-ray sweeps that the three field methods' fused kernels share (nerf_render.hip,
// surf_render.hip, offsets_render.hip), written once on the building blocks of ray_scan.h.
//
// Layout: a ray is owned by a 32-lane half-wave, lanes = consecutive samples (coalesced rows),
// segmented scans / reductions by shuffles, chunks of 32 samples with a carried running value for
// longer rays.  No atomics: every output element has exactly one writer, so the output bits depend
// only on the inputs.  The build has -ffp-contract=off, so every fp32 operation below is a single
// rounding, in the order written: the scans and reductions are the ones of packed.hip's cumprod /
// cumsum / integrate / sum_over_rays / compute_cdf kernels, which makes the fused kernels
// bit-identical to the chains of single ops (tests/test_nerf_render.py, test_surf_render.py,
// test_offsets_surfs_render.py).
//
// What differs between the methods comes in as callables.  `alpha_of(s, i)` gives the alpha of
// sample s, the i-th of its ray, as a float or as a record that alpha_value() reads (the record
// travels on to the caller's own code, e.g. NeusAlpha to neus_alpha_bwd).  Every lane calls it; a
// lane past the ray's end (i >= n) gets s = i0 and its alpha is not used.
#pragma once
#include "ray_scan.h"

// One block size, one grid, one prologue, one argument check and one launch for the per-ray kernels
#define RAY_PROLOGUE() VSA_RAY_PROLOGUE(vsa_ray::RAY_BLOCK)
#define RAY_CHECK(cond) \
  if (!(cond)) return VSA_ERR_ARG
#define RAY_LAUNCH(kernel, N, ...)                                                      \
  if ((N) == 0) return VSA_OK;                                                          \
  hipLaunchKernelGGL(kernel, vsa_ray::ray_grid(N), dim3(vsa_ray::RAY_BLOCK), 0,         \
                     (hipStream_t)stream, __VA_ARGS__);                                 \
  VSA_RETURN_LAUNCH_STATUS()

namespace vsa_ray {

constexpr int RAY_BLOCK = 256;
inline dim3 ray_grid(int N) { return dim3(vsa_div_up((long long)N * SUB, RAY_BLOCK)); }

__device__ __forceinline__ float alpha_value(float alpha) { return alpha; }

// The forward weight sweep over the ray's samples [i0, i0 + n): per chunk of 32 samples
//   a1 = (1 - alpha) + 1e-6;  T = cumprod(a1) (exclusive: transmittance_step);  w = alpha T
// (compute_transmittance_from_alphas, weights = alpha * transmittance), then
// body(s, in, a, T, w) on every lane, in = false past the ray's end.  The caller accumulates what
// it wants there; the per-ray weight sum in sum_over_rays_kernel<1>'s order is
//   ws += sub_reduce_add(in ? w : 0)   (the butterfly sum of each chunk, chunk after chunk).
template <class AlphaOf, class Body>
__device__ __forceinline__ void for_each_weight(int n, int l, int i0, AlphaOf alpha_of, Body body) {
  float carry = 1.0f;
  for (int c = 0; c < n; c += SUB) {
    const int i = c + l;
    const bool in = i < n;
    const long long s = i0 + (in ? i : 0);
    const auto a = alpha_of(s, i);
    const float alpha = alpha_value(a);
    const float a1 = (1.0f - alpha) + 1e-6f;
    const float T = transmittance_step(a1, in, l, carry);
    body(s, in, a, T, alpha * T);
  }
}

// The background's part of a composite backward.  With g_d = g_rgb_d of the ray:
//   g_bgT = (g_0 bg_0 + g_1 bg_1) + g_2 bg_2   (returned; 0 without a background),
//   g_bg_d = g_d bgT                           (lane 0 writes it when g_rgb_bg is given),
// bgT = bgT_of(), the forward's background transmittance, read only where it is written out.
template <class BgT>
__device__ __forceinline__ float bg_grad(const float g[3], const float* rgb_bg, int bg_stride,
                                         long long ray, int l, float* g_rgb_bg, BgT bgT_of) {
  if (!rgb_bg) return 0.0f;
  const float* b = rgb_bg + ray * bg_stride;
  float g_bgT = g[0] * b[0];
  g_bgT += g[1] * b[1];
  g_bgT += g[2] * b[2];
  if (g_rgb_bg && l == 0) {
    const float bgT = bgT_of();
#pragma unroll
    for (int d = 0; d < 3; ++d) g_rgb_bg[ray * 3 + d] = g[d] * bgT;
  }
  return g_bgT;
}

// The gradient of a ray's weight sum where rgb = rgb_fg + (1 - wsum) bg:
//   g_wsum = g_wsum_in + (-g_bgT)   (g_wsum_in = 0 without the mask term, no -g_bgT without a
//                                    background: sum_over_rays_bwd_kernel's per-ray gradient).
__device__ __forceinline__ float wsum_grad(const float* g_wsum_in, long long ray, bool has_bg,
                                           float g_bgT) {
  const float g_ws = g_wsum_in ? g_wsum_in[ray] : 0.0f;
  if (!has_bg) return g_ws;
  return g_wsum_in ? g_ws + (-g_bgT) : -g_bgT;
}

// The composite backward of one field: column k of per-sample arrays [S, K] (K = 1, k = 0 for a
// method with one field), in two sweeps over the ray.  scratch: 2 floats per sample and column.
//
// Forward sweep (alpha and T recomputed as in the forward kernel).  Per sample
//   g_w   = (g_0 rgb_0 + g_1 rgb_1) + g_2 rgb_c   (c = 1 under bug_compat, else 2: integrate_bwd_kernel<3>)
//           + g_w_rest(s, a, w)                    (the weight's other uses: the per-ray gradient of
//                                                   the weight sum, a second integral)
//   g_rgb_sample_d = g_d w;  lv = (g_w alpha) T -> scratch[2 sk];  g_w T -> scratch[2 sk + 1].
template <class AlphaOf, class GradWRest>
__device__ __forceinline__ void composite_bwd_weights(int n, int l, int i0, int K, int k,
                                                      AlphaOf alpha_of, const float g[3],
                                                      const float* rgb, int bug_compat,
                                                      GradWRest g_w_rest, float* g_rgb_samples,
                                                      float* scratch) {
  for_each_weight(n, l, i0, alpha_of, [&](long long s, bool in, const auto& a, float T, float w) {
    if (!in) return;
    const long long sk = s * K + k;
#pragma unroll
    for (int d = 0; d < 3; ++d) g_rgb_samples[sk * 3 + d] = g[d] * w;
    const float gw = integrate3_grad_w(g, rgb + sk * 3, bug_compat) + g_w_rest(s, a, w);
    const float gT = gw * alpha_value(a);
    scratch[2 * sk] = gT * T;
    scratch[2 * sk + 1] = gw * T;
  });
}

// Reversed sweep (lane l of chunk c holds the sample n - 1 - (c + l)): the suffix sums of lv in
// cumsum_kernel(inverse)'s order, the cumprod backward (next suffix sum / max(a1, 1e-6), 0 for the
// ray's last sample), then
//   g_alpha = g_w T + (-g_a1)
// handed to alpha_bwd(s, a, g_alpha), the method's backward of its alpha.
template <class AlphaOf, class AlphaBwd>
__device__ __forceinline__ void composite_bwd_alphas(int n, int l, int i0, int i1, int K, int k,
                                                     AlphaOf alpha_of, const float* scratch,
                                                     AlphaBwd alpha_bwd) {
  float csum = 0.0f;
  for (int c = 0; c < n; c += SUB) {
    const int i = c + l;
    const bool in = i < n;
    const long long s = in ? (long long)i1 - 1 - i : (long long)i0;
    const long long sk = s * K + k;
    const float cs_next = cumprod_bwd_suffix_step(in ? scratch[2 * sk] : 0.0f, in, l, csum);
    if (in) {
      const auto a = alpha_of(s, n - 1 - i);
      const float a1 = (1.0f - alpha_value(a)) + 1e-6f;
      float ga1 = 0.f;
      if (i > 0) ga1 = cs_next / fmaxf(a1, 1e-6f);
      const float g_alpha = scratch[2 * sk + 1] + (-ga1);
      alpha_bwd(s, a, g_alpha);
    }
  }
}

// The tail of a coarse CDF (compute_cdf_kernel) in three pieces.  Rays with fewer than 2 samples
// get a zero CDF (compute_cdf leaves them at zero); true when the ray was such a one.
__device__ __forceinline__ bool cdf_of_short_ray(int n, int l, int i0, float* cdf) {
  if (n == 1 && l == 0) cdf[i0] = 0.0f;
  return n < 2;
}
// One chunk step of the exclusive scan of the normalised weights x:
//   cdf_i = run + (incl_i - x_i) with incl the chunk's inclusive shuffle scan; advances `run`.
__device__ __forceinline__ float cdf_scan_step(float x, int l, float& run) {
  const float incl = sub_scan_add(x, l);
  const float excl = run + (incl - x);
  run += __shfl(incl, SUB - 1, SUB);
  return excl;
}
// The last entry is snapped to 1 when |wsum' - 1| < 1e-3 and |cdf_last - 1| > 1e-3 (wsum' = run
// after the last chunk, the sum of the normalised weights).
__device__ __forceinline__ bool cdf_snaps_last(float run, float last_cdf) {
  return fabs((double)run - 1.0) < 1e-3 && fabs((double)last_cdf - 1.0) > 1e-3;
}

// The coarse pass of importance sampling from the samples' alphas to the CDF of one ray:
//   T = cumprod((1 - alpha) + 1e-6);  w = alpha T;
//   wsum  = sum over chunks of the butterfly sum of the chunk (sum_over_rays_kernel<1>);
//   w    /= max(wsum, 1e-6);
//   cdf   = the exclusive scan of w with its last entry snapped (above).
// The first sweep parks w in `cdf` (each lane re-reads only what it wrote).
template <class AlphaOf>
__device__ __forceinline__ void coarse_cdf(int n, int l, int i0, int i1, AlphaOf alpha_of,
                                           float* cdf) {
  if (cdf_of_short_ray(n, l, i0, cdf)) return;
  float ws = 0.f;
  for_each_weight(n, l, i0, alpha_of, [&](long long s, bool in, const auto&, float, float w) {
    if (in) cdf[s] = w;
    ws += sub_reduce_add(in ? w : 0.f);
  });
  const float wn = fmaxf(ws, 1e-6f);
  float run = 0.0f, last_cdf = 0.0f;
  for (int c = 0; c < n; c += SUB) {
    const int i = c + l;
    const float excl = cdf_scan_step(i < n ? cdf[i0 + i] / wn : 0.0f, l, run);
    if (i < n) cdf[i0 + i] = excl;
    if (i == n - 1) last_cdf = excl;
  }
  const int owner = (n - 1) & (SUB - 1);
  if (l == owner && cdf_snaps_last(run, last_cdf)) cdf[i1 - 1] = 1.0f;
}

}  // namespace vsa_ray
