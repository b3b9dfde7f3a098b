// The two per-ray chains of the NeRF method (volsurfs_py/methods/nerf.py, utils/nerf_utils.py)
// that the reference runs as long sequences of single ops on every ray of every iteration, fused
// into one launch each.  The half-wave layout, the sweeps and the order of their fp32 operations
// are ray_sweep.h's; this file holds what is the NeRF method's: its alpha and what it accumulates.
#include "ray_sweep.h"

namespace {

using namespace vsa_ray;

// alpha = 1 - exp(-density dt) of one sample, with the e its backward multiplies by
struct NerfAlpha {
  float e, alpha;
};
__device__ __forceinline__ float alpha_value(const NerfAlpha& a) { return a.alpha; }
__device__ __forceinline__ NerfAlpha nerf_alpha(float density, float dt) {
  NerfAlpha a;
  a.e = expf((-density) * dt);
  a.alpha = 1.0f - a.e;
  return a;
}

// Forward.  Per ray, with w_i = alpha_i T_i:
//   rgb_fg_d = sum_i w_i rgb_id   lane-strided partial sums over i = l, l + 32, .. then the
//                                 xor butterfly (integrate_fwd_kernel<3>);
//   depth    = sum_i w_i z_i      the same order (integrate_fwd_kernel<1>);
//   wsum     = sum over chunks of the butterfly sum of the chunk (sum_over_rays_kernel<1>);
//   rgb_d    = rgb_fg_d + (1 - wsum) bg_d.
__global__ void nerf_composite_fwd_kernel(const int* __restrict__ start_end,
                                          const float* __restrict__ density,
                                          const float* __restrict__ dt,
                                          const float* __restrict__ z,
                                          const float* __restrict__ rgb,
                                          const float* __restrict__ rgb_bg, int bg_stride,
                                          float* __restrict__ rgb_fg, float* __restrict__ rgb_out,
                                          float* __restrict__ wsum_out,
                                          float* __restrict__ depth_out,
                                          float* __restrict__ weights, int N) {
  RAY_PROLOGUE();
  float acc[3] = {0.f, 0.f, 0.f};
  float accz = 0.f, ws = 0.f;
  for_each_weight(
      n, l, i0, [&](long long s, int) { return nerf_alpha(density[s], dt[s]); },
      [&](long long s, bool in, const NerfAlpha&, float, float w) {
        if (in) {
          if (weights) weights[s] = w;
#pragma unroll
          for (int d = 0; d < 3; ++d) acc[d] += w * rgb[s * 3 + d];
          accz += w * z[s];
        }
        ws += sub_reduce_add(in ? w : 0.f);
      });
  float fg[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) fg[d] = sub_reduce_add(acc[d]);
  const float depth = sub_reduce_add(accz);
  if (l == 0) {
    wsum_out[ray] = ws;
    depth_out[ray] = depth;
    const float bgT = 1.0f - ws;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      rgb_fg[ray * 3 + d] = fg[d];
      if (rgb_out) rgb_out[ray * 3 + d] = rgb_bg ? fg[d] + bgT * rgb_bg[ray * bg_stride + d] : fg[d];
    }
  }
}

// Backward (bg_grad, wsum_grad and the two sweeps of ray_sweep.h).  The weight's use besides the
// colour integral is the weight sum, so g_w's other term is g_wsum; the alpha backward is
//   g_density = -(((-g_alpha) e) dt).
// scratch: 2 floats per sample.
__global__ void nerf_composite_bwd_kernel(const int* __restrict__ start_end,
                                          const float* __restrict__ density,
                                          const float* __restrict__ dt,
                                          const float* __restrict__ rgb,
                                          const float* __restrict__ rgb_bg, int bg_stride,
                                          const float* __restrict__ wsum,
                                          const float* __restrict__ g_rgb,
                                          const float* __restrict__ g_wsum_in,
                                          float* __restrict__ g_density,
                                          float* __restrict__ g_rgb_samples,
                                          float* __restrict__ g_rgb_bg,
                                          float* __restrict__ scratch, int N, int bug_compat) {
  RAY_PROLOGUE();
  float g[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) g[d] = g_rgb[ray * 3 + d];
  const float g_bgT =
      bg_grad(g, rgb_bg, bg_stride, ray, l, g_rgb_bg, [&] { return 1.0f - wsum[ray]; });
  const float g_ws = wsum_grad(g_wsum_in, ray, rgb_bg != nullptr, g_bgT);
  if (n <= 0) return;
  const auto alpha_of = [&](long long s, int) { return nerf_alpha(density[s], dt[s]); };
  composite_bwd_weights(
      n, l, i0, 1, 0, alpha_of, g, rgb, bug_compat,
      [&](long long, const NerfAlpha&, float) { return g_ws; }, g_rgb_samples, scratch);
  composite_bwd_alphas(n, l, i0, i1, 1, 0, alpha_of, scratch,
                       [&](long long s, const NerfAlpha& a, float g_alpha) {
                         const float gu = (-g_alpha) * a.e;
                         g_density[s] = -(gu * dt[s]);
                       });
}

// The coarse pass of importance_sampling_nerf (utils/nerf_utils.py:61-82) from the uniform
// samples' densities to the CDF: coarse_cdf with
//   alpha = min(max(1 - exp(-density dt), 0), 1).
__global__ void nerf_coarse_cdf_kernel(const int* __restrict__ start_end,
                                       const float* __restrict__ density,
                                       const float* __restrict__ dt, float* __restrict__ cdf,
                                       int N) {
  RAY_PROLOGUE();
  coarse_cdf(n, l, i0, i1, [&](long long s, int) {
    const float e = expf((-density[s]) * dt[s]);
    return fminf(fmaxf(1.0f - e, 0.0f), 1.0f);
  }, cdf);
}

}  // namespace

extern "C" int vsa_nerf_composite_fwd(const int32_t* start_end, const float* density,
                                      const float* dt, const float* samples_z, const float* rgb,
                                      const float* rgb_bg, int bg_per_ray, float* rgb_fg,
                                      float* rgb_out, float* weights_sum, float* depth,
                                      float* weights, int nr_rays, void* stream) {
  // the per-sample arrays are only read for rays with samples: NULL is fine for a pack without any
  RAY_CHECK(nr_rays >= 0);
  if (nr_rays == 0) return VSA_OK;
  RAY_CHECK(start_end && rgb_fg && weights_sum && depth && (bg_per_ray == 0 || bg_per_ray == 1) &&
           (!rgb_bg || rgb_out));
  RAY_LAUNCH(nerf_composite_fwd_kernel, nr_rays, start_end, density, dt, samples_z, rgb, rgb_bg,
            bg_per_ray ? 3 : 0, rgb_fg, rgb_out, weights_sum, depth, weights, nr_rays);
}

extern "C" int vsa_nerf_composite_bwd(const int32_t* start_end, const float* density,
                                      const float* dt, const float* rgb, const float* rgb_bg,
                                      int bg_per_ray, const float* weights_sum, const float* g_rgb,
                                      const float* g_weights_sum, float* g_density,
                                      float* g_rgb_samples, float* g_rgb_bg, float* scratch,
                                      int nr_rays, int bug_compat, void* stream) {
  RAY_CHECK(nr_rays >= 0);
  if (nr_rays == 0) return VSA_OK;
  RAY_CHECK(start_end && g_rgb && (bg_per_ray == 0 || bg_per_ray == 1) &&
           (!g_rgb_bg || (rgb_bg && weights_sum)));
  RAY_LAUNCH(nerf_composite_bwd_kernel, nr_rays, start_end, density, dt, rgb, rgb_bg,
            bg_per_ray ? 3 : 0, weights_sum, g_rgb, g_weights_sum, g_density, g_rgb_samples,
            g_rgb_bg, scratch, nr_rays, bug_compat);
}

extern "C" int vsa_nerf_coarse_cdf(const int32_t* start_end, const float* density, const float* dt,
                                   float* cdf, int nr_rays, void* stream) {
  RAY_CHECK(nr_rays >= 0);
  if (nr_rays == 0) return VSA_OK;
  RAY_CHECK(start_end);
  RAY_LAUNCH(nerf_coarse_cdf_kernel, nr_rays, start_end, density, dt, cdf, nr_rays);
}
