// The two per-ray chains of the Surf method (volsurfs_py/methods/surf.py render_fg_volumetric,
// volume_rendering_modules.py VolumeRenderingNeuS, utils/sdf_utils.py importance_sampling_sdf) that
// the reference runs as long sequences of single ops on every ray of every iteration, fused into one
// launch each.
//
// The half-wave layout, the sweeps and the order of their fp32 operations are ray_sweep.h's; this
// file holds what is the Surf method's: the NeuS alpha (neus_alpha.h) and what it accumulates.
#include "neus_alpha.h"
#include "ray_sweep.h"

namespace {

using namespace vsa_ray;

// Forward.  Per ray, with alpha from neus_alpha, T = cumprod((1 - alpha) + 1e-6) and w = alpha T
// (compute_transmittance_from_alphas, weights = alpha * transmittance):
//   rgb_fg_d  = sum_i w_i rgb_id    lane-strided partial sums over i = l, l + 32, .. then the xor
//                                   butterfly (integrate_fwd_kernel<3>);
//   normals_d = sum_i w_i nrm_id    the same order;  depth = sum_i w_i z_i (integrate_fwd_kernel<1>);
//   wsum      = sum over chunks of the butterfly sum of the chunk (sum_over_rays_kernel<1>);
//   rgb_d     = rgb_fg_d + (1 - wsum) bg_d.
__global__ void neus_composite_fwd_kernel(
    const int* __restrict__ start_end, const float* __restrict__ sdf,
    const float* __restrict__ sdf_grad, const float* __restrict__ dirs,
    const float* __restrict__ dt, const float* __restrict__ z, const float* __restrict__ normals,
    const float* __restrict__ rgb, const float* __restrict__ rgb_bg, int bg_stride, float car,
    float omc, float beta, float* __restrict__ rgb_fg, float* __restrict__ rgb_out,
    float* __restrict__ wsum_out, float* __restrict__ depth_out, float* __restrict__ normals_out,
    float* __restrict__ weights, float* __restrict__ alpha_out, int N) {
  RAY_PROLOGUE();
  float acc[3] = {0.f, 0.f, 0.f}, accn[3] = {0.f, 0.f, 0.f};
  float accz = 0.f, ws = 0.f;
  for_each_weight(
      n, l, i0,
      [&](long long s, int) {
        return neus_alpha(sdf[s], sdf_grad + s * 3, dirs + s * 3, dt[s], car, omc, beta);
      },
      [&](long long s, bool in, const NeusAlpha& a, float, float w) {
        if (in) {
          if (weights) weights[s] = w;
          if (alpha_out) alpha_out[s] = a.alpha;
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            acc[d] += w * rgb[s * 3 + d];
            accn[d] += w * normals[s * 3 + d];
          }
          accz += w * z[s];
        }
        ws += sub_reduce_add(in ? w : 0.f);
      });
  float fg[3], nf[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    fg[d] = sub_reduce_add(acc[d]);
    nf[d] = sub_reduce_add(accn[d]);
  }
  const float depth = sub_reduce_add(accz);
  if (l == 0) {
    wsum_out[ray] = ws;
    depth_out[ray] = depth;
    const float bgT = 1.0f - ws;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      rgb_fg[ray * 3 + d] = fg[d];
      normals_out[ray * 3 + d] = nf[d];
      if (rgb_out) rgb_out[ray * 3 + d] = rgb_bg ? fg[d] + bgT * rgb_bg[ray * bg_stride + d] : fg[d];
    }
  }
}

// Backward (bg_grad, wsum_grad and the two sweeps of ray_sweep.h), as nerf_composite_bwd_kernel:
// g_w's other term is g_wsum; the alpha backward is neus_alpha_bwd.  scratch: 2 floats per sample.
__global__ void neus_composite_bwd_kernel(
    const int* __restrict__ start_end, const float* __restrict__ sdf,
    const float* __restrict__ sdf_grad, const float* __restrict__ dirs,
    const float* __restrict__ dt, const float* __restrict__ rgb, const float* __restrict__ rgb_bg,
    int bg_stride, float car, float omc, float beta, const float* __restrict__ wsum,
    const float* __restrict__ g_rgb, const float* __restrict__ g_wsum_in,
    float* __restrict__ g_sdf, float* __restrict__ g_sdf_grad, float* __restrict__ g_rgb_samples,
    float* __restrict__ g_rgb_bg, float* __restrict__ scratch, int N, int bug_compat) {
  RAY_PROLOGUE();
  float g[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) g[d] = g_rgb[ray * 3 + d];
  const float g_bgT =
      bg_grad(g, rgb_bg, bg_stride, ray, l, g_rgb_bg, [&] { return 1.0f - wsum[ray]; });
  const float g_ws = wsum_grad(g_wsum_in, ray, rgb_bg != nullptr, g_bgT);
  if (n <= 0) return;
  const auto alpha_of = [&](long long s, int) {
    return neus_alpha(sdf[s], sdf_grad + s * 3, dirs + s * 3, dt[s], car, omc, beta);
  };
  composite_bwd_weights(
      n, l, i0, 1, 0, alpha_of, g, rgb, bug_compat,
      [&](long long, const NeusAlpha&, float) { return g_ws; }, g_rgb_samples, scratch);
  composite_bwd_alphas(n, l, i0, i1, 1, 0, alpha_of, scratch,
                       [&](long long s, const NeusAlpha& a, float g_alpha) {
                         float gs, gg[3];
                         neus_alpha_bwd(a, g_alpha, dirs + s * 3, dt[s], car, omc, beta, gs, gg);
                         g_sdf[s] = gs;
#pragma unroll
                         for (int d = 0; d < 3; ++d) g_sdf_grad[s * 3 + d] = gg[d];
                       });
}

// One round of importance_sampling_sdf (utils/sdf_utils.py:87-109 / :153-175) from the pack's SDF
// to the CDF: coarse_cdf with
//   alpha = sdf2alpha(sdf, beta) for every sample but the ray's last, 0 there (vsa_packed_sdf2alpha
//           leaves it at zero).
__global__ void sdf_coarse_cdf_kernel(const int* __restrict__ start_end,
                                      const float* __restrict__ sdf, const float* __restrict__ dt,
                                      float beta, float* __restrict__ cdf, int N) {
  RAY_PROLOGUE();
  coarse_cdf(n, l, i0, i1, [&](long long s, int i) {
    return (i < n - 1) ? sdf2alpha_sample(sdf[s], sdf[s + 1], dt[s], beta) : 0.0f;
  }, cdf);
}

}  // namespace

extern "C" int vsa_neus_composite_fwd(const int32_t* start_end, const float* sdf,
                                      const float* sdf_grad, const float* dirs, const float* dt,
                                      const float* samples_z, const float* normals,
                                      const float* rgb, const float* rgb_bg, int bg_per_ray,
                                      double cos_anneal_ratio, double logistic_beta,
                                      float* rgb_fg, float* rgb_out, float* weights_sum,
                                      float* depth, float* normals_out, float* weights,
                                      float* alpha, int nr_rays, void* stream) {
  // the per-sample arrays are only read for rays with samples: NULL is fine for a pack without any
  RAY_CHECK(nr_rays >= 0);
  if (nr_rays == 0) return VSA_OK;
  RAY_CHECK(start_end && rgb_fg && weights_sum && depth && normals_out &&
           (bg_per_ray == 0 || bg_per_ray == 1) && (!rgb_bg || rgb_out));
  // the reference's scalars are Python floats: torch rounds them to fp32 at the op, and
  // 1 - cos_anneal_ratio is formed in double before that
  RAY_LAUNCH(neus_composite_fwd_kernel, nr_rays, start_end, sdf, sdf_grad, dirs, dt, samples_z,
            normals, rgb, rgb_bg, bg_per_ray ? 3 : 0, (float)cos_anneal_ratio,
            (float)(1.0 - cos_anneal_ratio), (float)logistic_beta, rgb_fg, rgb_out, weights_sum,
            depth, normals_out, weights, alpha, nr_rays);
}

extern "C" int vsa_neus_composite_bwd(const int32_t* start_end, const float* sdf,
                                      const float* sdf_grad, const float* dirs, const float* dt,
                                      const float* rgb, const float* rgb_bg, int bg_per_ray,
                                      double cos_anneal_ratio, double logistic_beta,
                                      const float* weights_sum, const float* g_rgb,
                                      const float* g_weights_sum, float* g_sdf, float* g_sdf_grad,
                                      float* g_rgb_samples, float* g_rgb_bg, float* scratch,
                                      int nr_rays, int bug_compat, void* stream) {
  RAY_CHECK(nr_rays >= 0);
  if (nr_rays == 0) return VSA_OK;
  RAY_CHECK(start_end && g_rgb && (bg_per_ray == 0 || bg_per_ray == 1) &&
           (!g_rgb_bg || (rgb_bg && weights_sum)));
  RAY_LAUNCH(neus_composite_bwd_kernel, nr_rays, start_end, sdf, sdf_grad, dirs, dt, rgb, rgb_bg,
            bg_per_ray ? 3 : 0, (float)cos_anneal_ratio, (float)(1.0 - cos_anneal_ratio),
            (float)logistic_beta, weights_sum, g_rgb, g_weights_sum, g_sdf, g_sdf_grad,
            g_rgb_samples, g_rgb_bg, scratch, nr_rays, bug_compat);
}

extern "C" int vsa_sdf_coarse_cdf(const int32_t* start_end, const float* sdf, const float* dt,
                                  float logistic_beta, float* cdf, int nr_rays, void* stream) {
  RAY_CHECK(nr_rays >= 0);
  if (nr_rays == 0) return VSA_OK;
  RAY_CHECK(start_end);
  RAY_LAUNCH(sdf_coarse_cdf_kernel, nr_rays, start_end, sdf, dt, logistic_beta, cdf, nr_rays);
}
