// The two per-ray chains of the Surf method (volsurfs_py/methods/surf.py render_fg_volumetric,
// volume_rendering_modules.py VolumeRenderingNeuS, utils/sdf_utils.py importance_sampling_sdf) that
// the reference runs as long sequences of single ops on every ray of every iteration, fused into one
// launch each.
//
// Layout as in nerf_render.hip: a ray is owned by a 32-lane half-wave, lanes = consecutive samples,
// the scans / reductions of ray_scan.h, chunks of 32 samples with a carried running value for
// longer rays.  No atomics: every output element has exactly one writer, so the output bits depend
// only on the inputs.  The build has -ffp-contract=off, so every fp32 operation below is a single
// rounding, in the order written.
#include "neus_alpha.h"

namespace {

constexpr int SR_BLOCK = 256;
using namespace vsa_ray;

#define SR_RAY_PROLOGUE() VSA_RAY_PROLOGUE(SR_BLOCK)

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
  SR_RAY_PROLOGUE();
  float acc[3] = {0.f, 0.f, 0.f}, accn[3] = {0.f, 0.f, 0.f};
  float accz = 0.f, ws = 0.f;
  float carry = 1.0f;
  for (int c = 0; c < n; c += SUB) {
    const int i = c + l;
    const bool in = i < n;
    const long long s = i0 + (in ? i : 0);
    const float dts = dt[s];
    const NeusAlpha a = neus_alpha(sdf[s], sdf_grad + s * 3, dirs + s * 3, dts, car, omc, beta);
    const float a1 = (1.0f - a.alpha) + 1e-6f;
    const float T = transmittance_step(a1, in, l, carry);
    const float w = a.alpha * T;
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
  }
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

// Backward.  Per ray, as vsa_nerf_composite_bwd: g_d = g_rgb_d;  with a background
//   g_bgT = (g_0 bg_0 + g_1 bg_1) + g_2 bg_2,  g_bg_d = g_d (1 - wsum),
//   g_wsum = g_wsum_in + (-g_bgT)             (g_wsum_in = 0 without it).
// Per sample, forward sweep (alpha and T recomputed as in the forward kernel):
//   g_w = integrate3_grad_w (bug_compat as vsa_packed_integrate_bwd) + g_wsum;
//   g_rgb_sample_d = g_d w;  lv = (g_w alpha) T;  g_w T kept for the reversed sweep.
// Reversed sweep: the suffix sums of lv in cumsum_kernel(inverse)'s order, the cumprod backward
// (next suffix sum / max(a1, 1e-6), 0 for the ray's last sample), g_alpha = g_w T + (-g_a1), then
// neus_alpha_bwd.  scratch: 2 floats per sample.
__global__ void neus_composite_bwd_kernel(
    const int* __restrict__ start_end, const float* __restrict__ sdf,
    const float* __restrict__ sdf_grad, const float* __restrict__ dirs,
    const float* __restrict__ dt, const float* __restrict__ rgb, const float* __restrict__ rgb_bg,
    int bg_stride, float car, float omc, float beta, const float* __restrict__ wsum,
    const float* __restrict__ g_rgb, const float* __restrict__ g_wsum_in,
    float* __restrict__ g_sdf, float* __restrict__ g_sdf_grad, float* __restrict__ g_rgb_samples,
    float* __restrict__ g_rgb_bg, float* __restrict__ scratch, int N, int bug_compat) {
  SR_RAY_PROLOGUE();
  float g[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) g[d] = g_rgb[ray * 3 + d];
  float g_ws = g_wsum_in ? g_wsum_in[ray] : 0.0f;
  if (rgb_bg) {
    const float* b = rgb_bg + ray * bg_stride;
    float g_bgT = g[0] * b[0];
    g_bgT += g[1] * b[1];
    g_bgT += g[2] * b[2];
    g_ws = g_wsum_in ? g_ws + (-g_bgT) : -g_bgT;
    if (g_rgb_bg && l == 0) {
      const float bgT = 1.0f - wsum[ray];
#pragma unroll
      for (int d = 0; d < 3; ++d) g_rgb_bg[ray * 3 + d] = g[d] * bgT;
    }
  }
  if (n <= 0) return;
  float carry = 1.0f;
  for (int c = 0; c < n; c += SUB) {
    const int i = c + l;
    const bool in = i < n;
    const long long s = i0 + (in ? i : 0);
    const NeusAlpha a = neus_alpha(sdf[s], sdf_grad + s * 3, dirs + s * 3, dt[s], car, omc, beta);
    const float a1 = (1.0f - a.alpha) + 1e-6f;
    const float T = transmittance_step(a1, in, l, carry);
    if (in) {
      const float w = a.alpha * T;
#pragma unroll
      for (int d = 0; d < 3; ++d) g_rgb_samples[s * 3 + d] = g[d] * w;
      const float gw = integrate3_grad_w(g, rgb + s * 3, bug_compat) + g_ws;
      const float gT = gw * a.alpha;
      scratch[2 * s] = gT * T;
      scratch[2 * s + 1] = gw * T;
    }
  }
  float csum = 0.0f;
  for (int c = 0; c < n; c += SUB) {
    const int i = c + l;
    const bool in = i < n;
    const long long s = in ? (long long)i1 - 1 - i : (long long)i0;
    const float cs_next = cumprod_bwd_suffix_step(in ? scratch[2 * s] : 0.0f, in, l, csum);
    if (in) {
      const float dts = dt[s];
      const float* dir = dirs + s * 3;
      const NeusAlpha a = neus_alpha(sdf[s], sdf_grad + s * 3, dir, dts, car, omc, beta);
      const float a1 = (1.0f - a.alpha) + 1e-6f;
      float ga1 = 0.f;
      if (i > 0) ga1 = cs_next / fmaxf(a1, 1e-6f);
      const float g_alpha = scratch[2 * s + 1] + (-ga1);
      float gs, gg[3];
      neus_alpha_bwd(a, g_alpha, dir, dts, car, omc, beta, gs, gg);
      g_sdf[s] = gs;
#pragma unroll
      for (int d = 0; d < 3; ++d) g_sdf_grad[s * 3 + d] = gg[d];
    }
  }
}

// One round of importance_sampling_sdf (utils/sdf_utils.py:87-109 / :153-175) from the pack's SDF
// to the CDF:
//   alpha = sdf2alpha(sdf, beta) for every sample but the ray's last, 0 there (vsa_packed_sdf2alpha
//           leaves it at zero);  T = cumprod((1 - alpha) + 1e-6);  w = alpha T;
//   wsum  = sum over chunks of the butterfly sum of the chunk (sum_over_rays_kernel<1>);
//   w    /= max(wsum, 1e-6);
//   cdf_i = carry + (incl_i - w_i) with incl the chunk's inclusive shuffle scan, and the last entry
//           snapped to 1 when |wsum' - 1| < 1e-3 and |cdf_last - 1| > 1e-3 (compute_cdf_kernel).
// Rays with fewer than 2 samples get a zero CDF.  The first sweep parks w in `cdf` (each lane
// re-reads only what it wrote).
__global__ void sdf_coarse_cdf_kernel(const int* __restrict__ start_end,
                                      const float* __restrict__ sdf, const float* __restrict__ dt,
                                      float beta, float* __restrict__ cdf, int N) {
  SR_RAY_PROLOGUE();
  if (n < 2) {
    if (n == 1 && l == 0) cdf[i0] = 0.0f;
    return;
  }
  float carry = 1.0f, ws = 0.f;
  for (int c = 0; c < n; c += SUB) {
    const int i = c + l;
    const bool in = i < n;
    const long long s = i0 + (in ? i : 0);
    const float alpha = (i < n - 1) ? sdf2alpha_sample(sdf[s], sdf[s + 1], dt[s], beta) : 0.0f;
    const float a1 = (1.0f - alpha) + 1e-6f;
    const float T = transmittance_step(a1, in, l, carry);
    const float w = alpha * T;
    if (in) cdf[s] = w;
    ws += sub_reduce_add(in ? w : 0.f);
  }
  const float wn = fmaxf(ws, 1e-6f);
  float run = 0.0f, last_cdf = 0.0f;
  for (int c = 0; c < n; c += SUB) {
    const int i = c + l;
    const float x = i < n ? cdf[i0 + i] / wn : 0.0f;
    const float incl = sub_scan_add(x, l);
    const float excl = run + (incl - x);
    if (i < n) cdf[i0 + i] = excl;
    if (i == n - 1) last_cdf = excl;
    run += __shfl(incl, SUB - 1, SUB);
  }
  const int owner = (n - 1) & (SUB - 1);
  if (l == owner && fabs((double)run - 1.0) < 1e-3 && fabs((double)last_cdf - 1.0) > 1e-3)
    cdf[i1 - 1] = 1.0f;
}

inline dim3 sr_grid(int N) { return dim3(vsa_div_up((long long)N * SUB, SR_BLOCK)); }

}  // namespace

#define SR_CHECK(cond) \
  if (!(cond)) return VSA_ERR_ARG
#define SR_LAUNCH(kernel, N, ...)                                                          \
  if ((N) == 0) return VSA_OK;                                                             \
  hipLaunchKernelGGL(kernel, sr_grid(N), dim3(SR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); \
  VSA_RETURN_LAUNCH_STATUS()

extern "C" int vsa_neus_composite_fwd(const int32_t* start_end, const float* sdf,
                                      const float* sdf_grad, const float* dirs, const float* dt,
                                      const float* samples_z, const float* normals,
                                      const float* rgb, const float* rgb_bg, int bg_per_ray,
                                      double cos_anneal_ratio, double logistic_beta,
                                      float* rgb_fg, float* rgb_out, float* weights_sum,
                                      float* depth, float* normals_out, float* weights,
                                      float* alpha, int nr_rays, void* stream) {
  // the per-sample arrays are only read for rays with samples: NULL is fine for a pack without any
  SR_CHECK(nr_rays >= 0);
  if (nr_rays == 0) return VSA_OK;
  SR_CHECK(start_end && rgb_fg && weights_sum && depth && normals_out &&
           (bg_per_ray == 0 || bg_per_ray == 1) && (!rgb_bg || rgb_out));
  // the reference's scalars are Python floats: torch rounds them to fp32 at the op, and
  // 1 - cos_anneal_ratio is formed in double before that
  SR_LAUNCH(neus_composite_fwd_kernel, nr_rays, start_end, sdf, sdf_grad, dirs, dt, samples_z,
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
  SR_CHECK(nr_rays >= 0);
  if (nr_rays == 0) return VSA_OK;
  SR_CHECK(start_end && g_rgb && (bg_per_ray == 0 || bg_per_ray == 1) &&
           (!g_rgb_bg || (rgb_bg && weights_sum)));
  SR_LAUNCH(neus_composite_bwd_kernel, nr_rays, start_end, sdf, sdf_grad, dirs, dt, rgb, rgb_bg,
            bg_per_ray ? 3 : 0, (float)cos_anneal_ratio, (float)(1.0 - cos_anneal_ratio),
            (float)logistic_beta, weights_sum, g_rgb, g_weights_sum, g_sdf, g_sdf_grad,
            g_rgb_samples, g_rgb_bg, scratch, nr_rays, bug_compat);
}

extern "C" int vsa_sdf_coarse_cdf(const int32_t* start_end, const float* sdf, const float* dt,
                                  float logistic_beta, float* cdf, int nr_rays, void* stream) {
  SR_CHECK(nr_rays >= 0);
  if (nr_rays == 0) return VSA_OK;
  SR_CHECK(start_end);
  SR_LAUNCH(sdf_coarse_cdf_kernel, nr_rays, start_end, sdf, dt, logistic_beta, cdf, nr_rays);
}
