// The per-ray chains of the OffsetsSurfs method (volsurfs_py/methods/offsets_surfs.py
// render_fg_volumetric and render_rays, utils/sdfs_utils.py importance_sampling_sdfs_iter): for each
// of K surfaces a full NeuS chain, then the dense blend of the K shells and the background, and one
// importance round that averages K CDFs.  The reference runs these as K chains of single ops per ray;
// here each is one launch.
//
// The half-wave layout, the sweeps and the order of their fp32 operations are ray_sweep.h's, the
// surfaces one after the other inside the half-wave.  Per-sample arrays are [S, K] (sample-major,
// as the model returns them).  This file holds what is the OffsetsSurfs method's: the second
// integral (the transparency), the blend of the K shells and the average of K CDFs.  The per-ray
// K-vectors of the blend live in fixed arrays of OR_MAX_SURFS registers indexed only by unrolled
// constants (k < K guards), so they never go to scratch.
#include "neus_alpha.h"
#include "ray_sweep.h"

namespace {

constexpr int OR_MAX_SURFS = 16;
using namespace vsa_ray;

// arr[k] = v / arr[k] for a runtime k, as a chain of selects over constant indices (registers only)
__device__ __forceinline__ void put_k(float (&arr)[OR_MAX_SURFS], int k, float v) {
#pragma unroll
  for (int j = 0; j < OR_MAX_SURFS; ++j)
    if (j == k) arr[j] = v;
}
__device__ __forceinline__ float get_k(const float (&arr)[OR_MAX_SURFS], int k) {
  float v = 0.0f;
#pragma unroll
  for (int j = 0; j < OR_MAX_SURFS; ++j)
    if (j == k) v = arr[j];
  return v;
}

// render_fg_volumetric's transparency decay (no gradient in the reference):
//   dot = clamp((-d_0 n_0 + -d_1 n_1) + -d_2 n_2, 0, 1)     torch.sum(-dirs * normals, dim=1)
//   decay = sigmoid(f dot) 2 - 1
__device__ __forceinline__ float transparency_decay(const float* dir, const float* nrm, float f) {
  float dot = (-dir[0]) * nrm[0];
  dot = dot + (-dir[1]) * nrm[1];
  dot = dot + (-dir[2]) * nrm[2];
  dot = fminf(fmaxf(dot, 0.0f), 1.0f);
  return sigmoid_torch(f * dot) * 2.0f - 1.0f;
}

// Forward.  For each surface k (column k of the [S, K] inputs, inner to outer), as
// neus_composite_fwd_kernel: alpha from neus_alpha, T = cumprod((1 - alpha) + 1e-6), w = alpha T;
//   surfs_rgb_k    = sum_i w_i rgb_ik             (integrate_fwd_kernel<3> order)
//   surfs_alpha_k  = sum_i w_i t_i                t_i = transparency_ik (times the decay when on)
//   surfs_depth_k  = sum_i w_i z_i,  surfs_normals_k = sum_i w_i nrm_ik,  surfs_wsum_k = sum_i w_i
// Then the blend, outer shell to inner (j = K - 1 - k, sequential over j):
//   t_0 = 1 - a_0, t_j = t_{j-1} (1 - a_j);  Tsurf_0 = 1, Tsurf_j = t_{j-1};  bw_j = Tsurf_j a_j;
//   rgb_fg = rgb_0 bw_0 + rgb_1 bw_1 + ..;  bgT = t_{K-1};  rgb = rgb_fg + rgb_bg bgT.
// Lane 0 holds the reduced values the outputs take, and writes every per-ray output.
__global__ void offsets_composite_fwd_kernel(
    const int* __restrict__ start_end, int K, const float* __restrict__ sdfs,
    const float* __restrict__ sdfs_grad, const float* __restrict__ normals,
    const float* __restrict__ rgb, const float* __restrict__ transp,
    const float* __restrict__ dirs, const float* __restrict__ dt, const float* __restrict__ z,
    const float* __restrict__ rgb_bg, int bg_stride, float car, float omc, float beta, int with_decay,
    float decay_f, float* __restrict__ surfs_rgb, float* __restrict__ surfs_normals,
    float* __restrict__ surfs_depths, float* __restrict__ surfs_wsum, float* __restrict__ surfs_alpha,
    float* __restrict__ surfs_T, float* __restrict__ surfs_bw, float* __restrict__ rgb_fg_out,
    float* __restrict__ bgT_out, float* __restrict__ rgb_out, float* __restrict__ alpha_out, int N) {
  RAY_PROLOGUE();
  float ra[OR_MAX_SURFS], rr[OR_MAX_SURFS], rg[OR_MAX_SURFS], rb[OR_MAX_SURFS];
  for (int k = 0; k < K; ++k) {
    float acc[3] = {0.f, 0.f, 0.f}, accn[3] = {0.f, 0.f, 0.f};
    float acct = 0.f, accz = 0.f, ws = 0.f;
    for_each_weight(
        n, l, i0,
        [&](long long s, int) {
          const long long sk = s * K + k;
          return neus_alpha(sdfs[sk], sdfs_grad + sk * 3, dirs + s * 3, dt[s], car, omc, beta);
        },
        [&](long long s, bool in, const NeusAlpha& a, float, float w) {
          if (in) {
            const long long sk = s * K + k;
            if (alpha_out) alpha_out[sk] = a.alpha;
            const float* nrm = normals + sk * 3;
            float t = transp[sk];
            if (with_decay) t = t * transparency_decay(dirs + s * 3, nrm, decay_f);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              acc[d] += w * rgb[sk * 3 + d];
              accn[d] += w * nrm[d];
            }
            acct += w * t;
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
    const float alpha_k = sub_reduce_add(acct);
    const float depth = sub_reduce_add(accz);
    if (l == 0) {
      const long long rk = ray * K + k;
      surfs_depths[rk] = depth;
      surfs_wsum[rk] = ws;
      surfs_alpha[rk] = alpha_k;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        surfs_rgb[rk * 3 + d] = fg[d];
        surfs_normals[rk * 3 + d] = nf[d];
      }
    }
    put_k(ra, k, alpha_k);
    put_k(rr, k, fg[0]);
    put_k(rg, k, fg[1]);
    put_k(rb, k, fg[2]);
  }
  if (l != 0) return;
  float t = 1.0f, out[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < OR_MAX_SURFS; ++j) {
    if (j < K) {
      const int k = K - 1 - j;
      const float a = get_k(ra, k);
      const float Ts = t;
      t = (j == 0) ? 1.0f - a : t * (1.0f - a);
      const float bw = Ts * a;
      const float col[3] = {get_k(rr, k), get_k(rg, k), get_k(rb, k)};
#pragma unroll
      for (int d = 0; d < 3; ++d) out[d] = (j == 0) ? col[d] * bw : out[d] + col[d] * bw;
      surfs_T[ray * K + k] = Ts;
      surfs_bw[ray * K + k] = bw;
    }
  }
  bgT_out[ray] = t;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    rgb_fg_out[ray * 3 + d] = out[d];
    rgb_out[ray * 3 + d] = rgb_bg ? out[d] + rgb_bg[ray * bg_stride + d] * t : out[d];
  }
}

// Backward.  From g_rgb [N,3] (of rgb), per ray, the blend's reverse sweep on the forward's
// surfs_rgb / surfs_alpha / surfs_T / bgT (every lane the same values):
//   g_bgT = (g_0 bg_0 + g_1 bg_1) + g_2 bg_2 (0 without a background), g_bg_d = g_d bgT;
//   g_rgb_j,d = g_d bw_j;  g_bw_j = (g_0 rgb_j0 + g_1 rgb_j1) + g_2 rgb_j2;
//   from j = K - 1 down to 0 with gt = g_bgT:  g_a_j = g_bw_j Tsurf_j - gt Tsurf_j,
//                                               gt = gt (1 - a_j) + g_bw_j a_j.
// Then per surface k the two sweeps of ray_sweep.h on column k with g_rgb_k = g bw_k: the weight's
// use besides the colour integral is the transparency integral, so g_w's other term is g_a_k t,
// with g_transparency = (g_a_k w) decay written on the way; the alpha backward is neus_alpha_bwd.
// scratch: 2 S K floats.
__global__ void offsets_composite_bwd_kernel(
    const int* __restrict__ start_end, int K, const float* __restrict__ sdfs,
    const float* __restrict__ sdfs_grad, const float* __restrict__ normals,
    const float* __restrict__ rgb, const float* __restrict__ transp,
    const float* __restrict__ dirs, const float* __restrict__ dt, const float* __restrict__ rgb_bg,
    int bg_stride, float car, float omc, float beta, int with_decay, float decay_f,
    const float* __restrict__ surfs_rgb, const float* __restrict__ surfs_alpha,
    const float* __restrict__ surfs_T, const float* __restrict__ bgT_in,
    const float* __restrict__ g_rgb, float* __restrict__ g_sdfs, float* __restrict__ g_sdfs_grad,
    float* __restrict__ g_rgb_samples, float* __restrict__ g_transp, float* __restrict__ g_rgb_bg,
    float* __restrict__ scratch, int N, int bug_compat) {
  RAY_PROLOGUE();
  float g[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) g[d] = g_rgb[ray * 3 + d];
  const float g_bgT = bg_grad(g, rgb_bg, bg_stride, ray, l, g_rgb_bg, [&] { return bgT_in[ray]; });
  // the blend's reverse sweep: per-surface g of surfs_rgb (times g_d below) and of surfs_alpha
  float gbw[OR_MAX_SURFS], ga[OR_MAX_SURFS];
  float gt = g_bgT;
#pragma unroll
  for (int j = OR_MAX_SURFS - 1; j >= 0; --j) {
    gbw[j] = 0.0f;
    ga[j] = 0.0f;
    if (j < K) {
      const long long rk = ray * K + (K - 1 - j);
      const float a = surfs_alpha[rk], Ts = surfs_T[rk];
      float gw = g[0] * surfs_rgb[rk * 3];
      gw += g[1] * surfs_rgb[rk * 3 + 1];
      gw += g[2] * surfs_rgb[rk * 3 + 2];
      gbw[j] = Ts * a;          // bw_j, for g_rgb_j = g bw_j
      ga[j] = gw * Ts - gt * Ts;
      gt = gt * (1.0f - a) + gw * a;
    }
  }
  if (n <= 0) return;
  for (int k = 0; k < K; ++k) {
    const int j = K - 1 - k;
    const float bwk = get_k(gbw, j), gak = get_k(ga, j);
    float gk[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) gk[d] = g[d] * bwk;
    const auto alpha_of = [&](long long s, int) {
      const long long sk = s * K + k;
      return neus_alpha(sdfs[sk], sdfs_grad + sk * 3, dirs + s * 3, dt[s], car, omc, beta);
    };
    composite_bwd_weights(
        n, l, i0, K, k, alpha_of, gk, rgb, bug_compat,
        [&](long long s, const NeusAlpha&, float w) {
          const long long sk = s * K + k;
          const float dec =
              with_decay ? transparency_decay(dirs + s * 3, normals + sk * 3, decay_f) : 1.0f;
          const float t = with_decay ? transp[sk] * dec : transp[sk];
          g_transp[sk] = (gak * w) * dec;
          return gak * t;
        },
        g_rgb_samples, scratch);
    composite_bwd_alphas(n, l, i0, i1, K, k, alpha_of, scratch,
                         [&](long long s, const NeusAlpha& a, float g_alpha) {
                           const long long sk = s * K + k;
                           float gs, gg[3];
                           neus_alpha_bwd(a, g_alpha, dirs + s * 3, dt[s], car, omc, beta, gs, gg);
                           g_sdfs[sk] = gs;
#pragma unroll
                           for (int d = 0; d < 3; ++d) g_sdfs_grad[sk * 3 + d] = gg[d];
                         });
  }
}

// One round of importance_sampling_sdfs_iter (utils/sdfs_utils.py:12-64) from the pack's SDFs [S, K]
// to the CDF [S]: for k = 0 .. K - 1, as sdf_coarse_cdf_kernel on column k but with the transmittance
// clipped (T = min(max(cumprod((1 - alpha) + 1e-6), 0), 1)), and agg = (0 + cdf_0) + cdf_1 + ..;
// cdf = agg (1 / K) (torch's division of a tensor by a host scalar multiplies by its reciprocal).
// The weight sum needs the whole ray before the CDF can start, so the second sweep recomputes
// alpha and T (same inputs, same operations, same bits) instead of parking w.  The aggregate lives
// in `cdf`: each lane reads back only the samples it wrote.  Rays with fewer than 2 samples get a
// zero CDF.
__global__ void sdfs_coarse_cdf_kernel(const int* __restrict__ start_end, int K,
                                       const float* __restrict__ sdfs, const float* __restrict__ dt,
                                       float beta, float inv_k, float* __restrict__ cdf, int N) {
  RAY_PROLOGUE();
  if (cdf_of_short_ray(n, l, i0, cdf)) return;
  const int owner = (n - 1) & (SUB - 1);
  for (int k = 0; k < K; ++k) {
    const auto alpha_of = [&](long long s, int i) {
      return (i < n - 1) ? sdf2alpha_sample(sdfs[s * K + k], sdfs[(s + 1) * K + k], dt[s], beta)
                         : 0.0f;
    };
    // the reference clips T before it forms the weight, so the sweep's own w (alpha times the
    // unclipped T) is not used in either body
    const auto clip01 = [](float T) { return fminf(fmaxf(T, 0.0f), 1.0f); };
    float ws = 0.f;
    for_each_weight(n, l, i0, alpha_of, [&](long long, bool in, float alpha, float T, float) {
      ws += sub_reduce_add(in ? alpha * clip01(T) : 0.f);
    });
    const float wn = fmaxf(ws, 1e-6f);
    float run = 0.0f, last_cdf = 0.0f, agg_last = 0.0f;
    for_each_weight(n, l, i0, alpha_of, [&](long long s, bool in, float alpha, float T, float) {
      const float excl = cdf_scan_step(in ? (alpha * clip01(T)) / wn : 0.0f, l, run);
      if (in) {
        const float prev = k == 0 ? 0.0f : cdf[s];
        if (s == i1 - 1) {
          last_cdf = excl;
          agg_last = prev;
        } else {
          const float agg = prev + excl;
          cdf[s] = k == K - 1 ? agg * inv_k : agg;
        }
      }
    });
    // the ray's last sample: compute_cdf's snap to 1, then the aggregate
    if (l == owner) {
      const float v = cdf_snaps_last(run, last_cdf) ? 1.0f : last_cdf;
      const float agg = agg_last + v;
      cdf[i1 - 1] = k == K - 1 ? agg * inv_k : agg;
    }
  }
}

}  // namespace

extern "C" int vsa_offsets_composite_fwd(
    const int32_t* start_end, int nr_surfs, const float* sdfs, const float* sdfs_grad,
    const float* normals, const float* rgb, const float* transparency, const float* dirs,
    const float* dt, const float* samples_z, const float* rgb_bg, int bg_per_ray,
    double cos_anneal_ratio, double logistic_beta, int with_alpha_decay, double alpha_decay_factor,
    float* surfs_rgb, float* surfs_normals, float* surfs_depths, float* surfs_weight_sum,
    float* surfs_alpha, float* surfs_transmittance, float* surfs_blending_weights, float* rgb_fg,
    float* bg_transmittance, float* rgb_out, float* alpha, int nr_rays, void* stream) {
  RAY_CHECK(nr_rays >= 0);
  if (nr_surfs < 1 || nr_surfs > OR_MAX_SURFS) return VSA_ERR_UNSUPPORTED;
  if (nr_rays == 0) return VSA_OK;
  RAY_CHECK(start_end && surfs_rgb && surfs_normals && surfs_depths && surfs_weight_sum &&
           surfs_alpha && surfs_transmittance && surfs_blending_weights && rgb_fg &&
           bg_transmittance && rgb_out && (bg_per_ray == 0 || bg_per_ray == 1));
  RAY_LAUNCH(offsets_composite_fwd_kernel, nr_rays, start_end, nr_surfs, sdfs, sdfs_grad, normals,
            rgb, transparency, dirs, dt, samples_z, rgb_bg, bg_per_ray ? 3 : 0,
            (float)cos_anneal_ratio, (float)(1.0 - cos_anneal_ratio), (float)logistic_beta,
            with_alpha_decay ? 1 : 0, (float)alpha_decay_factor, surfs_rgb, surfs_normals,
            surfs_depths, surfs_weight_sum, surfs_alpha, surfs_transmittance,
            surfs_blending_weights, rgb_fg, bg_transmittance, rgb_out, alpha, nr_rays);
}

extern "C" int vsa_offsets_composite_bwd(
    const int32_t* start_end, int nr_surfs, const float* sdfs, const float* sdfs_grad,
    const float* normals, const float* rgb, const float* transparency, const float* dirs,
    const float* dt, const float* rgb_bg, int bg_per_ray, double cos_anneal_ratio,
    double logistic_beta, int with_alpha_decay, double alpha_decay_factor, const float* surfs_rgb,
    const float* surfs_alpha, const float* surfs_transmittance, const float* bg_transmittance,
    const float* g_rgb, float* g_sdfs, float* g_sdfs_grad, float* g_rgb_samples,
    float* g_transparency, float* g_rgb_bg, float* scratch, int nr_rays, int bug_compat,
    void* stream) {
  RAY_CHECK(nr_rays >= 0);
  if (nr_surfs < 1 || nr_surfs > OR_MAX_SURFS) return VSA_ERR_UNSUPPORTED;
  if (nr_rays == 0) return VSA_OK;
  RAY_CHECK(start_end && surfs_rgb && surfs_alpha && surfs_transmittance && bg_transmittance &&
           g_rgb && (bg_per_ray == 0 || bg_per_ray == 1) && (!g_rgb_bg || rgb_bg));
  RAY_LAUNCH(offsets_composite_bwd_kernel, nr_rays, start_end, nr_surfs, sdfs, sdfs_grad, normals,
            rgb, transparency, dirs, dt, rgb_bg, bg_per_ray ? 3 : 0, (float)cos_anneal_ratio,
            (float)(1.0 - cos_anneal_ratio), (float)logistic_beta, with_alpha_decay ? 1 : 0,
            (float)alpha_decay_factor, surfs_rgb, surfs_alpha, surfs_transmittance,
            bg_transmittance, g_rgb, g_sdfs, g_sdfs_grad, g_rgb_samples, g_transparency, g_rgb_bg,
            scratch, nr_rays, bug_compat);
}

extern "C" int vsa_sdfs_coarse_cdf(const int32_t* start_end, int nr_surfs, const float* sdfs,
                                   const float* dt, float logistic_beta, float* cdf, int nr_rays,
                                   void* stream) {
  RAY_CHECK(nr_rays >= 0);
  if (nr_surfs < 1 || nr_surfs > OR_MAX_SURFS) return VSA_ERR_UNSUPPORTED;
  if (nr_rays == 0) return VSA_OK;
  RAY_CHECK(start_end && cdf);
  RAY_LAUNCH(sdfs_coarse_cdf_kernel, nr_rays, start_end, nr_surfs, sdfs, dt, logistic_beta,
            1.0f / (float)nr_surfs, cdf, nr_rays);
}
