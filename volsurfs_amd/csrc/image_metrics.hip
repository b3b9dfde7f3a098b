// Held-out-view image metrics: per-image PSNR and SSIM of B image pairs of one size (piq 0.8.0's `psnr` / `ssim`
// with their defaults, as the reference's evaluation calls them: volsurfs_py/utils/evaluation.py:167-168).
//
//   psnr = -10 log10(mean((x - y)^2) + 1e-8)                over all 3 H W full-resolution values
//   ssim = mean over (channel, pixel) of the SSIM map        of the f x f average-pooled images, 11 x 11 Gaussian
//          (sigma 1.5), valid convolution, C1 = 0.01^2, C2 = 0.03^2
//
// Kernel 1 (`metrics_tile_kernel`), one workgroup per (image, tile of 64 x 16 pooled SSIM outputs):
//   1. squared error: the tile's disjoint share of the image's flat value range, in 16-value units (each value is
//      counted by exactly one workgroup of its image: the pooled tiles' halos do not line up with full-resolution
//      pixels, so this share is not the tile's footprint);
//   2. the full-resolution rows under the tile plus its 10-pixel halo are staged in LDS as aligned 16-byte chunks
//      (row runs, not pixels), pooled f x f into LDS (all three channels of pred and gt);
//   3. per channel an 11-tap horizontal pass over the five moments (x, y, x^2, y^2, xy) into LDS, then the 11-tap
//      vertical pass and the SSIM map in registers;
//   4. the two partial sums (squared error, SSIM map) go to the workspace: no atomics.
// Kernel 2 (`metrics_finish_kernel`), one workgroup per image: adds the image's tile partials in index order in
// fp64 and forms PSNR and SSIM.
//
// Every sum runs in an order fixed by the image size alone (never by the batch index, the tile a value was loaded
// in, or the pointer's alignment), so two calls return the same bits and B images in one call equal B calls of one.
// For x == y the expressions below give cs == ss == 1 exactly (2 s == s + s, 2 (m m) == m m + m m), so identical
// images score ssim == 1 and psnr == -10 log10(1e-8).
#include "common.h"

namespace {

constexpr int MT_BLOCK = 256;
constexpr int MT_TW = 64;                 // pooled SSIM outputs per tile, x
constexpr int MT_TH = 16;                 // ... y
constexpr int MT_K = 11;                  // Gaussian taps
constexpr int MT_C = MT_TW + MT_K - 1;    // pooled input columns per tile (74)
constexpr int MT_R = MT_TH + MT_K - 1;    // pooled input rows per tile (26)
constexpr int MT_HBUF = 5 * MT_R * MT_TW; // floats of the horizontal-pass buffer; the staging area aliases it
constexpr int MT_STAGE_BYTES = MT_HBUF * 4;
constexpr float MT_C1 = 0.01f * 0.01f;
constexpr float MT_C2 = 0.03f * 0.03f;

struct Taps {
  float g[MT_K];
};

struct MetricsArgs {
  const unsigned char* pred;
  const unsigned char* gt;
  long long pred_bytes, gt_bytes;   // whole buffers: the last 16-byte chunk of a buffer is never read past its end
  int pred_u8, gt_u8, quantize;     // dtype flags; quantize: the 8-bit rule on an fp32 pred
  int H, W, f, Hp, Wp, Ho, Wo;      // full, pooled, SSIM-map sizes
  int tiles_x, tiles;               // tiles per image
  int pc_max, gc_max, rows_per_round;   // staging: 16-byte chunks per full-res row (pred, gt), rows per round
  double* ws;                       // [B][tiles][2]: squared error, SSIM map sum
};

// The 8-bit round trip of a rendered image written as PNG and read back (u8 = trunc(clamp(x, 0, 1) * 255), read
// as u8 / 255): a restatement of mvdatasets' save_numpy_as_png / image_to_tensor, kept in this one function.
__device__ __forceinline__ float quantize8(float x) {
  return (float)(unsigned)(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f) / 255.0f;
}

__device__ __forceinline__ float u8_value(unsigned v) { return (float)v / 255.0f; }

// value `e` (in elements) of a staged or global byte run
__device__ __forceinline__ float value_at(const unsigned char* p, long long e, int is_u8, int quantize) {
  if (is_u8) return u8_value(p[e]);
  const float v = *reinterpret_cast<const float*>(p + 4 * e);
  return quantize ? quantize8(v) : v;
}

// sum over the block in a fixed tree; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* s_part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < MT_BLOCK / 64; ++w) r += s_part[w];
  }
  __syncthreads();
  return r;
}

// squared error of the 16 values [16 u, 16 u + 16) of one image (n values in all), summed in value order
__device__ __forceinline__ float sq_err_unit(const MetricsArgs& a, long long img, long long u, long long n,
                                             bool vec) {
  float xp[16], yp[16];
  const long long e0 = 16 * u;
  const unsigned char* P = a.pred + img * n * (a.pred_u8 ? 1 : 4);
  const unsigned char* G = a.gt + img * n * (a.gt_u8 ? 1 : 4);
  if (vec && e0 + 16 <= n) {      // both runs 16-byte aligned
    if (a.pred_u8) {
      const uint4 v = *reinterpret_cast<const uint4*>(P + e0);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 16; ++i) xp[i] = u8_value((w[i >> 2] >> (8 * (i & 3))) & 255u);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(P + 4 * (e0 + 4 * q));
        xp[4 * q] = v.x; xp[4 * q + 1] = v.y; xp[4 * q + 2] = v.z; xp[4 * q + 3] = v.w;
      }
      if (a.quantize) {
#pragma unroll
        for (int i = 0; i < 16; ++i) xp[i] = quantize8(xp[i]);
      }
    }
    if (a.gt_u8) {
      const uint4 v = *reinterpret_cast<const uint4*>(G + e0);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int i = 0; i < 16; ++i) yp[i] = u8_value((w[i >> 2] >> (8 * (i & 3))) & 255u);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(G + 4 * (e0 + 4 * q));
        yp[4 * q] = v.x; yp[4 * q + 1] = v.y; yp[4 * q + 2] = v.z; yp[4 * q + 3] = v.w;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool in = e0 + i < n;
      xp[i] = in ? value_at(P, e0 + i, a.pred_u8, a.quantize) : 0.0f;
      yp[i] = in ? value_at(G, e0 + i, a.gt_u8, 0) : 0.0f;
    }
  }
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float d = xp[i] - yp[i];
    s = fmaf(d, d, s);
  }
  return s;
}

// Stage full-res rows [r0, r1) of the tile's column run of one tensor into LDS: row k at stage + k * cmax * 16,
// starting at the 16-byte chunk that holds the run's first byte.
__device__ __forceinline__ void stage_rows(unsigned char* stage, const unsigned char* base, long long total_bytes,
                                           int esz, const MetricsArgs& a, long long img, int r0, int r1, int col0,
                                           int ncols, int cmax) {
  const int nq = (r1 - r0) * cmax;
  for (int q = threadIdx.x; q < nq; q += MT_BLOCK) {
    const int k = q / cmax, j = q - k * cmax;
    const long long s = ((img * a.H + r0 + k) * a.W + col0) * 3ll * esz;
    const long long a0 = s & ~15ll;
    const long long a1 = (s + 3ll * esz * ncols + 15) & ~15ll;
    const long long c = a0 + 16ll * j;
    if (c >= a1) continue;
    uint4* dst = reinterpret_cast<uint4*>(stage + (size_t)q * 16);
    if (c + 16 <= total_bytes) {
      *dst = *reinterpret_cast<const uint4*>(base + c);
    } else {                       // the buffer's last, partial chunk
      unsigned char tmp[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) tmp[i] = c + i < total_bytes ? base[c + i] : 0;
      *dst = *reinterpret_cast<const uint4*>(tmp);
    }
  }
}

__global__ __launch_bounds__(MT_BLOCK) void metrics_tile_kernel(MetricsArgs a, Taps taps) {
  __shared__ float s_x[3][MT_R][MT_C];
  __shared__ float s_y[3][MT_R][MT_C];
  __shared__ __attribute__((aligned(16))) float s_h[MT_HBUF];   // staging area, then the horizontal moments
  __shared__ double s_part[MT_BLOCK / 64];

  const int t = blockIdx.x % a.tiles;
  const long long img = blockIdx.x / a.tiles;
  const int tx = t % a.tiles_x, ty = t / a.tiles_x;
  const int ox = tx * MT_TW, oy = ty * MT_TH;                 // tile origin in pooled / SSIM-map coordinates
  const int rv = min(MT_R, a.Hp - oy), cv = min(MT_C, a.Wp - ox);   // pooled input rows / columns present

  // 1. squared error over this tile's share of the image's 16-value units
  const long long n = 3ll * a.H * a.W;
  const long long units = (n + 15) / 16;
  const long long u0 = units * t / a.tiles, u1 = units * (t + 1) / a.tiles;
  const bool vec = ((img * n * (a.pred_u8 ? 1 : 4)) & 15) == 0 && ((img * n * (a.gt_u8 ? 1 : 4)) & 15) == 0;
  double se = 0.0;
  for (long long u = u0 + threadIdx.x; u < u1; u += MT_BLOCK) se += (double)sq_err_unit(a, img, u, n, vec);

  // 2. pooled tile + halo in LDS (zeros outside the image: they feed only SSIM outputs that are not counted)
  for (int i = threadIdx.x; i < 3 * MT_R * MT_C; i += MT_BLOCK) {
    (&s_x[0][0][0])[i] = 0.0f;
    (&s_y[0][0][0])[i] = 0.0f;
  }
  const int f = a.f;
  const int pe = a.pred_u8 ? 1 : 4, ge = a.gt_u8 ? 1 : 4;
  unsigned char* stage = reinterpret_cast<unsigned char*>(s_h);
  unsigned char* stage_g = stage + (size_t)a.rows_per_round * a.pc_max * 16;
  const int fr_begin = oy * f, fr_end = (oy + rv) * f;       // full-res rows under the tile
  const int col0 = ox * f, ncols = cv * f;
  for (int r0 = fr_begin; r0 < fr_end; r0 += a.rows_per_round) {
    const int r1 = min(fr_end, r0 + a.rows_per_round);
    __syncthreads();               // the previous round's pooling has read the stage
    stage_rows(stage, a.pred, a.pred_bytes, pe, a, img, r0, r1, col0, ncols, a.pc_max);
    stage_rows(stage_g, a.gt, a.gt_bytes, ge, a, img, r0, r1, col0, ncols, a.gc_max);
    __syncthreads();
    // pooled rows this round touches; each (row, column, channel) item is owned by one thread per round, and adds
    // its full-res rows in row order
    const int p0 = r0 / f, p1 = (r1 - 1) / f + 1;
    const int nit = (p1 - p0) * cv * 3;
    for (int it = threadIdx.x; it < nit; it += MT_BLOCK) {
      const int pr = p0 + it / (cv * 3);
      const int rem = it - (pr - p0) * cv * 3;
      const int c = rem / 3, ch = rem - 3 * c;
      float ax = s_x[ch][pr - oy][c], ay = s_y[ch][pr - oy][c];
      const int ra = max(r0, pr * f), rb = min(r1, pr * f + f);
      for (int r = ra; r < rb; ++r) {
        const int k = r - r0;
        const long long row_e = (img * a.H + r) * a.W + col0;        // first element (pixel) of the run
        const unsigned char* sp = stage + (size_t)k * a.pc_max * 16 + ((row_e * 3 * pe) & 15);
        const unsigned char* sg = stage_g + (size_t)k * a.gc_max * 16 + ((row_e * 3 * ge) & 15);
        float rx = 0.0f, ry = 0.0f;
        for (int j = 0; j < f; ++j) {
          const int e = (c * f + j) * 3 + ch;
          rx += value_at(sp, e, a.pred_u8, a.quantize);
          ry += value_at(sg, e, a.gt_u8, 0);
        }
        ax += rx;
        ay += ry;
      }
      s_x[ch][pr - oy][c] = ax;
      s_y[ch][pr - oy][c] = ay;
    }
  }
  __syncthreads();
  if (f > 1) {
    const float ff = (float)(f * f);
    for (int i = threadIdx.x; i < 3 * MT_R * MT_C; i += MT_BLOCK) {
      (&s_x[0][0][0])[i] /= ff;
      (&s_y[0][0][0])[i] /= ff;
    }
  }

  // 3. per channel: horizontal 11-tap pass of the five moments into LDS, vertical pass + SSIM map in registers
  float* hx = s_h;
  float* hy = s_h + MT_R * MT_TW;
  float* hxx = s_h + 2 * MT_R * MT_TW;
  float* hyy = s_h + 3 * MT_R * MT_TW;
  float* hxy = s_h + 4 * MT_R * MT_TW;
  const int oc = threadIdx.x & (MT_TW - 1), band = threadIdx.x / MT_TW;
  double ss_sum = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    __syncthreads();               // pooling / the previous channel's vertical pass are done with s_h
    for (int i = threadIdx.x; i < MT_R * MT_TW; i += MT_BLOCK) {
      const int r = i / MT_TW, c = i - r * MT_TW;
      float mx = 0.0f, my = 0.0f, mxx = 0.0f, myy = 0.0f, mxy = 0.0f;
#pragma unroll
      for (int k = 0; k < MT_K; ++k) {
        const float x = s_x[ch][r][c + k], y = s_y[ch][r][c + k], g = taps.g[k];
        mx = fmaf(g, x, mx);
        my = fmaf(g, y, my);
        mxx = fmaf(g, x * x, mxx);
        myy = fmaf(g, y * y, myy);
        mxy = fmaf(g, x * y, mxy);
      }
      hx[i] = mx; hy[i] = my; hxx[i] = mxx; hyy[i] = myy; hxy[i] = mxy;
    }
    __syncthreads();
    for (int rr = 0; rr < MT_TH / (MT_BLOCK / MT_TW); ++rr) {
      const int orow = band * (MT_TH / (MT_BLOCK / MT_TW)) + rr;
      float mx = 0.0f, my = 0.0f, mxx = 0.0f, myy = 0.0f, mxy = 0.0f;
#pragma unroll
      for (int k = 0; k < MT_K; ++k) {
        const int i = (orow + k) * MT_TW + oc;
        const float g = taps.g[k];
        mx = fmaf(g, hx[i], mx);
        my = fmaf(g, hy[i], my);
        mxx = fmaf(g, hxx[i], mxx);
        myy = fmaf(g, hyy[i], myy);
        mxy = fmaf(g, hxy[i], mxy);
      }
      const float mx2 = mx * mx, my2 = my * my, mxmy = mx * my;
      const float sxx = mxx - mx2, syy = myy - my2, sxy = mxy - mxmy;
      const float cs = (2.0f * sxy + MT_C2) / (sxx + syy + MT_C2);
      const float ss = (2.0f * mxmy + MT_C1) / (mx2 + my2 + MT_C1) * cs;
      if (oy + orow < a.Ho && ox + oc < a.Wo) ss_sum += (double)ss;
    }
  }

  // 4. the tile's two partials
  const double se_t = block_sum(se, s_part);
  const double ss_t = block_sum(ss_sum, s_part);
  if (threadIdx.x == 0) {
    a.ws[(img * a.tiles + t) * 2] = se_t;
    a.ws[(img * a.tiles + t) * 2 + 1] = ss_t;
  }
}

__global__ __launch_bounds__(MT_BLOCK) void metrics_finish_kernel(const double* __restrict__ ws, int tiles,
                                                                  double n_values, double n_ssim,
                                                                  double* __restrict__ psnr,
                                                                  double* __restrict__ ssim) {
  __shared__ double s_part[MT_BLOCK / 64];
  const double* w = ws + (size_t)blockIdx.x * tiles * 2;
  double se = 0.0, ss = 0.0;
  for (int i = threadIdx.x; i < tiles; i += MT_BLOCK) {
    se += w[2 * i];
    ss += w[2 * i + 1];
  }
  const double se_t = block_sum(se, s_part);
  const double ss_t = block_sum(ss, s_part);
  if (threadIdx.x == 0) {
    psnr[blockIdx.x] = -10.0 * log10(se_t / n_values + 1e-8);
    ssim[blockIdx.x] = ss_t / n_ssim;
  }
}

struct Plan {
  int Hp, Wp, Ho, Wo, tiles_x, tiles, pc_max, gc_max, rows_per_round;
};

// 0, VSA_ERR_ARG or VSA_ERR_UNSUPPORTED
int make_plan(int B, int H, int W, int pool, int pred_u8, int gt_u8, Plan* p) {
  if (B < 1 || H < 1 || W < 1 || pool < 1) return VSA_ERR_ARG;
  if ((pred_u8 != 0 && pred_u8 != 1) || (gt_u8 != 0 && gt_u8 != 1)) return VSA_ERR_ARG;
  p->Hp = H / pool;
  p->Wp = W / pool;
  if (p->Hp < MT_K || p->Wp < MT_K) return VSA_ERR_ARG;    // piq raises for a pooled image under the kernel size
  p->Ho = p->Hp - (MT_K - 1);
  p->Wo = p->Wp - (MT_K - 1);
  p->tiles_x = vsa_div_up(p->Wo, MT_TW);
  p->tiles = p->tiles_x * vsa_div_up(p->Ho, MT_TH);
  const long long run = 3ll * MT_C * pool;                 // values of one full-res row run
  p->pc_max = (int)((run * (pred_u8 ? 1 : 4) + 15) / 16 + 1);
  p->gc_max = (int)((run * (gt_u8 ? 1 : 4) + 15) / 16 + 1);
  p->rows_per_round = MT_STAGE_BYTES / (16 * (p->pc_max + p->gc_max));
  if (p->rows_per_round < 1) return VSA_ERR_UNSUPPORTED;   // one row run of pred + gt exceeds the staging area
  if ((long long)B * p->tiles > 0x7fffffffll) return VSA_ERR_UNSUPPORTED;
  return VSA_OK;
}

}  // namespace

extern "C" long long vsa_image_metrics_workspace_bytes(int B, int H, int W, int pool, int pred_u8, int gt_u8) {
  Plan p;
  const int rc = make_plan(B, H, W, pool, pred_u8, gt_u8, &p);
  if (rc != VSA_OK) return rc;
  return (long long)B * p.tiles * 2 * (long long)sizeof(double);
}

extern "C" int vsa_image_metrics(const void* pred, int pred_u8, const void* gt, int gt_u8, int B, int H, int W,
                                 int pool, int quantize_pred, void* workspace, long long workspace_bytes,
                                 double* psnr_out, double* ssim_out, void* stream) {
  if (!pred || !gt || !workspace || !psnr_out || !ssim_out) return VSA_ERR_ARG;
  if (quantize_pred != 0 && quantize_pred != 1) return VSA_ERR_ARG;
  Plan p;
  const int rc = make_plan(B, H, W, pool, pred_u8, gt_u8, &p);
  if (rc != VSA_OK) return rc;
  if (workspace_bytes < (long long)B * p.tiles * 2 * (long long)sizeof(double)) return VSA_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) & 15) return VSA_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return VSA_ERR_ARG;
  MetricsArgs a;
  a.pred = static_cast<const unsigned char*>(pred);
  a.gt = static_cast<const unsigned char*>(gt);
  const long long n = 3ll * H * W * B;
  a.pred_bytes = n * (pred_u8 ? 1 : 4);
  a.gt_bytes = n * (gt_u8 ? 1 : 4);
  a.pred_u8 = pred_u8;
  a.gt_u8 = gt_u8;
  a.quantize = pred_u8 ? 0 : quantize_pred;
  a.H = H; a.W = W; a.f = pool;
  a.Hp = p.Hp; a.Wp = p.Wp; a.Ho = p.Ho; a.Wo = p.Wo;
  a.tiles_x = p.tiles_x; a.tiles = p.tiles;
  a.pc_max = p.pc_max; a.gc_max = p.gc_max; a.rows_per_round = p.rows_per_round;
  a.ws = static_cast<double*>(workspace);
  // piq's gaussian_filter(11, 1.5): exp(-(i - 5)^2 / (2 sigma^2)), normalised; the 2-D kernel is the outer product
  Taps taps;
  double g[MT_K], sum = 0.0;
  for (int i = 0; i < MT_K; ++i) {
    const double d = i - (MT_K - 1) / 2;
    g[i] = exp(-d * d / (2.0 * 1.5 * 1.5));
    sum += g[i];
  }
  for (int i = 0; i < MT_K; ++i) taps.g[i] = (float)(g[i] / sum);
  hipLaunchKernelGGL(metrics_tile_kernel, dim3(B * p.tiles), dim3(MT_BLOCK), 0, (hipStream_t)stream, a, taps);
  VSA_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(B), dim3(MT_BLOCK), 0, (hipStream_t)stream,
                     static_cast<const double*>(workspace), p.tiles, (double)(3ll * H * W),
                     (double)(3ll * p.Ho * p.Wo), psnr_out, ssim_out);
  VSA_RETURN_LAUNCH_STATUS();
}
