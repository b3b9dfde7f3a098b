// Neural-texture step 5: per-hit shading from the quantised texel rows, forward
// and backward.
//
// Forward, per (ray, shell) hit — the reference's op sequence:
//   4 corner rows per degree -> fp16 range expansion (neural_texture.py:177-185,
//   a 256-entry LUT per degree) -> fp32 lerp (:188-191) -> fp16 SH coefficients
//   (sh_neural_textures.py:88) -> SH evaluation with the view direction
//   (encodings/sphericalharmonics.py:155-229) -> sigmoid (:92) -> alpha decay
//   (methods/volsurfs.py:583-594) -> scatter into surfs_rgb / surfs_alpha
//   (:550, :596).
// Backward: the same chain reversed; gradients w.r.t. the quantised texel value
// o = q/255 are accumulated per slot (f32 rows, per-degree width) with wave-cooperative
// atomics: lanes = the 64 (channel, SH coefficient) pairs of ONE hit, so each
// wave instruction adds contiguous row segments instead of 64 scattered dwords.
#include "nt_shade_common.h"   // launch geometry, hit context, corner rows, SH sums, the shared forward of one ray

namespace {

// Evaluate raw SH sum with the reference's exact order.  y, z, x come in through
// the pre-multiplied basis b[] except for degree 1 where the reference
// multiplies (C1*y)*sh — b[1..3] already carry the sign, so subtraction of
// (C1*y)*sh1 is written as addition of b[1]*sh1 (bit-identical: a - p == a + (-p)).
__device__ __forceinline__ float sh_raw(const float b[16], const float* sh, int degrees) {
  float r = vsa_round_f16(C0 * sh[0]);
  if (degrees > 1) {
    r = r + b[1] * sh[1];
    r = r + b[2] * sh[2];
    r = r + b[3] * sh[3];
    if (degrees > 2) {
#pragma unroll
      for (int m = 4; m < 9; ++m) r = r + b[m] * sh[m];
      if (degrees > 3) {
#pragma unroll
        for (int m = 9; m < 16; ++m) r = r + b[m] * sh[m];
      }
    }
  }
  return r;
}

// SH coefficients (fp16-rounded, as floats): sh_rgb[ch][16], sh_a[16]
template <bool F16ROWS = false>
__device__ __forceinline__ void gather_coeffs(const vsa_nt_plan& plan, const HitCtx& c,
                                              const unsigned* __restrict__ texels,
                                              const float* s_lut, bool has_alpha,
                                              float sh_rgb[3][16], float sh_a[16]) {
#pragma unroll
  for (int d = 0; d < VSA_NT_MAX_DEG; ++d) {
    const int n = 2 * d + 1, m0 = d * d;
    const bool do_rgb = d < plan.rgb_degrees, do_a = has_alpha && d < plan.alpha_degrees;
    if (!do_rgb && !do_a) continue;
    float acc[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) add_corner_row<F16ROWS>(plan, d, texels, c.row[d][k], c.w[d][k], s_lut, acc);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int i = 0; i < n; ++i) sh_rgb[ch][m0 + i] = do_rgb ? vsa_round_f16(acc[ch * n + i]) : 0.f;
#pragma unroll
    for (int i = 0; i < n; ++i) sh_a[m0 + i] = do_a ? vsa_round_f16(acc[21 + i]) : 0.f;
  }
}

#define NT_SHADE_FWD_OCC 3     /* round 3: 4 waves per SIMD (128 VGPRs) gave 0.163 -> 0.152 ms with run-time band counts; with FULL4 the hoisted slot-id loads spill there (0.19) and 3 waves run 0.139 */
template <bool FULL4, bool F16ROWS = false>
__global__ __launch_bounds__(SH_BLOCK, NT_SHADE_FWD_OCC) void nt_shade_fwd_kernel(
    vsa_nt_plan plan, const int* __restrict__ hit_slot, const float* __restrict__ tex_uv,
    const float* __restrict__ rays_d, const float4* __restrict__ tris,
    const int* __restrict__ slot_of, const int* __restrict__ seg_start,
    const unsigned* __restrict__ texels, int N, float* __restrict__ surfs_rgb, float* __restrict__ surfs_alpha,
    float* __restrict__ surfs_normals, float* __restrict__ coeffs_out,
    float4* __restrict__ act_out) {
  __shared__ float s_lut[VSA_NT_MAX_DEG * 256];
  build_lut(plan, s_lut);
  __syncthreads();
  const int K = plan.nr_shells;
  const ShadeIdx wi = shade_idx(K, (N + SH_BLOCK - 1) / SH_BLOCK);      // (shell, ray tile), XCD-aware: see shade_idx
  const long long n = wi.tile * SH_BLOCK + threadIdx.x;
  const int s = wi.shell;
  if (!wi.valid) return;
  if (n >= N) return;
  nt_shade_ray<FULL4>(plan, s, n, N, hit_slot, tex_uv, rays_d, tris, slot_of, seg_start, surfs_rgb, surfs_alpha,
                      surfs_normals, coeffs_out, act_out, RowSums<F16ROWS>{plan, texels, s_lut});
}

// ---------------------------------------------------------------- backward
// Per hit: g_raw[4] (3 rgb + alpha, through the output sigmoid and the decay) and
// the 16 SH basis values; then lanes = 64 (channel, coefficient) pairs of one
// hit at a time add  span_d * w_corner * g_raw[ch] * basis[m]  to the slot rows.
// RECOMPUTE = false: the caller hands back the forward pass's sigmoids (act_in) and phase 1
// is a handful of loads; RECOMPUTE = true re-gathers the texel rows.  The per-hit record
// that phase 2 reads is 39 dwords (4 g_raw, 16 basis, 2 row ids + 2 lerp fractions per band)
// so that a 128-thread workgroup needs 20 KiB of LDS and 16 waves fit a CU: halving the
// occupancy of this atomic-bound kernel cost 27 % (measured), i.e. it is latency-sensitive.
constexpr int SHB_BLOCK = 128;

// no-return packed f16 add at the memory side (global_atomic_pk_add_f16: one dword per lane)
// (uniform base + 32-bit byte offset: the buffer is far below 4 GiB)
__device__ __forceinline__ void atomic_pk_add_f16(const _Float16* base, unsigned byte_off, float a, float b) {
  const half2_t v = {(_Float16)a, (_Float16)b};
  asm volatile("global_atomic_pk_add_f16 %0, %1, %2" ::"v"(byte_off), "v"(__builtin_bit_cast(unsigned, v)), "s"(base) : "memory");
}

#define NT_SHADE_BWD_OCC 4
template <bool RECOMPUTE, bool FULL4, bool F16ROWS = false>
__global__ __launch_bounds__(SHB_BLOCK, RECOMPUTE ? 2 : NT_SHADE_BWD_OCC) void nt_shade_bwd_kernel(
    vsa_nt_plan plan, const int* __restrict__ hit_slot, const float* __restrict__ tex_uv,
    const float* __restrict__ rays_d, const float4* __restrict__ tris,
    const int* __restrict__ slot_of, const int* __restrict__ seg_start,
    const unsigned* __restrict__ texels, int N, const float* __restrict__ g_surfs_rgb,
    const float* __restrict__ g_surfs_alpha, float grad_scale, _Float16* __restrict__ grad_rows,
    const float4* __restrict__ act_in) {
  __shared__ float s_lut[RECOMPUTE ? VSA_NT_MAX_DEG * 256 : 1];
  __shared__ float s_graw[SHB_BLOCK][4];
  __shared__ float s_basis[SHB_BLOCK][17];
  __shared__ int s_row[SHB_BLOCK][9];    // corners (x0,y0) and (x0,y1) per band; x1 = the next slot's row
  __shared__ float s_f[SHB_BLOCK][9];
  if (RECOMPUTE) {
    build_lut(plan, s_lut);
    __syncthreads();
  }
  const int K = plan.nr_shells;
  const ShadeIdx wi = shade_idx(K, (N + SHB_BLOCK - 1) / SHB_BLOCK);    // as in the forward: the reads of g_surfs_* share lines
  const long long n = wi.valid ? wi.tile * SHB_BLOCK + threadIdx.x : (long long)N;
  const int s = wi.shell;
  const int t = threadIdx.x;
  HitCtx c;
  c.hit = false;
  float nrm[3];
  const bool has_alpha = nt_shell_has_alpha(plan, s);
  if (n < N && load_ctx<FULL4>(plan, s, n, N, hit_slot, tex_uv, rays_d, tris, slot_of, seg_start, c, nrm)) {
    float b[16];
    sh_basis(c.dir[0], c.dir[1], c.dir[2], b);
    const long long o = n * K + s;
    float sg4[4];
    if (!RECOMPUTE) {   // the forward pass kept its four sigmoids: no texel gather, no SH sums
      const float4 a = act_in[(long long)s * N + n];
      sg4[0] = a.x, sg4[1] = a.y, sg4[2] = a.z, sg4[3] = a.w;
    } else {
      float sh_rgb[3][16], sh_a[16];
      gather_coeffs<F16ROWS>(plan, c, texels, s_lut, has_alpha, sh_rgb, sh_a);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) sg4[ch] = sigmoidf_(sh_raw(b, sh_rgb[ch], plan.rgb_degrees));
      sg4[3] = has_alpha ? sigmoidf_(sh_raw(b, sh_a, plan.alpha_degrees)) : 0.f;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float sg = sg4[ch];
      s_graw[t][ch] = g_surfs_rgb[3 * o + ch] * sg * (1.0f - sg) * grad_scale;
    }
    float ga = 0.f;
    if (has_alpha) {
      const float sg = sg4[3];
      ga = g_surfs_alpha[o] * c.decay * sg * (1.0f - sg) * grad_scale;
    }
    s_graw[t][3] = ga;
#pragma unroll
    for (int m = 0; m < 16; ++m) s_basis[t][m] = b[m];
#pragma unroll
    for (int d = 0; d < VSA_NT_MAX_DEG; ++d) {
      // slots are numbered in domain order and all four corners are marked, so the x1
      // corner is always the slot right after the x0 corner
      s_row[t][2 * d] = c.row[d][0];
      s_row[t][2 * d + 1] = c.row[d][2];
      s_f[t][2 * d] = c.fx[d];
      s_f[t][2 * d + 1] = c.fy[d];
    }
  }
  // per-wave cooperative scatter (no workgroup barrier needed: each wave reads
  // only what its own lanes wrote).  The memory-side atomic path is bound by its 64-byte
  // REQUESTS (PMC: 18 G requests/s whatever their fill), so the unit of accumulation is the
  // 64-byte LINE of gradient rows, not the row: a lane owns one PAIR of adjacent f16 elements
  // at a fixed position of a line (one global_atomic_pk_add_f16 per flush) —
  //   degree 0: 16-B rows, 4 slots per line x 3 pairs   (lanes  0..11)
  //   degree 1: 32-B rows, 2 slots per line x 7 pairs   (lanes 12..25)
  //   degree 2: 64-B rows, 11 pairs                      (lanes 26..36)
  //   degree 3: 64-B rows, 15 pairs                      (lanes 37..51)
  // (pairs of a row: ceil(3 nn / 2) rgb + ceil(nn / 2) alpha, nn = 2d + 1; an odd tail pairs
  // with a padding element and adds zero to it.)
  const int lane = t & 63, wbase = t & ~63;
  const unsigned long long hits = __ballot(c.hit);
  const int d = lane < 12 ? 0 : (lane < 26 ? 1 : (lane < 37 ? 2 : 3));
  const int lb = lane - (d == 0 ? 0 : (d == 1 ? 12 : (d == 2 ? 26 : 37)));
  const int nn = 2 * d + 1, n_rgb_pairs = (3 * nn + 1) >> 1, row_pairs = n_rgb_pairs + ((nn + 1) >> 1);
  // (small unsigned divisions by multiply-high: the generic sequence is ~25 instructions each)
  const unsigned magic3 = 0x55555556u, magic5 = 0x33333334u, magic7 = 0x24924925u;   // 2^32 / n + 1
  const unsigned magic_nn = d == 1 ? magic3 : (d == 2 ? magic5 : magic7);
  auto div_nn = [&](int x) { return d == 0 ? x : (int)__umulhi((unsigned)x, magic_nn); };
  const int q = d == 0 ? (int)__umulhi((unsigned)lb, magic3) : (d == 1 ? (int)__umulhi((unsigned)lb, magic7) : 0);
  const int jb = lb - q * row_pairs;                                  // q: slot within the line, jb: pair within the row
  const bool is_alpha = jb >= n_rgb_pairs;
  const int e0 = is_alpha ? 2 * (jb - n_rgb_pairs) : 2 * jb;          // element index within the part
  const int part = is_alpha ? nn : 3 * nn;
  const int qd = nt_row_quads(d), qsh = d == 0 ? 1 : (d == 1 ? 2 : 3);
  // position of the pair in its line, in halfs (even: a 4-byte aligned f16 pair)
  const int lofs = 4 * (q * qd + (is_alpha ? nt_alpha_quad(d) : 0)) + e0;
  const bool band_on = lane < 52 && (is_alpha ? (has_alpha && d < alpha_degs<FULL4>(plan)) : d < rgb_degs<FULL4>(plan));
  const bool on1 = band_on && e0 + 1 < part;
  const int c0 = div_nn(e0), c1 = div_nn(e0 + 1);
  const int ch0 = is_alpha ? 3 : c0, ch1 = is_alpha ? 3 : c1;
  const int m0 = d * d + (is_alpha ? e0 : e0 - c0 * nn), m1 = on1 ? d * d + (is_alpha ? e0 + 1 : e0 + 1 - c1 * nn) : 0;
  float span = plan.row_format == 2 ? 1.0f : plan.sh_span[d];     // (raw rows: d row / d output = 1)
  // `d` differs per lane, so this is a VECTOR load from the kernel-argument segment; its first use
  // is inside the hit loop below, and the compiler put the `s_waitcnt vmcnt(0)` for it THERE — where,
  // on every trip, it also waited for every gradient atomic the wave had in flight (no-return
  // atomics stay counted in vmcnt until the memory side acknowledges them: ~1-3 k cycles).  Using
  // the value once here retires the load in front of the loop.
  asm volatile("" : "+v"(span));
  // Consecutive hits of a wave are neighbouring pixels: their 2x2 footprints fall on the same
  // or on neighbouring lines.  Each lane keeps up to four lines open with a running sum (the
  // lines the previous footprint touched: {x0, x1} x {y0, y1}, fewer when corners share a
  // line); a line of the new footprint that matches ANY open line inherits its sum, and only
  // lines the new footprint no longer touches are flushed — all lanes of a degree take the
  // same decisions, so a flush is ONE request for the whole line.
  // (the pair's two running sums travel as one float2: v_pk_mul / v_pk_fma_f32, and the
  // "inherit if same line" select is an fma with a 1.0 / 0.0 factor — the loop is VALU-bound)
  typedef float float2_t __attribute__((ext_vector_type(2)));
  int cur[4] = {-1, -1, -1, -1};
  float2_t acc[4] = {float2_t(0.f), float2_t(0.f), float2_t(0.f), float2_t(0.f)};
  const unsigned lofs_b = 2u * (unsigned)lofs;
  unsigned long long rem = hits;
  // the eight LDS values a lane needs of a hit are read one hit ahead of their use
  struct HitIn { float g0, g1, b0, b1, fx, fy; int r0, r1; };
  auto fetch = [&](int ht) {
    HitIn r;
    r.g0 = s_graw[ht][ch0], r.g1 = s_graw[ht][ch1], r.b0 = s_basis[ht][m0], r.b1 = s_basis[ht][m1];
    r.fx = s_f[ht][2 * d], r.fy = s_f[ht][2 * d + 1];
    r.r0 = s_row[ht][2 * d], r.r1 = s_row[ht][2 * d + 1];
    return r;
  };
  HitIn nx = fetch(wbase + (rem ? __ffsll((long long)rem) - 1 : 0));
  while (rem) {
    const int hl = __ffsll((long long)rem) - 1;
    rem &= rem - 1;
    const HitIn cu = nx;
    nx = fetch(wbase + (rem ? __ffsll((long long)rem) - 1 : hl));
    if (band_on) {
      float2_t gg;
      gg.x = cu.g0 * cu.b0;
      gg.y = on1 ? cu.g1 * cu.b1 : 0.f;
      const float fx = cu.fx, fy = cu.fy;
      // the lerp weights exactly as load_ctx forms them, then x span, then x g
      const float w[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
      int sl[4];
      float wl[4];
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        const int ra = y ? cu.r1 : cu.r0, rb = ra + qd;              // the x0 and x1 corner rows (quads)
        const int la = ra >> 3, lbn = rb >> 3;                        // their lines (8 quads of 8 B)
        const bool ma = q == ((ra & 7) >> qsh), mb = q == ((rb & 7) >> qsh), one = la == lbn;
        sl[2 * y] = la;
        wl[2 * y] = ma ? w[2 * y] : ((one && mb) ? w[2 * y + 1] : 0.f);
        sl[2 * y + 1] = one ? -1 : lbn;
        wl[2 * y + 1] = (!one && mb) ? w[2 * y + 1] : 0.f;
      }
      // the y1 corners may sit on a line of the y0 corners (sparsely marked regions): rare,
      // so the fold is behind a wave-uniform test
      const bool dup = sl[2] == sl[0] || sl[2] == sl[1] || ((sl[3] == sl[0] || sl[3] == sl[1]) && sl[3] >= 0);
      if (__builtin_expect(__ballot(dup) != 0ull, 0)) {
#pragma unroll
        for (int k = 2; k < 4; ++k)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            if (sl[k] == sl[i] && sl[k] >= 0) {
              wl[i] += wl[k];
              wl[k] = 0.f;
              sl[k] = -1;
            }
      }
      float2_t v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = float2_t(wl[k] * span) * gg;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bool kept = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool same = cur[j] == sl[k];
          v[k] = __builtin_elementwise_fma(acc[j], float2_t(same ? 1.0f : 0.0f), v[k]);
          kept |= same;
        }
        if (!kept && cur[j] >= 0) atomic_pk_add_f16(grad_rows, (unsigned)cur[j] * 64u + lofs_b, acc[j].x, acc[j].y);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        cur[k] = sl[k];
        acc[k] = v[k];
      }
    }
  }
  if (band_on) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (cur[k] >= 0) atomic_pk_add_f16(grad_rows, (unsigned)cur[k] * 64u + lofs_b, acc[k].x, acc[k].y);
  }
}

}  // namespace

extern "C" int vsa_nt_shade_fwd(const vsa_nt_plan* plan, const int32_t* hit_slot,
                                const float* tex_uv, const float* rays_d, const float* tris,
                                const int32_t* slot_of, const int32_t* seg_start,
                                const uint8_t* texels, int nr_rays, float* surfs_rgb,
                                float* surfs_alpha, float* surfs_normals, float* coeffs_out,
                                float* act_out, void* stream) {
  if (!plan || nr_rays < 0) return VSA_ERR_ARG;
  if (nr_rays == 0) return VSA_OK;
  if (!hit_slot || !tex_uv || !rays_d || !tris || !slot_of || !seg_start || !texels || !surfs_rgb ||
      !surfs_alpha)
    return VSA_ERR_ARG;
  if (plan->row_format < 0 || plan->row_format > 2) return VSA_ERR_UNSUPPORTED;
  dim3 grid = shade_grid(vsa_div_up(nr_rays, SH_BLOCK), plan->nr_shells);
  if (plan->row_format != 0)          // f16 rows (using_sh_quantization = 0): the generic-band-count kernel
    hipLaunchKernelGGL((nt_shade_fwd_kernel<false, true>), grid, dim3(SH_BLOCK), 0, (hipStream_t)stream, *plan,
                       hit_slot, tex_uv, rays_d, reinterpret_cast<const float4*>(tris), slot_of,
                       seg_start, reinterpret_cast<const unsigned*>(texels), nr_rays, surfs_rgb,
                       surfs_alpha, surfs_normals, coeffs_out, reinterpret_cast<float4*>(act_out));
  else if (plan->rgb_degrees == VSA_NT_MAX_DEG && plan->alpha_degrees == VSA_NT_MAX_DEG)
    hipLaunchKernelGGL(nt_shade_fwd_kernel<true>, grid, dim3(SH_BLOCK), 0, (hipStream_t)stream, *plan,
                       hit_slot, tex_uv, rays_d, reinterpret_cast<const float4*>(tris), slot_of,
                       seg_start, reinterpret_cast<const unsigned*>(texels), nr_rays, surfs_rgb,
                       surfs_alpha, surfs_normals, coeffs_out, reinterpret_cast<float4*>(act_out));
  else
    hipLaunchKernelGGL(nt_shade_fwd_kernel<false>, grid, dim3(SH_BLOCK), 0, (hipStream_t)stream, *plan,
                       hit_slot, tex_uv, rays_d, reinterpret_cast<const float4*>(tris), slot_of,
                       seg_start, reinterpret_cast<const unsigned*>(texels), nr_rays, surfs_rgb,
                       surfs_alpha, surfs_normals, coeffs_out, reinterpret_cast<float4*>(act_out));
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_nt_shade_bwd(const vsa_nt_plan* plan, const int32_t* hit_slot,
                                const float* tex_uv, const float* rays_d, const float* tris,
                                const int32_t* slot_of, const int32_t* seg_start,
                                const uint8_t* texels, int nr_rays, const float* g_surfs_rgb,
                                const float* g_surfs_alpha, float grad_scale, uint16_t* grad_rows,
                                const float* act_in, void* stream) {
  if (!plan || nr_rays < 0) return VSA_ERR_ARG;
  if (nr_rays == 0) return VSA_OK;
  if (!hit_slot || !tex_uv || !rays_d || !tris || !slot_of || !seg_start || !texels || !g_surfs_rgb ||
      !g_surfs_alpha || !grad_rows)
    return VSA_ERR_ARG;
  if (plan->row_base[VSA_MAX_SHELLS * VSA_NT_MAX_DEG] * 8 >= (1ll << 32)) return VSA_ERR_UNSUPPORTED;   // 32-bit atomic offsets
  if (plan->row_format < 0 || plan->row_format > 2) return VSA_ERR_UNSUPPORTED;
  dim3 grid = shade_grid(vsa_div_up(nr_rays, SHB_BLOCK), plan->nr_shells);
  const bool full4 = plan->rgb_degrees == VSA_NT_MAX_DEG && plan->alpha_degrees == VSA_NT_MAX_DEG;
  if (act_in && full4)
    hipLaunchKernelGGL((nt_shade_bwd_kernel<false, true>), grid, dim3(SHB_BLOCK), 0, (hipStream_t)stream, *plan,
                       hit_slot, tex_uv, rays_d, reinterpret_cast<const float4*>(tris), slot_of,
                       seg_start, reinterpret_cast<const unsigned*>(texels), nr_rays, g_surfs_rgb,
                       g_surfs_alpha, grad_scale, reinterpret_cast<_Float16*>(grad_rows),
                       reinterpret_cast<const float4*>(act_in));
  else if (act_in)
    hipLaunchKernelGGL((nt_shade_bwd_kernel<false, false>), grid, dim3(SHB_BLOCK), 0, (hipStream_t)stream, *plan,
                       hit_slot, tex_uv, rays_d, reinterpret_cast<const float4*>(tris), slot_of,
                       seg_start, reinterpret_cast<const unsigned*>(texels), nr_rays, g_surfs_rgb,
                       g_surfs_alpha, grad_scale, reinterpret_cast<_Float16*>(grad_rows),
                       reinterpret_cast<const float4*>(act_in));
  else if (plan->row_format != 0)     // no kept sigmoids: re-gather the f16 rows
    hipLaunchKernelGGL((nt_shade_bwd_kernel<true, false, true>), grid, dim3(SHB_BLOCK), 0, (hipStream_t)stream, *plan,
                       hit_slot, tex_uv, rays_d, reinterpret_cast<const float4*>(tris), slot_of,
                       seg_start, reinterpret_cast<const unsigned*>(texels), nr_rays, g_surfs_rgb,
                       g_surfs_alpha, grad_scale, reinterpret_cast<_Float16*>(grad_rows), nullptr);
  else
    hipLaunchKernelGGL((nt_shade_bwd_kernel<true, false>), grid, dim3(SHB_BLOCK), 0, (hipStream_t)stream, *plan,
                       hit_slot, tex_uv, rays_d, reinterpret_cast<const float4*>(tris), slot_of,
                       seg_start, reinterpret_cast<const unsigned*>(texels), nr_rays, g_surfs_rgb,
                       g_surfs_alpha, grad_scale, reinterpret_cast<_Float16*>(grad_rows), nullptr);
  VSA_RETURN_LAUNCH_STATUS();
}
