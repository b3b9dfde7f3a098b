// What the per-hit shading kernels share: nt_shade.hip (vsa_nt_shade_fwd / _bwd, from the texel rows) and
// texture_mip.hip (vsa_nt_shade_mip_fwd, the same shade with footprint-filtered coefficients).  One text for the launch
// geometry, the hit context, the expand LUT, the corner-row lerp, the SH sums, the sigmoids, the alpha decay and the
// dense scatter: the kernels differ only in where a band's 28 lerp sums come from (nt_shade_ray's `sums`).
#pragma once
#include "nt_common.h"

// Launch geometry of the shading kernels: a workgroup = (one shell, one tile of consecutive rays).
// 1-D grid, XCD-aware — workgroups are dealt to the 8 XCDs round-robin by their linear id, so (tile t, shell s) gets
// id = ((t / 8) * K + s) * 8 + t % 8: the K workgroups of one tile run on ONE XCD, back to back, and their K partial
// writes into the tile's [N,K,3] / [N,K] lines (12 and 4 bytes at a stride of 12 K and 4 K) merge in that XCD's L2
// before they leave it.  (A (shell, tile) grid put the K workgroups on K different XCDs, each L2 writing its partial
// line back by itself: at 1920x1080, K = 7 the launch wrote 0.98 GB for 0.30 GB of outputs; a (tile, shell) grid
// 1.22 GB.)
struct ShadeIdx {
  long long tile;
  int shell;
  bool valid;
};
__device__ __forceinline__ ShadeIdx shade_idx(int K, int tiles) {
  const unsigned id = blockIdx.x, x = id & 7u, q = id >> 3;
  const unsigned s = q % (unsigned)K, tg = q / (unsigned)K;
  const long long t = (long long)tg * 8 + x;
  return {t, (int)s, t < tiles};
}
static inline dim3 shade_grid(int tiles, int shells) {
  return dim3((unsigned)(((tiles + 7) / 8) * 8 * shells));
}

namespace {

constexpr int SH_BLOCK = 256;

constexpr float C0 = 0.28209479177387814f;
constexpr float C1 = 0.4886025119029199f;
constexpr float C2_0 = 1.0925484305920792f, C2_1 = -1.0925484305920792f,
                C2_2 = 0.31539156525252005f, C2_3 = -1.0925484305920792f,
                C2_4 = 0.5462742152960396f;
constexpr float C3_0 = -0.5900435899266435f, C3_1 = 2.890611442640554f,
                C3_2 = -0.4570457994644658f, C3_3 = 0.3731763325901154f,
                C3_4 = -0.4570457994644658f, C3_5 = 1.445305721320277f,
                C3_6 = -0.5900435899266435f;

// SH basis factors exactly as SHEncoder.eval forms them (left-to-right fp32
// products; index 0 is applied in fp16 and handled by the caller).
__device__ __forceinline__ void sh_basis(float x, float y, float z, float b[16]) {
  b[0] = C0;
  b[1] = -(C1 * y);
  b[2] = C1 * z;
  b[3] = -(C1 * x);
  const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  b[4] = C2_0 * xy;
  b[5] = C2_1 * yz;
  b[6] = C2_2 * ((2.0f * zz - xx) - yy);
  b[7] = C2_3 * xz;
  b[8] = C2_4 * (xx - yy);
  b[9] = (C3_0 * y) * (3.0f * xx - yy);
  b[10] = (C3_1 * xy) * z;
  b[11] = (C3_2 * y) * ((4.0f * zz - xx) - yy);
  b[12] = (C3_3 * z) * ((2.0f * zz - 3.0f * xx) - 3.0f * yy);
  b[13] = (C3_4 * x) * ((4.0f * zz - xx) - yy);
  b[14] = (C3_5 * z) * (xx - yy);
  b[15] = (C3_6 * x) * (xx - 3.0f * yy);
}

struct HitCtx {
  bool hit;
  float dir[3];
  float decay;        // alpha decay factor (1 when disabled)
  int row[VSA_NT_MAX_DEG][4];   // first quad of each corner's texel / gradient row
  float w[VSA_NT_MAX_DEG][4];
  float fx[VSA_NT_MAX_DEG], fy[VSA_NT_MAX_DEG];   // lerp fractions (w = products of these)
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

__device__ __forceinline__ void build_lut(const vsa_nt_plan& plan, float* s_lut) {
  // expand_lut (oracle) : fp16(lo + fp16(span * fp16(q/255)))
  for (int i = threadIdx.x; i < VSA_NT_MAX_DEG * 256; i += blockDim.x) {
    const int d = i >> 8, q = i & 255;
    const float o = vsa_round_f16((float)q / 255.0f);
    const float t = vsa_round_f16(plan.sh_span[d] * o);
    s_lut[i] = vsa_round_f16(plan.sh_lo[d] + t);
  }
}

// FULL4: both texture types carry all four SH bands (the shipped configuration, base_5.cfg:12-20):
// the band counts become compile-time constants, so the per-band `if (d >= D) continue` branches go
// and the compiler issues the slot-id loads of all four bands together — with the run-time counts
// every band was its own load -> wait round (four dependent memory latencies in a kernel that PMC
// shows waiting 74 % of its wave cycles).
template <bool FULL4>
__device__ __forceinline__ int rgb_degs(const vsa_nt_plan& p) { return FULL4 ? VSA_NT_MAX_DEG : p.rgb_degrees; }
template <bool FULL4>
__device__ __forceinline__ int alpha_degs(const vsa_nt_plan& p) { return FULL4 ? VSA_NT_MAX_DEG : p.alpha_degrees; }

template <bool FULL4 = false>
__device__ __forceinline__ bool load_ctx(const vsa_nt_plan& plan, int s, long long n, int N,
                                         const int* hit_slot, const float* tex_uv,
                                         const float* rays_d, const float4* tris,
                                         const int* slot_of, const int* seg_start, HitCtx& c,
                                         float nrm[3]) {
  const long long o = (long long)s * N + n;
  const int tslot = hit_slot[o];
  c.hit = tslot >= 0;
  nrm[0] = nrm[1] = nrm[2] = 0.f;
  if (!c.hit) return false;
  c.dir[0] = rays_d[3 * n];
  c.dir[1] = rays_d[3 * n + 1];
  c.dir[2] = rays_d[3 * n + 2];
  const float4 e1 = tris[3 * (long long)tslot + 1], e2 = tris[3 * (long long)tslot + 2];
  const float cx = e1.y * e2.z - e1.z * e2.y, cy = e1.z * e2.x - e1.x * e2.z,
              cz = e1.x * e2.y - e1.y * e2.x;
  const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
  const float inv = len > 0.f ? 1.0f / len : 0.f;
  nrm[0] = cx * inv;
  nrm[1] = cy * inv;
  nrm[2] = cz * inv;
  c.decay = 1.0f;
  if (plan.with_alpha_decay) {
    float dot = ((-c.dir[0]) * nrm[0] + (-c.dir[1]) * nrm[1]) + (-c.dir[2]) * nrm[2];
    dot = fminf(fmaxf(dot, 0.0f), 1.0f);
    c.decay = sigmoidf_(10.0f * dot) * 2.0f - 1.0f;
  }
  const float u = tex_uv[2 * o], v = tex_uv[2 * o + 1];
  const int D = max(rgb_degs<FULL4>(plan), alpha_degs<FULL4>(plan));
#pragma unroll
  for (int d = 0; d < VSA_NT_MAX_DEG; ++d) {   // static indices: the arrays stay in registers
    if (d >= D) {
#pragma unroll
      for (int k = 0; k < 4; ++k) c.row[d][k] = 0, c.w[d][k] = 0.f;
      c.fx[d] = c.fy[d] = 0.f;
      continue;
    }
    const int R = plan.tex_res[d], W = R + 2;
    const bool anchor = plan.anchor != 0;
    const NtFootprint f = nt_footprint(u, v, R, anchor);
    const long long base = plan.dom_off[s * VSA_NT_MAX_DEG + d] + (long long)(f.j0 + 1) * W + (f.i0 + 1);
    const int sd = s * VSA_NT_MAX_DEG + d;
    const int rb = (int)plan.row_base[sd] - seg_start[sd] * nt_row_quads(d);
    c.row[d][0] = rb + slot_of[base] * nt_row_quads(d);
    // anchor: only that texel is marked (slot_of is valid for marked texels only): the three other
    // "corners" are the same row with weight 0
    c.row[d][1] = anchor ? c.row[d][0] : rb + slot_of[base + 1] * nt_row_quads(d);
    c.row[d][2] = anchor ? c.row[d][0] : rb + slot_of[base + W] * nt_row_quads(d);
    c.row[d][3] = anchor ? c.row[d][0] : rb + slot_of[base + W + 1] * nt_row_quads(d);
    c.fx[d] = f.fx;
    c.fy[d] = f.fy;
    c.w[d][0] = (1.0f - f.fx) * (1.0f - f.fy);
    c.w[d][1] = f.fx * (1.0f - f.fy);
    c.w[d][2] = (1.0f - f.fx) * f.fy;
    c.w[d][3] = f.fx * f.fy;
  }
  return true;
}

// One corner row of band d added into the band's 28 lerp sums (3 n colour + n alpha at 21).  F16ROWS = false: the
// 8-bit quantised row through the expand LUT; true (row_format 1): f16 sigmoid values, expanded as the reference
// does in half arithmetic — fl16(lo + fl16(span * o)) (neural_texture.py:183-187) — a quad being 4 halves (8 bytes).
template <bool F16ROWS>
__device__ __forceinline__ void add_corner_row(const vsa_nt_plan& plan, int d, const unsigned* __restrict__ texels,
                                               int row, float wk, const float* s_lut, float acc[28]) {
  const int n = 2 * d + 1;
  if constexpr (!F16ROWS) {
    unsigned wds[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned* rp = texels + row;
    if (d == 0) {
      const uint2 v = *reinterpret_cast<const uint2*>(rp);
      wds[0] = v.x, wds[1] = v.y;
    } else {
      const uint4 lo = *reinterpret_cast<const uint4*>(rp);
      wds[0] = lo.x, wds[1] = lo.y, wds[2] = lo.z, wds[3] = lo.w;
      if (d >= 2) {
        const uint4 hi = *reinterpret_cast<const uint4*>(rp + 4);
        wds[4] = hi.x, wds[5] = hi.y, wds[6] = hi.z, wds[7] = hi.w;
      }
    }
#pragma unroll
    for (int i = 0; i < 3 * n; ++i) {
      const unsigned q = (wds[i >> 2] >> (8 * (i & 3))) & 255u;
      acc[i] = acc[i] + s_lut[d * 256 + q] * wk;
    }
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const unsigned q = (wds[nt_alpha_quad(d) + (i >> 2)] >> (8 * (i & 3))) & 255u;
      acc[21 + i] = acc[21 + i] + s_lut[d * 256 + q] * wk;
    }
  } else {
    unsigned wds[16];
    const uint4* rp = reinterpret_cast<const uint4*>(texels + 2 * (long long)row);     // quad = 2 dwords
    const int nv = d == 0 ? 1 : d == 1 ? 2 : 4;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const uint4 x = v < nv ? rp[v] : make_uint4(0, 0, 0, 0);
      wds[4 * v] = x.x, wds[4 * v + 1] = x.y, wds[4 * v + 2] = x.z, wds[4 * v + 3] = x.w;
    }
    const float lo = plan.sh_lo[d], span = plan.sh_span[d];
    const bool raw = plan.row_format == 2;     // using_sh_squeezing = 0: the row is the network output, no expansion (:181-187)
    auto expand = [&](int elem) {
      const unsigned short hb = (unsigned short)(wds[elem >> 1] >> (16 * (elem & 1)));
      const float o = (float)__builtin_bit_cast(_Float16, hb);
      return raw ? o : vsa_round_f16(lo + vsa_round_f16(vsa_pin_f32(span * o)));
    };
#pragma unroll
    for (int i = 0; i < 3 * n; ++i) acc[i] = acc[i] + expand(i) * wk;
#pragma unroll
    for (int i = 0; i < n; ++i) acc[21 + i] = acc[21 + i] + expand(4 * nt_alpha_quad(d) + i) * wk;
  }
}

// Forward of one hit, one SH band at a time: the band's 28 sums (sums(d, acc): 3 n colour + n alpha at 21; from the
// texel rows, its 4 corner rows expanded and lerped) are rounded to fp16 (gather_coeffs's arithmetic), then added to
// the raw SH sums in coefficient order — the same additions sh_raw performs, so the result is bit-identical, but only
// one band's coefficients are live (the all-bands-first form needed 197 VGPRs = two waves per
// SIMD on a kernel that PMC shows waiting on gathers: 16 % VALU-busy).
template <bool FULL4 = false, class Sums>
__device__ __forceinline__ void shade_hit(const vsa_nt_plan& plan, const HitCtx& c, bool has_alpha, const float b[16],
                                          float raw[4], float* __restrict__ coeffs_out, const Sums& sums) {
  raw[0] = raw[1] = raw[2] = raw[3] = 0.f;
#pragma unroll
  for (int d = 0; d < VSA_NT_MAX_DEG; ++d) {
    const int n = 2 * d + 1, m0 = d * d;
    const bool do_rgb = d < rgb_degs<FULL4>(plan), do_a = has_alpha && d < alpha_degs<FULL4>(plan);
    if (!do_rgb && !do_a) {
      if (coeffs_out) {
#pragma unroll
        for (int i = 0; i < n; ++i)
          coeffs_out[m0 + i] = coeffs_out[16 + m0 + i] = coeffs_out[32 + m0 + i] = coeffs_out[48 + m0 + i] = 0.f;
      }
      continue;
    }
    float acc[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0.f;
    sums(d, c, acc);
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const bool on = ch < 3 ? do_rgb : do_a;
#pragma unroll
      for (int i = 0; i < n; ++i) {
        const int m = m0 + i;
        const float shv = on ? vsa_round_f16(ch < 3 ? acc[ch * n + i] : acc[21 + i]) : 0.f;
        if (coeffs_out) coeffs_out[ch * 16 + m] = shv;
        if (on) raw[ch] = m == 0 ? vsa_round_f16(C0 * shv) : raw[ch] + b[m] * shv;
      }
    }
  }
}

// The four corner rows of band d from the texel rows: what vsa_nt_shade_fwd shades from, and level 0 of the mip shade.
template <bool F16ROWS>
__device__ __forceinline__ void row_sums(const vsa_nt_plan& plan, int d, const HitCtx& c,
                                         const unsigned* __restrict__ texels, const float* s_lut, float acc[28]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) add_corner_row<F16ROWS>(plan, d, texels, c.row[d][k], c.w[d][k], s_lut, acc);
}
template <bool F16ROWS>
struct RowSums {
  const vsa_nt_plan& plan;
  const unsigned* __restrict__ texels;
  const float* s_lut;
  __device__ __forceinline__ void operator()(int d, const HitCtx& c, float acc[28]) const {
    row_sums<F16ROWS>(plan, d, c, texels, s_lut, acc);
  }
};

// One (ray n, shell s) of a forward shade: the hit context, the SH sums over sums(d, c, acc), the sigmoids, the alpha
// decay and the scatter into the dense outputs (zero on a miss).
template <bool FULL4, class Sums>
__device__ __forceinline__ void nt_shade_ray(const vsa_nt_plan& plan, int s, long long n, int N,
                                             const int* hit_slot, const float* tex_uv,
                                             const float* rays_d, const float4* tris,
                                             const int* slot_of, const int* seg_start,
                                             float* surfs_rgb, float* surfs_alpha,
                                             float* surfs_normals, float* coeffs_out,
                                             float4* act_out, const Sums& sums) {
  const int K = plan.nr_shells;
  HitCtx c;
  float nrm[3];
  float rgb[3] = {0.f, 0.f, 0.f}, alpha = 0.f;
  float4 act = make_float4(0.f, 0.f, 0.f, 0.f);   // the four sigmoids, for the backward pass
  if (load_ctx<FULL4>(plan, s, n, N, hit_slot, tex_uv, rays_d, tris, slot_of, seg_start, c, nrm)) {
    const bool has_alpha = nt_shell_has_alpha(plan, s);
    float b[16], raw[4];
    sh_basis(c.dir[0], c.dir[1], c.dir[2], b);
    shade_hit<FULL4>(plan, c, has_alpha, b, raw, coeffs_out ? coeffs_out + ((long long)s * N + n) * 64 : nullptr, sums);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float sg = sigmoidf_(raw[ch]);
      (ch == 0 ? act.x : ch == 1 ? act.y : act.z) = sg;
      rgb[ch] = rgb_degs<FULL4>(plan) > 1 ? sg : vsa_round_f16(sg);
    }
    if (has_alpha) {
      const float sg = sigmoidf_(raw[3]);
      act.w = sg;
      const float a = alpha_degs<FULL4>(plan) > 1 ? sg : vsa_round_f16(sg);
      alpha = a * c.decay;
    } else {
      alpha = 1.0f;
    }
    // (hits only: the backward reads act_in for hits only, and at 71 % misses the zeros were 165 MB of the
    //  464 MB this launch wrote at 1920x1080, K = 7)
    if (act_out) act_out[(long long)s * N + n] = act;
  } else if (coeffs_out) {
    float* co = coeffs_out + ((long long)s * N + n) * 64;
    for (int i = 0; i < 64; ++i) co[i] = 0.f;
  }
  const long long o = n * K + s;
  surfs_rgb[3 * o] = rgb[0];
  surfs_rgb[3 * o + 1] = rgb[1];
  surfs_rgb[3 * o + 2] = rgb[2];
  surfs_alpha[o] = alpha;
  if (surfs_normals) {
    surfs_normals[3 * o] = nrm[0];
    surfs_normals[3 * o + 1] = nrm[1];
    surfs_normals[3 * o + 2] = nrm[2];
  }
}

}  // namespace
