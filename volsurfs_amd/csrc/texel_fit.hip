// Texture fit: Adam on the 8-bit texel rows of a baked bank themselves (include/volsurfs_hip.h "Texture fit",
// DESIGN §41).  The reference has no such stage; the rule is this library's own, restated in
// tests/texture_fit_restated.py, which the step must equal bit for bit.
//
// One lane per (interior texel, quad) of a (shell, degree) domain, in domain order — for a baked bank that is slot
// order, so consecutive lanes touch consecutive quads: 8 B of f16 gradient, 16 B each of the fp32 master p and the
// moments m, v, 4 B of texel bytes per lane.  The one-texel apron owns no state: an apron texel's gradient is FOLDED
// into the interior texel it clamps to (vsa_nt_import_planes' rule) and that texel's new bytes are stored to it as
// well (the TIE), by the few edge lanes of a wave.  A quad whose folded gradient is all zero is IDLE: it reads its
// gradient and nothing else.  No scratch, no LDS but the 64 bytes of the counters; built without contraction, IEEE
// division and square root, like adam.hip, whose update (operation for operation) this is.
#include "nt_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int TF_BLOCK = 256;
constexpr int TF_BLOCKS_PER_CU = 6;     // the step's grid: within what stays resident at its 96 SGPRs (7 waves per SIMD)

struct TfCoef {
  float step_size, beta1, beta2, inv_bc2_sqrt, eps, inv_grad_scale;
};

__host__ __device__ inline long long tf_lanes(const vsa_nt_plan& p, int deg) {
  return (long long)p.tex_res[deg] * p.tex_res[deg] * VSA_NT_ROW_QUADS(deg);
}
__host__ __device__ inline long long tf_blocks(const vsa_nt_plan& p, int deg) {
  return (tf_lanes(p, deg) + TF_BLOCK - 1) / TF_BLOCK;
}
__host__ __device__ inline long long tf_blocks_per_shell(const vsa_nt_plan& p) {
  long long n = 0;
  for (int d = 0; d < p.rgb_degrees; ++d) n += tf_blocks(p, d);
  return n;
}

// Lane `threadIdx.x` of CHUNK c (256 consecutive lanes of one (shell, degree); chunks are numbered shell by shell,
// degree by degree): the segment, the texel's domain coordinates (1..R) and the first element of its quad in texels /
// grad_rows / p / m / v, or e = -1 (past the domain's last lane, or a slot outside the segment).
struct TfLane {
  NtRowSeg seg;
  int R, Y, X, quads, quad;
  long long e;
};

__device__ __forceinline__ TfLane tf_lane(const vsa_nt_plan& p, const int32_t* slot_of, const int32_t* seg_start,
                                          unsigned chunk) {
  const unsigned per = (unsigned)tf_blocks_per_shell(p);
  const int shell = (int)(chunk / per);
  unsigned rem = chunk % per;
  int deg = 0;
  for (; deg < p.rgb_degrees - 1; ++deg) {
    const unsigned b = (unsigned)tf_blocks(p, deg);
    if (rem < b) break;
    rem -= b;
  }
  TfLane l;
  l.seg = nt_row_seg(p, shell, deg, slot_of, seg_start);
  l.R = p.tex_res[deg];
  l.quads = VSA_NT_ROW_QUADS(deg);
  const unsigned shift = deg == 0 ? 1u : (deg == 1 ? 2u : 3u);     // quads = 1 << shift
  const long long i = (long long)rem * TF_BLOCK + threadIdx.x;
  l.e = -1;
  l.Y = l.X = 1;
  l.quad = 0;
  if (i < tf_lanes(p, deg)) {
    const unsigned t = (unsigned)(i >> shift), y = t / (unsigned)l.R;      // t < 2^28
    l.quad = (int)(i & (l.quads - 1));
    l.Y = (int)y + 1;
    l.X = (int)(t - y * (unsigned)l.R) + 1;
    const int row = nt_seg_row(l.seg, (long long)l.Y * (l.R + 2) + l.X);
    if (row >= 0) l.e = l.seg.row0 + ((long long)row * l.quads + l.quad) * 4;
  }
  return l;
}

// The apron texels that clamp to interior texel (Y, X) of an (R+2)^2 domain, in row-major (ay, ax) order: the 3 x 3
// candidates {0 | Y | R+1} x {0 | X | R+1} without the centre; row 0 / column 0 only for Y / X = 1, row / column R+1
// only for Y / X = R.  body(first element of the apron texel's quad) for each whose slot lies in the segment.
template <typename Body>
__device__ __forceinline__ void tf_for_each_apron(const TfLane& l, Body&& body) {
  const int W = l.R + 2;
  const int ys[3] = {0, l.Y, W - 1}, xs[3] = {0, l.X, W - 1};
  const bool yv[3] = {l.Y == 1, true, l.Y == l.R}, xv[3] = {l.X == 1, true, l.X == l.R};
#pragma unroll
  for (int cy = 0; cy < 3; ++cy) {
#pragma unroll
    for (int cx = 0; cx < 3; ++cx) {
      if ((cy == 1 && cx == 1) || !yv[cy] || !xv[cx]) continue;
      const int row = nt_seg_row(l.seg, (long long)ys[cy] * W + xs[cx]);
      if (row >= 0) body(l.seg.row0 + ((long long)row * l.quads + l.quad) * 4);
    }
  }
}

__device__ __forceinline__ bool tf_is_edge(const TfLane& l) {
  return l.Y == 1 || l.Y == l.R || l.X == 1 || l.X == l.R;
}

// The workgroup's sums of its lanes' four counters, added to stats by one lane each: wave sums by shuffles, the four
// waves' through 64 bytes of LDS.  Every lane calls it, once, at the end of the kernel.  (One atomic per WAVE and
// counter was measured first: the 24 k atomics of a launch arrive together on one cache line when the waves leave and
// cost 0.2 ms, as much as the bytes of a 512-texture step.)
__device__ __forceinline__ void tf_count(const unsigned (&n)[4], unsigned long long* stats) {
  __shared__ unsigned sums[TF_BLOCK / 64][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned v = n[k];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned v = 0;
#pragma unroll
    for (int w = 0; w < TF_BLOCK / 64; ++w) v += sums[w][threadIdx.x];
    if (v) atomicAdd(stats + threadIdx.x, (unsigned long long)v);
  }
}

__global__ __launch_bounds__(TF_BLOCK) void texel_fit_init_kernel(const vsa_nt_plan p,
                                                                  const int32_t* __restrict__ slot_of,
                                                                  const int32_t* __restrict__ seg_start,
                                                                  uint8_t* __restrict__ texels, float* __restrict__ par,
                                                                  float* __restrict__ m, float* __restrict__ v) {
  const TfLane l = tf_lane(p, slot_of, seg_start, blockIdx.x);
  if (l.e < 0) return;
  const uint32_t q = *reinterpret_cast<const uint32_t*>(texels + l.e);
  f32x4 x;
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = (float)((q >> (8 * k)) & 0xffu) / 255.0f;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  *reinterpret_cast<f32x4*>(par + l.e) = x;
  *reinterpret_cast<f32x4*>(m + l.e) = zero;
  *reinterpret_cast<f32x4*>(v + l.e) = zero;
  if (tf_is_edge(l))
    tf_for_each_apron(l, [&](long long a) { *reinterpret_cast<uint32_t*>(texels + a) = q; });
}

// A workgroup strides over the chunks: the counters stay in registers until it leaves (an atomic per wave of every
// chunk put 0.9 M atomics on four words and took 28 x the time of the bytes).
__global__ __launch_bounds__(TF_BLOCK) void texel_fit_step_kernel(const vsa_nt_plan p,
                                                                  const int32_t* __restrict__ slot_of,
                                                                  const int32_t* __restrict__ seg_start,
                                                                  uint2* __restrict__ grad_rows, const TfCoef c,
                                                                  float* __restrict__ par, float* __restrict__ m,
                                                                  float* __restrict__ v, uint8_t* __restrict__ texels,
                                                                  unsigned nr_chunks,
                                                                  unsigned long long* __restrict__ stats) {
  unsigned updated = 0, nonfinite = 0, changed = 0, clamped = 0;
  for (unsigned chunk = blockIdx.x; chunk < nr_chunks; chunk += gridDim.x) {
    const TfLane l = tf_lane(p, slot_of, seg_start, chunk);
    if (l.e < 0) continue;
    const bool edge = tf_is_edge(l);
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    // fold + consume: the own quad, then the apron quads in row-major order; a quad that is not all-zero bits is
    // added and cleared
    auto take = [&](long long e) {
      uint2* src = grad_rows + (e >> 2);
      const uint2 w = *src;
      if ((w.x | w.y) == 0u) return;
      half4_t h;
      __builtin_memcpy(&h, &w, 8);
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] = g[k] + (float)h[k];
      *src = make_uint2(0u, 0u);
    };
    take(l.e);
    if (edge) tf_for_each_apron(l, take);
    bool idle = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      g[k] = g[k] * c.inv_grad_scale;
      if (!(fabsf(g[k]) <= 3.4028234663852886e38f)) {
        g[k] = 0.f;
        ++nonfinite;
      }
      idle = idle && g[k] == 0.f;
    }
    if (idle) continue;
    f32x4 x = *reinterpret_cast<const f32x4*>(par + l.e);
    f32x4 mm = *reinterpret_cast<const f32x4*>(m + l.e);
    f32x4 vv = *reinterpret_cast<const f32x4*>(v + l.e);
    const uint32_t q_old = *reinterpret_cast<const uint32_t*>(texels + l.e);
    const float omb1 = 1.0f - c.beta1, omb2 = 1.0f - c.beta2;
    uint32_t q_new = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mm[k] = mm[k] + omb1 * (g[k] - mm[k]);
      vv[k] = vv[k] * c.beta2 + (omb2 * g[k]) * g[k];
      const float denom = sqrtf(vv[k]) * c.inv_bc2_sqrt + c.eps;
      float t = x[k] - c.step_size * (mm[k] / denom);
      clamped += !(t >= 0.f && t <= 1.f);
      t = fminf(fmaxf(t, 0.f), 1.f);
      x[k] = t;
      const uint32_t b = (uint32_t)(int)rintf(255.0f * t);
      changed += b != ((q_old >> (8 * k)) & 0xffu);
      q_new |= b << (8 * k);
    }
    *reinterpret_cast<f32x4*>(par + l.e) = x;
    *reinterpret_cast<f32x4*>(m + l.e) = mm;
    *reinterpret_cast<f32x4*>(v + l.e) = vv;
    *reinterpret_cast<uint32_t*>(texels + l.e) = q_new;
    if (edge) tf_for_each_apron(l, [&](long long a) { *reinterpret_cast<uint32_t*>(texels + a) = q_new; });   // tie
    ++updated;
  }
  const unsigned counts[4] = {updated, nonfinite, changed, clamped};
  tf_count(counts, stats);
}

// This stage's own limits, after nt_common.h's nt_baked_plan_supported.
int tf_check_supported(const vsa_nt_plan* p) {
  if (const int rc = nt_baked_plan_supported(p)) return rc;
  if (p->row_base[VSA_MAX_SHELLS * VSA_NT_MAX_DEG] * 8 >= (1ll << 32)) return VSA_ERR_UNSUPPORTED;   // vsa_nt_shade_bwd's limit
  if (p->nr_shells * tf_blocks_per_shell(*p) >= (1ll << 31)) return VSA_ERR_UNSUPPORTED;
  return VSA_OK;
}

bool tf_aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }
bool tf_finite_nonneg(float x) { return x >= 0.f && x <= 3.4028234663852886e38f; }

}  // namespace

extern "C" long long vsa_texel_fit_state_bytes(const vsa_nt_plan* plan) {
  int rc = nt_baked_plan_args(plan);
  if (!rc) rc = tf_check_supported(plan);
  if (rc) return rc;
  return plan->row_base[VSA_MAX_SHELLS * VSA_NT_MAX_DEG] * 4 * (long long)sizeof(float);
}

extern "C" int vsa_texel_fit_init(const vsa_nt_plan* plan, const int32_t* slot_of, const int32_t* seg_start,
                                  uint8_t* texels, float* p, float* m, float* v, void* stream) {
  int rc = nt_baked_plan_args(plan);
  if (rc) return rc;
  if (!slot_of || !seg_start || !texels || !p || !m || !v) return VSA_ERR_ARG;
  if (!tf_aligned16(texels) || !tf_aligned16(p) || !tf_aligned16(m) || !tf_aligned16(v)) return VSA_ERR_ARG;
  rc = tf_check_supported(plan);
  if (rc) return rc;
  const long long blocks = plan->nr_shells * tf_blocks_per_shell(*plan);
  hipLaunchKernelGGL(texel_fit_init_kernel, dim3((unsigned)blocks), dim3(TF_BLOCK), 0, (hipStream_t)stream, *plan,
                     slot_of, seg_start, texels, p, m, v);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_texel_fit_step(const vsa_nt_plan* plan, const int32_t* slot_of, const int32_t* seg_start,
                                  uint16_t* grad_rows, float inv_grad_scale, float* p, float* m, float* v,
                                  uint8_t* texels, float lr, float beta1, float beta2, float eps, int step,
                                  unsigned long long* stats, void* stream) {
  int rc = nt_baked_plan_args(plan);
  if (rc) return rc;
  if (!slot_of || !seg_start || !grad_rows || !p || !m || !v || !texels || !stats) return VSA_ERR_ARG;
  if (!tf_aligned16(grad_rows) || !tf_aligned16(p) || !tf_aligned16(m) || !tf_aligned16(v) || !tf_aligned16(texels) ||
      ((uintptr_t)stats & 7))
    return VSA_ERR_ARG;
  if (step < 1 || !tf_finite_nonneg(lr) || !tf_finite_nonneg(eps) || !tf_finite_nonneg(inv_grad_scale)) return VSA_ERR_ARG;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return VSA_ERR_ARG;
  rc = tf_check_supported(plan);
  if (rc) return rc;
  // bias corrections in double, as vsa_adam_step forms them
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const TfCoef coef = {(float)((double)lr / bc1), beta1, beta2, (float)(1.0 / sqrt(bc2)), eps, inv_grad_scale};
  int cus = 0;
  rc = vsa_cu_count(&cus);
  if (rc) return rc;
  VSA_HIP_TRY(hipMemsetAsync(stats, 0, 4 * sizeof(unsigned long long), (hipStream_t)stream));
  const long long chunks = plan->nr_shells * tf_blocks_per_shell(*plan);
  const long long resident = (long long)cus * TF_BLOCKS_PER_CU;
  hipLaunchKernelGGL(texel_fit_step_kernel, dim3((unsigned)(chunks < resident ? chunks : resident)), dim3(TF_BLOCK), 0,
                     (hipStream_t)stream, *plan, slot_of, seg_start, reinterpret_cast<uint2*>(grad_rows), coef, p, m, v,
                     texels, (unsigned)chunks, stats);
  VSA_RETURN_LAUNCH_STATUS();
}
