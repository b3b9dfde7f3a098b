// Baked textures of one stack of shells carried onto another stack with other faces and other UVs.  (The reference has
// no such stage: the rule is this library's own -- include/volsurfs_hip.h "Texture transfer", DESIGN §40: restated in
// tests/texture_transfer_restated.py, unpinned.)
//
// vsa_textransfer_owners: which destination face owns each texel of the (shell, degree) grids of one degree.  One wave
// per destination face walks the texels of the face's uv box grown by `reach` and offers (not covered by the face's
// raster, d2 bits, face) to the texel's 64-bit word with an integer atomicMin: the map is a function of the mesh alone.
// vsa_textransfer_owner_fields: the words of one shell decoded into face / barycentrics / d2 images.
// vsa_textransfer_planes: a wave takes an 8 x 8 tile of one (shell, degree) texel grid.  Every owned lane makes its
// samples' 3-D points on the owner face, walks the source shell's q16 tree (closest_walk.h: brute force's bits, the
// stack in LDS), fetches the source planes as the baked shade does (LUT, lerp or anchor, fp16 coefficient) and stores
// the nearest byte of the mean.  Counts by integer atomics, the fp64 sum of d2 as one word per wave added in a fixed
// order: the same inputs give the same bytes.
#include "closest_walk.h"
#include "nt_common.h"
#include "ordered_sum.h"
#include "uv_raster.h"

namespace {

constexpr int TT_TILE = 8;                  // 8 x 8 texels = one wave
constexpr unsigned long long TT_UNOWNED = ~0ull;
enum { TT_OWNED = 0, TT_COVERED = 1, TT_SAMPLES = 2, TT_MAX = 3, TT_FAR = 4, TT_SUM2 = 5, TT_WORDS = 8 };

struct TtShells {
  long long face_base[VSA_MAX_SHELLS + 1];   // first row of each destination shell in dst_uvs / dst_recs
};

__host__ __device__ inline int tt_tiles(int R) {
  const int t = (R + TT_TILE - 1) / TT_TILE;
  return t * t;
}

// The uv triangle of a destination face in texel units (uv times R, z = 0) as a record of "Mesh distance".
__device__ __forceinline__ void tt_uv_record(const float* __restrict__ uv6, float Rf, float4& a0, float4& e1,
                                             float4& e2) {
  const float x0 = uv6[0] * Rf, y0 = uv6[1] * Rf;
  const float x1 = uv6[2] * Rf, y1 = uv6[3] * Rf;
  const float x2 = uv6[4] * Rf, y2 = uv6[5] * Rf;
  a0 = make_float4(x0, y0, 0.0f, 0.0f);
  e1 = make_float4(x1 - x0, y1 - y0, 0.0f, 0.0f);
  e2 = make_float4(x2 - x0, y2 - y0, 0.0f, 0.0f);
}

// closest_on_triangle of the texel-unit point (qx, qy, 0).  A point the chain puts into the interior region is its own
// nearest point: d2 = 0 (the residual the chain forms there is the rounding of u and v, not a distance).
__device__ __forceinline__ void tt_project(const float4 a0, const float4 e1, const float4 e2, float qx, float qy,
                                           float& d2, float& u, float& v) {
  int region;
  closest_on_triangle(a0, e1, e2, qx, qy, 0.0f, d2, u, v, region);
  if (region == CR_IN) d2 = 0.0f;
}

__device__ __forceinline__ bool tt_finite(float x) { return fabsf(x) < INFINITY; }

// An owner word: the faces whose raster covers the texel come first (bit 63 clear, d2 = 0), then the others by the
// projection's d2; ties go to the lowest face.  d2 >= 0: the order of its bits is the order of its values.
constexpr unsigned long long TT_OUTSIDE = 1ull << 63;

__device__ __forceinline__ unsigned long long tt_key(bool covers, float d2, unsigned face) {
  return covers ? (unsigned long long)face
                : TT_OUTSIDE | ((unsigned long long)__float_as_uint(d2) << 32) | face;
}
__device__ __forceinline__ unsigned tt_key_d2_bits(unsigned long long key) {
  return (unsigned)(key >> 32) & 0x7fffffffu;
}

__global__ __launch_bounds__(64) void tt_owner_kernel(const float* __restrict__ dst_uvs,
                                                      const float* __restrict__ dst_recs, TtShells sh, int nr_shells,
                                                      int R, float reach, unsigned long long* __restrict__ keys) {
  const long long gf = blockIdx.x;
  const int lane = threadIdx.x;
  int shell = 0;
  for (int s = 1; s < nr_shells; ++s) shell = gf >= sh.face_base[s] ? s : shell;
  const float* uv6 = dst_uvs + 6 * gf;
  const float* rec = dst_recs + 12 * gf;
  bool ok = true;
  for (int k = 0; k < 6; ++k) ok = ok && tt_finite(uv6[k]);
  for (int k = 0; k < 12; ++k) ok = ok && ((k & 3) == 3 || tt_finite(rec[k]));
  if (!ok) return;                                   // a face with a NaN is a candidate of nothing
  const float Rf = (float)R;
  float4 a0, e1, e2;
  tt_uv_record(uv6, Rf, a0, e1, e2);
  const float x1 = a0.x + e1.x, x2 = a0.x + e2.x, y1 = a0.y + e1.y, y2 = a0.y + e2.y;
  const float minx = fminf(a0.x, fminf(x1, x2)), maxx = fmaxf(a0.x, fmaxf(x1, x2));
  const float miny = fminf(a0.y, fminf(y1, y2)), maxy = fmaxf(a0.y, fmaxf(y1, y2));
  if (!(tt_finite(minx) && tt_finite(maxx) && tt_finite(miny) && tt_finite(maxy))) return;
  // centres i + 0.5 within [min - reach, max + reach], a texel more on each side (the test below decides)
  const float top = Rf - 1.0f;
  if (maxx + reach + 1.5f < 0.0f || maxy + reach + 1.5f < 0.0f || minx - reach - 1.5f > top || miny - reach - 1.5f > top)
    return;
  const int i0 = (int)fminf(fmaxf(floorf(minx - reach - 1.5f), 0.0f), top);
  const int i1 = (int)fminf(fmaxf(ceilf(maxx + reach + 0.5f), 0.0f), top);
  const int j0 = (int)fminf(fmaxf(floorf(miny - reach - 1.5f), 0.0f), top);
  const int j1 = (int)fminf(fmaxf(ceilf(maxy + reach + 0.5f), 0.0f), top);
  const int w = i1 - i0 + 1, h = j1 - j0 + 1;
  const float reach2 = reach * reach;
  const UvTri snapped = uv_snap(uv6, R);                // coverage: uv_raster.h, vsa_atlas_rasterize's rule
  const unsigned face = (unsigned)(gf - sh.face_base[shell]);
  unsigned long long* map = keys + (long long)shell * R * R;
  for (long long t = lane; t < (long long)w * h; t += 64) {
    const int i = i0 + (int)(t % w), j = j0 + (int)(t / w);
    float d2, u, v;
    tt_project(a0, e1, e2, (float)i + 0.5f, (float)j + 0.5f, d2, u, v);
    const bool covers = uv_covers(snapped, i, j);
    if (!(covers || d2 <= reach2)) continue;
    const unsigned long long key = tt_key(covers, d2, face);
    unsigned long long* word = map + (long long)j * R + i;
    // (the word only shrinks: a candidate that does not beat the value it reads, however stale, has nothing to add)
    if (key < __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(word, key);
  }
}

__global__ __launch_bounds__(256) void tt_fields_kernel(const unsigned long long* __restrict__ keys,
                                                        const float* __restrict__ dst_uvs, long long face_first, int R,
                                                        int* __restrict__ face, float* __restrict__ bary,
                                                        float* __restrict__ d2_out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)R * R) return;
  const unsigned long long key = keys[t];
  if (key == TT_UNOWNED) {
    face[t] = -1;
    bary[2 * t] = bary[2 * t + 1] = 0.0f;
    d2_out[t] = INFINITY;
    return;
  }
  const unsigned f = (unsigned)(key & 0xffffffffull);
  float4 a0, e1, e2;
  tt_uv_record(dst_uvs + 6 * (face_first + f), (float)R, a0, e1, e2);
  float d2, u, v;
  tt_project(a0, e1, e2, (float)(t % R) + 0.5f, (float)(t / R) + 0.5f, d2, u, v);
  face[t] = (int)f;
  bary[2 * t] = u;
  bary[2 * t + 1] = v;
  d2_out[t] = __uint_as_float(tt_key_d2_bits(key));
}

struct TtArgs {
  // source
  const uint4* qnodes;
  const float4* tris;
  Roots roots;
  Frames frames;
  const float* src_face_uvs;        // [slots, 6], in the order of tris
  const uint8_t* src_planes;        // the planes of "Texture export"
  long long src_shell_stride, src_deg_off;
  int src_res, anchor, alpha_mask;  // bit s of alpha_mask: shell s has an alpha model
  float sh_lo, sh_span;
  // destination
  const float* dst_uvs;
  const float* dst_recs;
  TtShells sh;
  int dst_res, samples;
  float max_distance;
  const unsigned long long* keys;
  uint8_t* dst_planes;
  long long dst_shell_stride, dst_deg_off;
  unsigned long long* stats;        // [shells, TT_WORDS]
  double* partials;                 // [shells, tiles]
};

template <int D, int STACK, bool BOUNDS>
__global__ __launch_bounds__(TRACE_BLOCK) void tt_transfer_kernel(const TtArgs a) {
  constexpr int N = 2 * D + 1;
  __shared__ int s_node[STACK][TRACE_BLOCK];
  __shared__ float s_bound[BOUNDS ? STACK : 1][TRACE_BLOCK];
  __shared__ float s_lut[256];
  const int lane = threadIdx.x;
  for (int q = lane; q < 256; q += TRACE_BLOCK) {          // build_lut's three fp16 roundings
    const float o = vsa_round_f16((float)q / 255.0f);
    const float t = vsa_round_f16(a.sh_span * o);
    s_lut[q] = vsa_round_f16(a.sh_lo + t);
  }
  __syncthreads();
  const int shell = blockIdx.y, R2 = a.dst_res, R = a.src_res;
  const int tiles_x = (R2 + TT_TILE - 1) / TT_TILE;
  const int r = ((int)blockIdx.x / tiles_x) * TT_TILE + (lane >> 3);
  const int c = ((int)blockIdx.x % tiles_x) * TT_TILE + (lane & 7);
  const bool inside = r < R2 && c < R2;
  const long long texel = (long long)r * R2 + c;
  const unsigned long long key = inside ? a.keys[(long long)shell * R2 * R2 + texel] : TT_UNOWNED;
  const bool owned = key != TT_UNOWNED;
  const bool has_alpha = (a.alpha_mask >> shell) & 1;

  float4 ua0 = make_float4(0.f, 0.f, 0.f, 0.f), ue1 = ua0, ue2 = ua0, v0 = ua0, e1 = ua0, e2 = ua0;
  if (owned) {
    const long long gf = a.sh.face_base[shell] + (long long)(key & 0xffffffffull);
    tt_uv_record(a.dst_uvs + 6 * gf, (float)R2, ua0, ue1, ue2);
    const float4* rec = reinterpret_cast<const float4*>(a.dst_recs) + 3 * gf;
    v0 = rec[0], e1 = rec[1], e2 = rec[2];
  }
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.src_planes + shell * a.src_shell_stride + a.src_deg_off);
  const long long src_plane = (long long)R * R;

  float sum[4 * N];
#pragma unroll
  for (int k = 0; k < 4 * N; ++k) sum[k] = 0.0f;
  double s2 = 0.0;
  unsigned far = 0, dmax = 0;
  const int S = a.samples;
  const float Sf = (float)S;
  for (int n = 0; n < S * S; ++n) {                          // b outer, a inner
    const int sa = n % S, sb = n / S;
    const float qx = ((float)c + 0.5f) + (((float)sa + 0.5f) / Sf - 0.5f);
    const float qy = ((float)r + 0.5f) + (((float)sb + 0.5f) / Sf - 0.5f);
    float pd2, bu, bv;
    tt_project(ua0, ue1, ue2, qx, qy, pd2, bu, bv);
    const float px = (v0.x + bu * e1.x) + bv * e2.x;
    const float py = (v0.y + bu * e1.y) + bv * e2.y;
    const float pz = (v0.z + bu * e1.z) + bv * e2.z;
    const QPoint q = closest_qpoint(a.frames.f[shell], px, py, pz);
    Closest best = no_closest();
    closest_walk<STACK, BOUNDS>(a.qnodes, a.tris, q, px, py, pz, owned ? a.roots.root[shell] : TRACE_EMPTY, best,
                                s_node, s_bound, lane);
    if (owned && best.slot < 0) ++far;                       // no closest record (a point that is not finite)
    if (!(owned && best.slot >= 0)) continue;
    const float d = sqrtf(best.d2);
    s2 += (double)best.d2;
    dmax = max(dmax, __float_as_uint(d));
    far += d > a.max_distance ? 1u : 0u;
    const float2 uv = nt_interp_uv(a.src_face_uvs + 6 * (long long)best.slot, best.u, best.v);
    const NtFootprint f = nt_footprint(uv.x, uv.y, R, a.anchor != 0);
    const int step = a.anchor ? 0 : 1;
    // corner k = (ky, kx): texel (iy, ix) = (j0 + ky, i0 + kx) clamped to the edge = pixel (R-1-ix, iy)
    const int ix0 = min(max(f.i0, 0), R - 1), ix1 = min(max(f.i0 + step, 0), R - 1);
    const int iy0 = min(max(f.j0, 0), R - 1), iy1 = min(max(f.j0 + step, 0), R - 1);
    const long long p0 = (long long)(R - 1 - ix0) * R + iy0, p1 = (long long)(R - 1 - ix1) * R + iy0;
    const long long p2 = (long long)(R - 1 - ix0) * R + iy1, p3 = (long long)(R - 1 - ix1) * R + iy1;
    const float w0 = (1.0f - f.fx) * (1.0f - f.fy), w1 = f.fx * (1.0f - f.fy);
    const float w2 = (1.0f - f.fx) * f.fy, w3 = f.fx * f.fy;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const uint32_t* pl = src + i * src_plane;
      const uint32_t b0 = pl[p0], b1 = pl[p1], b2 = pl[p2], b3 = pl[p3];
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        float acc = 0.0f;
        acc = acc + s_lut[(b0 >> (8 * ch)) & 255u] * w0;
        acc = acc + s_lut[(b1 >> (8 * ch)) & 255u] * w1;
        acc = acc + s_lut[(b2 >> (8 * ch)) & 255u] * w2;
        acc = acc + s_lut[(b3 >> (8 * ch)) & 255u] * w3;
        sum[4 * i + ch] = sum[4 * i + ch] + vsa_round_f16(vsa_pin_f32(acc));
      }
    }
  }

  // resolve: the mean, then the byte whose LUT value is nearest (ties: the lowest byte)
  if (inside) {
    const float inv = 1.0f / (Sf * Sf);
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.dst_planes + shell * a.dst_shell_stride + a.dst_deg_off) + texel;
    const long long dst_plane = (long long)R2 * R2;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      uint32_t px = has_alpha ? 0u : 0xff000000u;
      if (owned) {
        float val[4], bd[4];
        unsigned bq[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) val[ch] = sum[4 * i + ch] * inv, bd[ch] = INFINITY, bq[ch] = 0u;
        for (int q = 0; q < 256; ++q) {
          const float lq = s_lut[q];
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) {
            const float dd = fabsf(lq - val[ch]);
            if (dd < bd[ch]) bd[ch] = dd, bq[ch] = (unsigned)q;
          }
        }
        px = bq[0] | (bq[1] << 8) | (bq[2] << 16) | (has_alpha ? bq[3] << 24 : 0xff000000u);
      }
      dst[i * dst_plane] = px;
    }
  }

  // report: counts and the maximum by integer atomics, the wave's fp64 sum in a fixed tree
  const unsigned long long m_owned = __builtin_amdgcn_ballot_w64(owned);
  const unsigned long long m_cov = __builtin_amdgcn_ballot_w64(owned && tt_key_d2_bits(key) == 0u);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    far += (unsigned)__shfl_xor((int)far, m);
    dmax = max(dmax, (unsigned)__shfl_xor((int)dmax, m));
    s2 += __shfl_xor(s2, m);
  }
  if (lane == 0) {
    unsigned long long* st = a.stats + (long long)shell * TT_WORDS;
    if (m_owned) atomicAdd(&st[TT_OWNED], (unsigned long long)__builtin_popcountll(m_owned));
    if (m_cov) atomicAdd(&st[TT_COVERED], (unsigned long long)__builtin_popcountll(m_cov));
    if (far) atomicAdd(&st[TT_FAR], (unsigned long long)far);
    if (dmax > __hip_atomic_load(&st[TT_MAX], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(&st[TT_MAX], (unsigned long long)dmax);
    a.partials[(long long)shell * gridDim.x + blockIdx.x] = s2;
  }
}

// One block per shell: the shell's per-wave sums of d2 added in ordered_sum.h's fixed order.
__global__ __launch_bounds__(ORDERED_SUM_BLOCK) void tt_sum_kernel(const double* __restrict__ partials, int nr_waves,
                                                                   int samples,
                                                                   unsigned long long* __restrict__ stats) {
  const int shell = blockIdx.x;
  double total[1];
  if (!ordered_sum<1, 1>(partials + (long long)shell * nr_waves, nr_waves, total)) return;
  unsigned long long* st = stats + (long long)shell * TT_WORDS;
  st[TT_SUM2] = (unsigned long long)__double_as_longlong(total[0]);
  st[TT_SAMPLES] = st[TT_OWNED] * (unsigned long long)(samples * samples);
}

struct TtLayout {
  size_t o_keys, o_partials, total;
};

TtLayout tt_layout(int nr_shells, int R) {
  TtLayout l;
  l.o_keys = 0;
  l.o_partials = (size_t)nr_shells * R * R * 8;
  l.total = l.o_partials + (size_t)nr_shells * tt_tiles(R) * 8;
  return l;
}

int tt_check_dst(const float* dst_uvs, const float* dst_recs, const long long* face_base, int nr_shells, int dst_res,
                 const void* workspace, long long workspace_bytes) {
  if (nr_shells < 1 || nr_shells > VSA_MAX_SHELLS || dst_res < 1 || dst_res > NT_MAX_TEX_RES) return VSA_ERR_ARG;
  if (!dst_uvs || !dst_recs || !face_base || !workspace) return VSA_ERR_ARG;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)dst_recs & 15)) return VSA_ERR_ARG;
  if (face_base[0] != 0) return VSA_ERR_ARG;
  for (int s = 0; s < nr_shells; ++s)
    if (face_base[s + 1] <= face_base[s]) return VSA_ERR_ARG;                  // every shell has a face
  if (face_base[nr_shells] > 0x7fffffffll) return VSA_ERR_UNSUPPORTED;
  if (workspace_bytes < (long long)tt_layout(nr_shells, dst_res).total) return VSA_ERR_ARG;
  return VSA_OK;
}

TtShells tt_shells(const long long* face_base, int nr_shells) {
  TtShells sh;
  for (int s = 0; s <= VSA_MAX_SHELLS; ++s) sh.face_base[s] = face_base[s < nr_shells ? s : nr_shells];
  return sh;
}

}  // namespace

extern "C" long long vsa_textransfer_workspace_bytes(int nr_shells, int dst_res) {
  if (nr_shells < 1 || nr_shells > VSA_MAX_SHELLS || dst_res < 1 || dst_res > NT_MAX_TEX_RES) return VSA_ERR_ARG;
  return (long long)tt_layout(nr_shells, dst_res).total;
}

extern "C" int vsa_textransfer_owners(const float* dst_uvs, const float* dst_recs, const long long* face_base,
                                      int nr_shells, int dst_res, float reach, void* workspace,
                                      long long workspace_bytes, void* stream) {
  if (const int rc = tt_check_dst(dst_uvs, dst_recs, face_base, nr_shells, dst_res, workspace, workspace_bytes))
    return rc;
  if (!(reach >= 0.0f) || !(reach <= 64.0f)) return VSA_ERR_ARG;               // negative, NaN or absurd
  const hipStream_t st = (hipStream_t)stream;
  const TtLayout l = tt_layout(nr_shells, dst_res);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + l.o_keys);
  VSA_HIP_TRY(hipMemsetAsync(keys, 0xff, l.o_partials, st));
  hipLaunchKernelGGL(tt_owner_kernel, dim3((unsigned)face_base[nr_shells]), dim3(64), 0, st, dst_uvs, dst_recs,
                     tt_shells(face_base, nr_shells), nr_shells, dst_res, reach, keys);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_textransfer_owner_fields(const void* workspace, long long workspace_bytes, const float* dst_uvs,
                                            const long long* face_base, int nr_shells, int shell, int dst_res,
                                            int32_t* face, float* bary, float* d2, void* stream) {
  if (nr_shells < 1 || nr_shells > VSA_MAX_SHELLS || dst_res < 1 || dst_res > NT_MAX_TEX_RES) return VSA_ERR_ARG;
  if (!workspace || !dst_uvs || !face_base || !face || !bary || !d2 || shell < 0 || shell >= nr_shells)
    return VSA_ERR_ARG;
  if ((uintptr_t)workspace & 15) return VSA_ERR_ARG;
  if (workspace_bytes < (long long)tt_layout(nr_shells, dst_res).total) return VSA_ERR_ARG;
  const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(workspace) +
                                   (long long)shell * dst_res * dst_res;
  const long long n = (long long)dst_res * dst_res;
  hipLaunchKernelGGL(tt_fields_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keys,
                     dst_uvs, face_base[shell], dst_res, face, bary, d2);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_textransfer_planes(const vsa_nt_plan* src_plan, int degree, const uint8_t* src_planes,
                                      long long src_planes_bytes, const uint32_t* qnodes, const float* tris,
                                      const int32_t* mesh_roots, const float* mesh_frames, int nr_meshes, int max_depth,
                                      const float* src_face_uvs, const float* dst_uvs, const float* dst_recs,
                                      const long long* face_base, const int32_t* dst_tex_res, int samples,
                                      float max_distance, void* workspace, long long workspace_bytes,
                                      uint8_t* dst_planes, long long dst_planes_bytes, unsigned long long* stats,
                                      void* stream) {
  // (nt_common.h's checks in this entry's order: an unsupported plan is reported before a bad resolution)
  if (!dst_tex_res) return VSA_ERR_ARG;
  if (const int rc = nt_baked_plan_counts(src_plan)) return rc;
  if (const int rc = nt_baked_plan_supported(src_plan)) return rc;
  const vsa_nt_plan& p = *src_plan;
  if (degree < 0 || degree >= p.rgb_degrees || samples < 1 || samples > 4 || nr_meshes != p.nr_shells)
    return VSA_ERR_ARG;
  if (max_distance != max_distance) return VSA_ERR_ARG;
  if (const int rc = nt_baked_plan_resolutions(src_plan)) return rc;
  for (int d = 0; d < p.rgb_degrees; ++d)
    if (dst_tex_res[d] < 1 || dst_tex_res[d] > NT_MAX_TEX_RES) return VSA_ERR_ARG;
  if (const int rc = check_qtree(qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth, VSA_ERR_ARG)) return rc;
  const int R2 = dst_tex_res[degree];
  if (const int rc = tt_check_dst(dst_uvs, dst_recs, face_base, nr_meshes, R2, workspace, workspace_bytes)) return rc;
  if (!src_planes || !src_face_uvs || !dst_planes || !stats) return VSA_ERR_ARG;
  if (((uintptr_t)src_planes & 15) || ((uintptr_t)dst_planes & 15) || ((uintptr_t)stats & 7)) return VSA_ERR_ARG;
  TtArgs a;
  nt_plane_layout(p.tex_res, p.rgb_degrees, degree, &a.src_shell_stride, &a.src_deg_off);
  nt_plane_layout(dst_tex_res, p.rgb_degrees, degree, &a.dst_shell_stride, &a.dst_deg_off);
  if (src_planes_bytes != a.src_shell_stride * p.nr_shells || dst_planes_bytes != a.dst_shell_stride * p.nr_shells)
    return VSA_ERR_ARG;
  const QTree t = make_qtree(qnodes, tris, mesh_roots, mesh_frames, nr_meshes);
  const TtLayout l = tt_layout(nr_meshes, R2);
  char* ws = static_cast<char*>(workspace);
  a.qnodes = t.qnodes, a.tris = t.tris, a.roots = t.roots, a.frames = t.frames;
  a.src_face_uvs = src_face_uvs, a.src_planes = src_planes;
  a.src_res = p.tex_res[degree], a.anchor = p.anchor != 0, a.alpha_mask = 0;
  for (int s = 0; s < p.nr_shells; ++s) a.alpha_mask |= nt_shell_has_alpha(p, s) ? 1 << s : 0;
  a.sh_lo = p.sh_lo[degree], a.sh_span = p.sh_span[degree];
  a.dst_uvs = dst_uvs, a.dst_recs = dst_recs, a.sh = tt_shells(face_base, nr_meshes);
  a.dst_res = R2, a.samples = samples, a.max_distance = max_distance;
  a.keys = reinterpret_cast<const unsigned long long*>(ws + l.o_keys);
  a.dst_planes = dst_planes, a.stats = stats;
  a.partials = reinterpret_cast<double*>(ws + l.o_partials);
  const hipStream_t st = (hipStream_t)stream;
  const int tiles = tt_tiles(R2);
  VSA_HIP_TRY(hipMemsetAsync(stats, 0, (size_t)nr_meshes * TT_WORDS * 8, st));
  const dim3 grid((unsigned)tiles, (unsigned)nr_meshes), block(TRACE_BLOCK);
  with_stack(max_depth, [&](auto sk) {
    with_flag(closest_walk_bounds(max_depth), [&](auto bd) {
      constexpr int SK = decltype(sk)::value;
      constexpr bool BD = decltype(bd)::value;
      switch (degree) {
        case 0: hipLaunchKernelGGL((tt_transfer_kernel<0, SK, BD>), grid, block, 0, st, a); break;
        case 1: hipLaunchKernelGGL((tt_transfer_kernel<1, SK, BD>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((tt_transfer_kernel<2, SK, BD>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((tt_transfer_kernel<3, SK, BD>), grid, block, 0, st, a); break;
      }
    });
  });
  VSA_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(tt_sum_kernel, dim3((unsigned)nr_meshes), dim3(ORDERED_SUM_BLOCK), 0, st, a.partials, tiles, samples,
                     stats);
  VSA_RETURN_LAUNCH_STATUS();
}
