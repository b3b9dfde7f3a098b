// Texture mips (include/volsurfs_hip.h "Texture mips"): the mip chain of a baked scene's RGBA8 planes, the
// uv density of the faces, and the baked shade that picks each degree's level from the pixel's footprint on the surface.
//
// vsa_texmip_reduce    one level from the previous one, every image of the level in one launch.  A streaming kernel:
//                      a lane makes two adjacent destination texels from two 16-byte loads (one per child row) and
//                      stores them with one 8-byte store; the children of both texels are summed two channels per
//                      dword (masked by their coverage), so that a texel costs a dozen integer operations.  No LDS,
//                      no atomics, integers only.
// vsa_texmip_density   uv area per world area of every face slot, once per scene.
// vsa_nt_shade_mip_fwd vsa_nt_shade_fwd's forward of one ray (nt_shade_common.h: hit context, SH sums, sigmoids, alpha
//                      decay, dense scatter) with each band's 28 lerp sums taken from the level the footprint asks for:
//                      level 0 from the scene's texel rows (row_sums, vsa_nt_shade_fwd's own), a level above from that
//                      level's planes with the clamp-to-edge corner rule of the texture transfer's source lookup.
#include "nt_shade_common.h"

namespace {

constexpr int MIP_BLOCK = 256;

// Geometry of one reduce launch: level l - 1 (src) -> level l (dst).
struct MipGeom {
  int degrees;
  int res_src[VSA_NT_MAX_DEG];              // R_d >> (l - 1); even
  int pair[VSA_NT_MAX_DEG];                 // 1: a lane makes two adjacent texels (the destination rows are 8-byte aligned)
  int block_first[VSA_NT_MAX_DEG + 1];      // first block of each degree within a shell's blocks
  long long src_before[VSA_NT_MAX_DEG], dst_before[VSA_NT_MAX_DEG];   // bytes of a shell's planes before degree d
  long long cov_src_before[VSA_NT_MAX_DEG], cov_dst_before[VSA_NT_MAX_DEG];
  long long src_stride, dst_stride, cov_src_stride, cov_dst_stride;   // bytes per shell
};

// Items of degree d per shell: (coefficient, destination row, destination column or column pair).
__host__ __device__ inline long long mip_items(int res_src, int pair, int d) {
  const long long Rd = res_src >> 1;
  return (2 * d + 1) * Rd * (pair ? Rd >> 1 : Rd);
}

// q = (2 sum + n) / (2 n) for n in 1..4 and sum <= 4 * 255, without a division: n = 1, 2, 4 are shifts; for n = 3,
// (2 sum + 3) / 6 = ((2 sum + 3) * 10923) >> 16 exactly (10923 / 65536 - 1 / 6 = 5.1e-6: below 1 / 6 up to 32767).
__device__ __forceinline__ unsigned mip_mean(unsigned sum, unsigned n) {
  const unsigned h = n >> 1;
  return n == 3 ? ((2u * sum + 3u) * 10923u) >> 16 : (sum + h) >> h;
}

// The destination texel of four children px[k] with coverage flags cv[k] (nonzero: covered); *any = some child covered.
__device__ __forceinline__ unsigned mip_texel(const unsigned px[4], const unsigned cv[4], unsigned* any) {
  unsigned n = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) n += cv[k] ? 1u : 0u;
  *any = n ? 1u : 0u;
  const bool all = n == 0;          // no child covered: the mean of all four
  if (all) n = 4;
  unsigned lo = 0, hi = 0;          // channels 0 | 2 and 1 | 3, 16 bits each (a sum is at most 1020)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned m = (all || cv[k]) ? 0x00ff00ffu : 0u;
    lo += px[k] & m;
    hi += (px[k] >> 8) & m;
  }
  return mip_mean(lo & 0xffffu, n) | (mip_mean(hi & 0xffffu, n) << 8) | (mip_mean(lo >> 16, n) << 16) |
         (mip_mean(hi >> 16, n) << 24);
}

__global__ void __launch_bounds__(MIP_BLOCK)
texmip_reduce_kernel(const MipGeom g, const uint8_t* __restrict__ src, const uint8_t* __restrict__ src_cover,
                     uint8_t* __restrict__ dst, uint8_t* __restrict__ dst_cover) {
  const int per_shell = g.block_first[g.degrees];
  const int shell = blockIdx.x / per_shell, rem = blockIdx.x % per_shell;
  int d = 0;
#pragma unroll
  for (int k = 1; k < VSA_NT_MAX_DEG; ++k)
    if (k < g.degrees && rem >= g.block_first[k]) d = k;
  int Rs = 0, pair = 0, first = 0;
  long long sb = 0, db = 0, csb = 0, cdb = 0;
#pragma unroll
  for (int k = 0; k < VSA_NT_MAX_DEG; ++k)      // (static indices: the arrays stay in the kernel-argument segment)
    if (k == d) {
      Rs = g.res_src[k], pair = g.pair[k], first = g.block_first[k];
      sb = g.src_before[k], db = g.dst_before[k], csb = g.cov_src_before[k], cdb = g.cov_dst_before[k];
    }
  const int Rd = Rs >> 1, cols = pair ? Rd >> 1 : Rd;
  const long long item = (long long)(rem - first) * MIP_BLOCK + threadIdx.x;
  if (item >= mip_items(Rs, pair, d)) return;
  const int cp = (int)(item % cols), r = (int)((item / cols) % Rd), i = (int)(item / ((long long)cols * Rd));
  const uint32_t* simg = reinterpret_cast<const uint32_t*>(src + shell * g.src_stride + sb + i * nt_plane_bytes(Rs));
  uint32_t* dimg = reinterpret_cast<uint32_t*>(dst + shell * g.dst_stride + db + i * nt_plane_bytes(Rd));
  const uint8_t* scov = src_cover ? src_cover + shell * g.cov_src_stride + csb : nullptr;
  uint8_t* dcov = (dst_cover && i == 0) ? dst_cover + shell * g.cov_dst_stride + cdb : nullptr;
  const long long top = (long long)(2 * r) * Rs;              // first child row, in texels
  if (pair) {
    const uint4 a = *reinterpret_cast<const uint4*>(simg + top + 4 * cp);
    const uint4 b = *reinterpret_cast<const uint4*>(simg + top + Rs + 4 * cp);
    unsigned ca = 0x01010101u, cb = 0x01010101u;
    if (scov) {
      ca = *reinterpret_cast<const uint32_t*>(scov + top + 4 * cp);
      cb = *reinterpret_cast<const uint32_t*>(scov + top + Rs + 4 * cp);
    }
    const unsigned p0[4] = {a.x, a.y, b.x, b.y}, p1[4] = {a.z, a.w, b.z, b.w};
    const unsigned c0[4] = {ca & 0xffu, (ca >> 8) & 0xffu, cb & 0xffu, (cb >> 8) & 0xffu};
    const unsigned c1[4] = {(ca >> 16) & 0xffu, ca >> 24, (cb >> 16) & 0xffu, cb >> 24};
    unsigned any0, any1;
    const unsigned q0 = mip_texel(p0, c0, &any0), q1 = mip_texel(p1, c1, &any1);
    *reinterpret_cast<uint2*>(dimg + (long long)r * Rd + 2 * cp) = make_uint2(q0, q1);
    if (dcov) {
      dcov[(long long)r * Rd + 2 * cp] = (uint8_t)any0;
      dcov[(long long)r * Rd + 2 * cp + 1] = (uint8_t)any1;
    }
  } else {
    const long long c = 2 * cp;
    const unsigned p[4] = {simg[top + c], simg[top + c + 1], simg[top + Rs + c], simg[top + Rs + c + 1]};
    unsigned cv[4] = {1, 1, 1, 1};
    if (scov) {
      cv[0] = scov[top + c], cv[1] = scov[top + c + 1];
      cv[2] = scov[top + Rs + c], cv[3] = scov[top + Rs + c + 1];
    }
    unsigned any;
    dimg[(long long)r * Rd + cp] = mip_texel(p, cv, &any);
    if (dcov) dcov[(long long)r * Rd + cp] = (uint8_t)any;
  }
}

__global__ void __launch_bounds__(MIP_BLOCK)
texmip_density_kernel(const float4* __restrict__ tris, const float* __restrict__ face_uvs, long long nr_slots,
                      float* __restrict__ density) {
  const long long t = (long long)blockIdx.x * MIP_BLOCK + threadIdx.x;
  if (t >= nr_slots) return;
  const float4 e1 = tris[3 * t + 1], e2 = tris[3 * t + 2];
  const float* uv = face_uvs + 6 * t;
  const float du1 = uv[2] - uv[0], dv1 = uv[3] - uv[1], du2 = uv[4] - uv[0], dv2 = uv[5] - uv[1];
  const float a2 = fabsf(du1 * dv2 - dv1 * du2);
  const float cx = e1.y * e2.z - e1.z * e2.y, cy = e1.z * e2.x - e1.x * e2.z, cz = e1.x * e2.y - e1.y * e2.x;
  const float a3 = sqrtf((cx * cx + cy * cy) + cz * cz);
  const float q = a2 / a3;
  density[t] = (a3 > 0.f && q - q == 0.f) ? q : 0.f;       // (q - q == 0: q is finite)
}

// The level and the fraction of a footprint of A texels^2 in a chain of L levels above level 0.
__device__ __forceinline__ void mip_level(float A, int L, int& l, float& f) {
  l = 0;
  f = 0.f;
  if (!(A >= 1.0f)) return;                                   // magnification, or NaN: level 0 alone
  const int l0 = ((int)(__float_as_uint(A) >> 23) - 127) >> 1;   // floor(log4 A) from the exponent (A >= 1: no sign bit)
  if (l0 >= L) {
    l = L;                                                    // the top level alone (+inf lands here: l0 = 64)
    return;
  }
  const float scale = __uint_as_float((unsigned)(127 - 2 * l0) << 23);   // 4^-l0, exact
  f = (A * scale - 1.0f) * 0.333333343f;
  l = l0;
}

struct MipChain {
  const uint32_t* level[VSA_TEXMIP_MAX_LEVELS];    // planes of level 1 .. L
  int levels;
};

// Band d's 28 lerp sums from the planes of level l >= 1: nt_footprint at R_d >> l, corners clamped to the edge.
__device__ __forceinline__ void mip_plane_sums(const vsa_nt_plan& plan, const MipChain& chain, int shell, int d, int l,
                                               float u, float v, const float* s_lut, float acc[28]) {
  const int n = 2 * d + 1, R = plan.tex_res[d] >> l;
  const uint32_t* planes = chain.level[0];
#pragma unroll
  for (int k = 1; k < VSA_TEXMIP_MAX_LEVELS; ++k) planes = (l == k + 1) ? chain.level[k] : planes;
  long long stride, before;
  nt_plane_layout(plan.tex_res, plan.rgb_degrees, d, &stride, &before);     // level 0's; level l's is 4^-l of it, exactly
  const uint32_t* img = planes + (((long long)shell * stride + before) >> (2 * l + 2));
  const bool anchor = plan.anchor != 0;
  const NtFootprint fp = nt_footprint(u, v, R, anchor);
  const float w[4] = {(1.0f - fp.fx) * (1.0f - fp.fy), fp.fx * (1.0f - fp.fy), (1.0f - fp.fx) * fp.fy, fp.fx * fp.fy};
  int pix[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ky = anchor ? 0 : k >> 1, kx = anchor ? 0 : k & 1;
    const int iy = min(max(fp.j0 + ky, 0), R - 1), ix = min(max(fp.i0 + kx, 0), R - 1);
    pix[k] = (R - 1 - ix) * R + iy;           // texel (iy, ix) is pixel (R-1-ix, iy); R <= 8192: below 2^26
  }
  const float* lut = s_lut + d * 256;
#pragma unroll
  for (int i = 0; i < n; ++i) {
    const uint32_t* pl = img + (long long)i * R * R;
    unsigned px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k] = pl[pix[k]];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[i] = acc[i] + lut[px[k] & 255u] * w[k];
      acc[n + i] = acc[n + i] + lut[(px[k] >> 8) & 255u] * w[k];
      acc[2 * n + i] = acc[2 * n + i] + lut[(px[k] >> 16) & 255u] * w[k];
      acc[21 + i] = acc[21 + i] + lut[px[k] >> 24] * w[k];
    }
  }
}

template <bool FULL4>
__global__ __launch_bounds__(SH_BLOCK, 2) void nt_shade_mip_kernel(
    vsa_nt_plan plan, const int* __restrict__ hit_slot, const float* __restrict__ tex_uv,
    const float* __restrict__ rays_d, const float4* __restrict__ tris, const int* __restrict__ slot_of,
    const int* __restrict__ seg_start, const unsigned* __restrict__ texels, int N, const float* __restrict__ hit_t,
    const float* __restrict__ slot_density, float spread2, const MipChain chain, float* __restrict__ surfs_rgb,
    float* __restrict__ surfs_alpha, float* __restrict__ surfs_normals, float* __restrict__ coeffs_out,
    float* __restrict__ lod_out) {
  __shared__ float s_lut[VSA_NT_MAX_DEG * 256];
  build_lut(plan, s_lut);
  __syncthreads();
  const int K = plan.nr_shells, D = plan.rgb_degrees;
  const ShadeIdx wi = shade_idx(K, (N + SH_BLOCK - 1) / SH_BLOCK);
  const long long n = wi.tile * SH_BLOCK + threadIdx.x;
  const int s = wi.shell;
  if (!wi.valid) return;
  if (n >= N) return;
  // the pixel's footprint on the surface, in uv^2
  const long long o = (long long)s * N + n;
  const int tslot = hit_slot[o];
  float a_uv = 0.f, u = 0.f, v = 0.f;
  if (tslot >= 0) {
    const float4 e1 = tris[3 * (long long)tslot + 1], e2 = tris[3 * (long long)tslot + 2];
    const float cx = e1.y * e2.z - e1.z * e2.y, cy = e1.z * e2.x - e1.x * e2.z, cz = e1.x * e2.y - e1.y * e2.x;
    const float dx = rays_d[3 * n], dy = rays_d[3 * n + 1], dz = rays_d[3 * n + 2];
    const float nn = (cx * cx + cy * cy) + cz * cz, dd = (dx * dx + dy * dy) + dz * dz;
    const float nd = fabsf((cx * dx + cy * dy) + cz * dz);
    const float cs = fmaxf(nd / sqrtf(nn * dd), 0.125f);       // (a NaN cosine takes the clamp)
    const float t = hit_t[o];
    a_uv = (((t * t) * spread2) * slot_density[tslot]) / cs;
    u = tex_uv[2 * o], v = tex_uv[2 * o + 1];
  } else if (lod_out) {
    for (int d = 0; d < D; ++d) lod_out[o * D + d] = __uint_as_float(0x7fc00000u);
  }
  nt_shade_ray<FULL4>(
      plan, s, n, N, hit_slot, tex_uv, rays_d, tris, slot_of, seg_start, surfs_rgb, surfs_alpha, surfs_normals, coeffs_out,
      nullptr, [&](int d, const HitCtx& c, float acc[28]) {
        const float Rf = (float)plan.tex_res[d];
        int l;
        float f;
        mip_level(a_uv * (Rf * Rf), chain.levels, l, f);
        if (lod_out) lod_out[o * D + d] = (float)l + f;
        if (l == 0)
          row_sums<false>(plan, d, c, texels, s_lut, acc);       // the scene's own bank, as vsa_nt_shade_fwd reads it
        else
          mip_plane_sums(plan, chain, s, d, l, u, v, s_lut, acc);
        if (f > 0.f) {                                           // (f > 0 only below the top level: l + 1 <= L)
          float up[28];
#pragma unroll
          for (int i = 0; i < 28; ++i) up[i] = 0.f;
          mip_plane_sums(plan, chain, s, d, l + 1, u, v, s_lut, up);
#pragma unroll
          for (int i = 0; i < 28; ++i) {
            const float c0 = vsa_round_f16(acc[i]), c1 = vsa_round_f16(up[i]);
            acc[i] = c0 + f * (c1 - c0);                         // rounded to fp16 by shade_hit
          }
        }
      });
}

// The plan checks of the three entry points: nt_common.h's, in the order of the sibling stages (an unsupported plan is
// reported before a bad resolution), then the chain's: levels in 1..8, every resolution divisible by 2^levels.
int mip_check_plan(const vsa_nt_plan* p, int levels) {
  if (const int rc = nt_baked_plan_counts(p)) return rc;
  if (const int rc = nt_baked_plan_supported(p)) return rc;
  if (const int rc = nt_baked_plan_resolutions(p)) return rc;
  if (levels < 1 || levels > VSA_TEXMIP_MAX_LEVELS) return VSA_ERR_ARG;
  for (int d = 0; d < p->rgb_degrees; ++d)
    if (p->tex_res[d] % (1 << levels)) return VSA_ERR_ARG;
  return VSA_OK;
}

inline bool mip_misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" long long vsa_texmip_planes_bytes(const vsa_nt_plan* plan, int level) {
  if (level == 0) {
    if (const int rc = nt_baked_plan_counts(plan)) return rc;
    if (const int rc = nt_baked_plan_supported(plan)) return rc;
    if (const int rc = nt_baked_plan_resolutions(plan)) return rc;
  } else if (const int rc = mip_check_plan(plan, level)) {
    return rc;
  }
  return nt_plane_offset(*plan, plan->nr_shells, 0) >> (2 * level);
}

extern "C" int vsa_texmip_reduce(const vsa_nt_plan* plan, int level, const uint8_t* src_planes,
                                 long long src_planes_bytes, const uint8_t* src_cover, uint8_t* dst_planes,
                                 long long dst_planes_bytes, uint8_t* dst_cover, void* stream) {
  if (const int rc = mip_check_plan(plan, level)) return rc;
  if (!src_planes || !dst_planes || src_planes == dst_planes) return VSA_ERR_ARG;
  if (mip_misaligned(src_planes, 16) || mip_misaligned(dst_planes, 16) || mip_misaligned(src_cover, 16) ||
      mip_misaligned(dst_cover, 16))
    return VSA_ERR_ARG;
  const long long total = nt_plane_offset(*plan, plan->nr_shells, 0);
  if (src_planes_bytes != total >> (2 * (level - 1)) || dst_planes_bytes != total >> (2 * level)) return VSA_ERR_ARG;
  MipGeom g = {};
  g.degrees = plan->rgb_degrees;
  int32_t rs[VSA_NT_MAX_DEG] = {}, rd[VSA_NT_MAX_DEG] = {};
  for (int d = 0; d < g.degrees; ++d) {
    rs[d] = g.res_src[d] = plan->tex_res[d] >> (level - 1);
    rd[d] = rs[d] >> 1;
  }
  for (int d = 0; d < g.degrees; ++d) {
    nt_plane_layout(rs, g.degrees, d, &g.src_stride, &g.src_before[d]);
    nt_plane_layout(rd, g.degrees, d, &g.dst_stride, &g.dst_before[d]);
    g.cov_src_before[d] = d ? g.cov_src_before[d - 1] + (long long)rs[d - 1] * rs[d - 1] : 0;
    g.cov_dst_before[d] = d ? g.cov_dst_before[d - 1] + (long long)rd[d - 1] * rd[d - 1] : 0;
  }
  g.cov_src_stride = g.cov_src_before[g.degrees - 1] + (long long)rs[g.degrees - 1] * rs[g.degrees - 1];
  g.cov_dst_stride = g.cov_dst_before[g.degrees - 1] + (long long)rd[g.degrees - 1] * rd[g.degrees - 1];
  long long blocks = 0;
  for (int d = 0; d < g.degrees; ++d) {
    // two texels per lane where every 8-byte store is aligned: an even row, on an 8-byte plane and shell offset
    g.pair[d] = (rd[d] % 2 == 0 && g.dst_before[d] % 8 == 0 && g.dst_stride % 8 == 0) ? 1 : 0;
    g.block_first[d] = (int)blocks;
    blocks += (mip_items(rs[d], g.pair[d], d) + MIP_BLOCK - 1) / MIP_BLOCK;
    if (blocks * plan->nr_shells >= (1ll << 31)) return VSA_ERR_UNSUPPORTED;
  }
  g.block_first[g.degrees] = (int)blocks;
  hipLaunchKernelGGL(texmip_reduce_kernel, dim3((unsigned)(blocks * plan->nr_shells)), dim3(MIP_BLOCK), 0,
                     (hipStream_t)stream, g, src_planes, src_cover, dst_planes, dst_cover);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_texmip_density(const float* tris, const float* face_uvs, long long nr_slots, float* density,
                                  void* stream) {
  if (!tris || !face_uvs || !density || nr_slots < 1) return VSA_ERR_ARG;
  if (mip_misaligned(tris, 16) || mip_misaligned(face_uvs, 16) || mip_misaligned(density, 16)) return VSA_ERR_ARG;
  if ((nr_slots + MIP_BLOCK - 1) / MIP_BLOCK >= (1ll << 31)) return VSA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(texmip_density_kernel, dim3((unsigned)((nr_slots + MIP_BLOCK - 1) / MIP_BLOCK)), dim3(MIP_BLOCK),
                     0, (hipStream_t)stream, reinterpret_cast<const float4*>(tris), face_uvs, nr_slots, density);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_nt_shade_mip_fwd(const vsa_nt_plan* plan, const int32_t* hit_slot, const float* tex_uv,
                                    const float* rays_d, const float* tris, const int32_t* slot_of,
                                    const int32_t* seg_start, const uint8_t* texels, int nr_rays, const float* hit_t,
                                    const float* slot_density, float spread2, int levels,
                                    const uint8_t* const* level_planes, float* surfs_rgb, float* surfs_alpha,
                                    float* surfs_normals, float* coeffs_out, float* lod_out, void* stream) {
  if (const int rc = mip_check_plan(plan, levels)) return rc;
  if (nr_rays < 0 || !(spread2 >= 0.f) || spread2 - spread2 != 0.f) return VSA_ERR_ARG;
  if (!hit_slot || !tex_uv || !rays_d || !tris || !slot_of || !seg_start || !texels || !hit_t || !slot_density ||
      !level_planes || !surfs_rgb || !surfs_alpha)
    return VSA_ERR_ARG;
  const void* aligned[] = {hit_slot, tex_uv, rays_d, tris, slot_of, seg_start, texels, hit_t, slot_density,
                           surfs_rgb, surfs_alpha, surfs_normals, coeffs_out, lod_out};
  for (const void* p : aligned)
    if (mip_misaligned(p, 16)) return VSA_ERR_ARG;
  MipChain chain = {};
  chain.levels = levels;
  for (int l = 0; l < levels; ++l) {
    if (!level_planes[l] || mip_misaligned(level_planes[l], 16)) return VSA_ERR_ARG;
    chain.level[l] = reinterpret_cast<const uint32_t*>(level_planes[l]);
  }
  if (nr_rays == 0) return VSA_OK;
  dim3 grid = shade_grid(vsa_div_up(nr_rays, SH_BLOCK), plan->nr_shells);
#define VSA_MIP_LAUNCH(FULL4)                                                                                          \
  hipLaunchKernelGGL(nt_shade_mip_kernel<FULL4>, grid, dim3(SH_BLOCK), 0, (hipStream_t)stream, *plan, hit_slot, tex_uv, \
                     rays_d, reinterpret_cast<const float4*>(tris), slot_of, seg_start,                                 \
                     reinterpret_cast<const unsigned*>(texels), nr_rays, hit_t, slot_density, spread2, chain,           \
                     surfs_rgb, surfs_alpha, surfs_normals, coeffs_out, lod_out)
  if (plan->rgb_degrees == VSA_NT_MAX_DEG)
    VSA_MIP_LAUNCH(true);
  else
    VSA_MIP_LAUNCH(false);
#undef VSA_MIP_LAUNCH
  VSA_RETURN_LAUNCH_STATUS();
}
