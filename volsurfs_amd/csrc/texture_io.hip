// Baked neural textures <-> the RGBA8 planes of the exported PNGs (the baker's `--extract_textures`,
// volsurfs_py/baker.py:778-1009; rules in include/volsurfs_hip.h and DESIGN §17).
//
// Both kernels only move bytes.  PNG pixel (r, c) of (shell, d) holds texel (iy, ix) = (c, R-1-r) of the network's
// grid, so the image is a transpose of the texel rows: a 32 x 32 tile is staged through LDS as [coefficient][png row]
// [png column] dwords (one RGBA pixel each, pitch 33 so that neither side conflicts).  On the texel-row side the 32
// lanes of a half-wave walk one texel row (consecutive slots: contiguous 8-32 byte rows, slot_of contiguous); on the
// image side 8 lanes store one png row's 128 bytes as 16-byte vectors.  Every pixel and every texel row is written by
// exactly one lane: the results are deterministic.
#include "nt_common.h"

#define TIO_TILE 32
#define TIO_PITCH 33
#define TIO_THREADS 256
#define TIO_MAX_COEFFS 7

typedef uint32_t TioLds[TIO_TILE][TIO_PITCH];

__host__ __device__ static inline int tio_tiles(int R) {
  const int t = (R + TIO_TILE - 1) / TIO_TILE;
  return t * t;
}
// Apron texels of one (R+2)^2 domain: 4 (R+2) - 4.
__host__ __device__ static inline int tio_apron_texels(int R) { return 4 * (R + 2) - 4; }
__host__ __device__ static inline int tio_apron_blocks(int R) {
  return (tio_apron_texels(R) + TIO_THREADS - 1) / TIO_THREADS;
}
__host__ __device__ static inline int tio_blocks_per_shell(const vsa_nt_plan& p, bool apron) {
  int n = 0;
  for (int d = 0; d < p.rgb_degrees; ++d) n += tio_tiles(p.tex_res[d]) + (apron ? tio_apron_blocks(p.tex_res[d]) : 0);
  return n;
}

// Byte k of a texel row held as dwords (k is a compile-time constant in every caller).
template <int Q>
__device__ __forceinline__ uint32_t tio_byte(const uint32_t (&w)[Q], int k) {
  return (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
}

template <int Q>
__device__ __forceinline__ void tio_load_row(const uint8_t* src, uint32_t (&w)[Q]) {
  if constexpr (Q == 2) {
    const uint2 a = *reinterpret_cast<const uint2*>(src);
    w[0] = a.x; w[1] = a.y;
  } else {
#pragma unroll
    for (int h = 0; h < Q / 4; ++h) {
      const uint4 a = reinterpret_cast<const uint4*>(src)[h];
      w[4 * h] = a.x; w[4 * h + 1] = a.y; w[4 * h + 2] = a.z; w[4 * h + 3] = a.w;
    }
  }
}

template <int Q>
__device__ __forceinline__ void tio_store_row(uint8_t* dst, const uint32_t (&w)[Q]) {
  if constexpr (Q == 2) {
    *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
  } else {
#pragma unroll
    for (int h = 0; h < Q / 4; ++h)
      reinterpret_cast<uint4*>(dst)[h] = make_uint4(w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]);
  }
}

// RGBA dword of coefficient i from a texel row: r, g, b = rgb channels 0..2 (element channel * n + i), a = the alpha
// coefficient, or 255 on a shell without an alpha model.
template <int D>
__device__ __forceinline__ uint32_t tio_pixel(const uint32_t (&w)[VSA_NT_ROW_QUADS(D)], int i, bool has_alpha) {
  constexpr int N = 2 * D + 1, AQ = VSA_NT_ALPHA_QUAD(D);
  const uint32_t a = has_alpha ? tio_byte(w, 4 * AQ + i) : 0xffu;
  return tio_byte(w, i) | (tio_byte(w, N + i) << 8) | (tio_byte(w, 2 * N + i) << 16) | (a << 24);
}

// The inverse: a texel row from the N RGBA dwords of one pixel (padding and, without alpha, the alpha elements zero:
// what the baking kernels leave there).
template <int D>
__device__ __forceinline__ void tio_row_of(const uint32_t* px, int stride, bool has_alpha,
                                           uint32_t (&w)[VSA_NT_ROW_QUADS(D)]) {
  constexpr int N = 2 * D + 1, Q = VSA_NT_ROW_QUADS(D), AQ = VSA_NT_ALPHA_QUAD(D);
#pragma unroll
  for (int k = 0; k < Q; ++k) w[k] = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t v = px[i * stride];
    const int e[4] = {i, N + i, 2 * N + i, 4 * AQ + i};
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      if (ch == 3 && !has_alpha) continue;
      w[e[ch] >> 2] |= ((v >> (8 * ch)) & 0xffu) << (8 * (e[ch] & 3));
    }
  }
}

template <int D>
__device__ void tio_export_tile(const vsa_nt_plan& p, int shell, int tile, const NtRowSeg& s, const uint8_t* texels,
                                uint8_t* planes, TioLds* lds) {
  constexpr int N = 2 * D + 1, Q = VSA_NT_ROW_QUADS(D);
  const int R = p.tex_res[D], W = R + 2, tx = (R + TIO_TILE - 1) / TIO_TILE;
  const int r0 = (tile / tx) * TIO_TILE, c0 = (tile % tx) * TIO_TILE;
  const bool has_alpha = nt_shell_has_alpha(p, shell);
  // texel rows -> LDS: a half-wave walks 32 png rows of one png column = 32 consecutive texels of one texel row
  for (int k = threadIdx.x; k < TIO_TILE * TIO_TILE; k += TIO_THREADS) {
    const int pr = k % TIO_TILE, pc = k / TIO_TILE;
    const int r = r0 + pr, c = c0 + pc;
    if (r >= R || c >= R) continue;
    const int row = nt_seg_row(s, (long long)(c + 1) * W + (R - r));       // (iy, ix) = (c, R-1-r), apron offset 1
    uint32_t w[Q];
    if (row >= 0)
      tio_load_row<Q>(texels + s.row0 + (long long)row * Q * 4, w);
    else
#pragma unroll
      for (int q = 0; q < Q; ++q) w[q] = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) lds[i][pr][pc] = tio_pixel<D>(w, i, has_alpha);
  }
  __syncthreads();
  // LDS -> planes: 8 lanes store one png row's 32 pixels as 16-byte vectors
  const int pr = threadIdx.x / 8, g = threadIdx.x % 8;
  const int r = r0 + pr, c = c0 + 4 * g;
  if (r >= R || c >= R) return;
  uint8_t* dst = planes + nt_plane_offset(p, shell, D) + ((long long)r * R + c) * 4;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t* src = &lds[i][pr][4 * g];
    uint8_t* d = dst + i * nt_plane_bytes(R);
    if ((R & 3) == 0) {
      *reinterpret_cast<uint4*>(d) = make_uint4(src[0], src[1], src[2], src[3]);
    } else {
      for (int j = 0; j < 4 && c + j < R; ++j) reinterpret_cast<uint32_t*>(d)[j] = src[j];
    }
  }
}

template <int D>
__device__ void tio_import_tile(const vsa_nt_plan& p, int shell, int tile, const NtRowSeg& s, const uint8_t* planes,
                                uint8_t* texels, TioLds* lds) {
  constexpr int Q = VSA_NT_ROW_QUADS(D), N = 2 * D + 1;
  const int R = p.tex_res[D], W = R + 2, tx = (R + TIO_TILE - 1) / TIO_TILE;
  const int r0 = (tile / tx) * TIO_TILE, c0 = (tile % tx) * TIO_TILE;
  const bool has_alpha = nt_shell_has_alpha(p, shell);
  {  // planes -> LDS: 16-byte loads along png rows
    const int pr = threadIdx.x / 8, g = threadIdx.x % 8;
    const int r = r0 + pr, c = c0 + 4 * g;
    if (r < R && c < R) {
      const uint8_t* src = planes + nt_plane_offset(p, shell, D) + ((long long)r * R + c) * 4;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        uint32_t* dst = &lds[i][pr][4 * g];
        const uint8_t* sp = src + i * nt_plane_bytes(R);
        if ((R & 3) == 0) {
          const uint4 v = *reinterpret_cast<const uint4*>(sp);
          dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        } else {
          for (int j = 0; j < 4 && c + j < R; ++j) dst[j] = reinterpret_cast<const uint32_t*>(sp)[j];
        }
      }
    }
  }
  __syncthreads();
  // LDS -> texel rows: a half-wave writes 32 consecutive texels of one texel row
  for (int k = threadIdx.x; k < TIO_TILE * TIO_TILE; k += TIO_THREADS) {
    const int pr = k % TIO_TILE, pc = k / TIO_TILE;
    const int r = r0 + pr, c = c0 + pc;
    if (r >= R || c >= R) continue;
    const int row = nt_seg_row(s, (long long)(c + 1) * W + (R - r));
    if (row < 0) continue;
    uint32_t w[Q];
    tio_row_of<D>(&lds[0][pr][pc], TIO_TILE * TIO_PITCH, has_alpha, w);
    tio_store_row<Q>(texels + s.row0 + (long long)row * Q * 4, w);
  }
}

// Apron texels (domain row or column 0 or R+1): clamp to the edge, i.e. the row of the nearest interior texel, read
// straight from the planes (4 R + 4 texels per domain; not worth a tile).
template <int D>
__device__ void tio_import_apron(const vsa_nt_plan& p, int shell, int block, const NtRowSeg& s, const uint8_t* planes,
                                 uint8_t* texels) {
  constexpr int Q = VSA_NT_ROW_QUADS(D);
  const int R = p.tex_res[D], W = R + 2;
  const int a = block * TIO_THREADS + threadIdx.x;
  if (a >= tio_apron_texels(R)) return;
  int Y, X;
  if (a < W) {
    Y = 0; X = a;
  } else if (a < 2 * W) {
    Y = W - 1; X = a - W;
  } else {
    const int k = a - 2 * W;
    Y = 1 + k / 2; X = (k & 1) ? W - 1 : 0;
  }
  const int row = nt_seg_row(s, (long long)Y * W + X);
  if (row < 0) return;
  const int iy = min(max(Y - 1, 0), R - 1), ix = min(max(X - 1, 0), R - 1);
  const uint32_t* px = reinterpret_cast<const uint32_t*>(planes + nt_plane_offset(p, shell, D)) +
                       ((long long)(R - 1 - ix) * R + iy);
  uint32_t w[Q];
  tio_row_of<D>(px, (int)(nt_plane_bytes(R) / 4), nt_shell_has_alpha(p, shell), w);
  tio_store_row<Q>(texels + s.row0 + (long long)row * Q * 4, w);
}

// Block b of a launch: shell b / per_shell, then the degrees' tiles (and, importing, their apron blocks) in order.
__device__ __forceinline__ void tio_decode(const vsa_nt_plan& p, bool apron, int& shell, int& deg, int& idx,
                                           bool& is_apron) {
  const int per = tio_blocks_per_shell(p, apron);
  shell = blockIdx.x / per;
  int rem = blockIdx.x % per;
  for (deg = 0; deg < p.rgb_degrees; ++deg) {
    const int t = tio_tiles(p.tex_res[deg]);
    if (rem < t) {
      idx = rem; is_apron = false;
      return;
    }
    rem -= t;
    if (apron) {
      const int a = tio_apron_blocks(p.tex_res[deg]);
      if (rem < a) {
        idx = rem; is_apron = true;
        return;
      }
      rem -= a;
    }
  }
  deg = -1;
}

__global__ void __launch_bounds__(TIO_THREADS)
tio_export_kernel(const vsa_nt_plan p, const int32_t* __restrict__ slot_of, const int32_t* __restrict__ seg_start,
                  const uint8_t* __restrict__ texels, uint8_t* __restrict__ planes) {
  __shared__ uint32_t lds[TIO_MAX_COEFFS][TIO_TILE][TIO_PITCH];
  int shell, deg, idx;
  bool is_apron;
  tio_decode(p, false, shell, deg, idx, is_apron);
  if (deg < 0) return;
  const NtRowSeg s = nt_row_seg(p, shell, deg, slot_of, seg_start);
  switch (deg) {
    case 0: tio_export_tile<0>(p, shell, idx, s, texels, planes, lds); break;
    case 1: tio_export_tile<1>(p, shell, idx, s, texels, planes, lds); break;
    case 2: tio_export_tile<2>(p, shell, idx, s, texels, planes, lds); break;
    default: tio_export_tile<3>(p, shell, idx, s, texels, planes, lds); break;
  }
}

__global__ void __launch_bounds__(TIO_THREADS)
tio_import_kernel(const vsa_nt_plan p, const uint8_t* __restrict__ planes, const int32_t* __restrict__ slot_of,
                  const int32_t* __restrict__ seg_start, uint8_t* __restrict__ texels) {
  __shared__ uint32_t lds[TIO_MAX_COEFFS][TIO_TILE][TIO_PITCH];
  int shell, deg, idx;
  bool is_apron;
  tio_decode(p, true, shell, deg, idx, is_apron);
  if (deg < 0) return;
  const NtRowSeg s = nt_row_seg(p, shell, deg, slot_of, seg_start);
  if (is_apron) {
    switch (deg) {
      case 0: tio_import_apron<0>(p, shell, idx, s, planes, texels); break;
      case 1: tio_import_apron<1>(p, shell, idx, s, planes, texels); break;
      case 2: tio_import_apron<2>(p, shell, idx, s, planes, texels); break;
      default: tio_import_apron<3>(p, shell, idx, s, planes, texels); break;
    }
    return;
  }
  switch (deg) {
    case 0: tio_import_tile<0>(p, shell, idx, s, planes, texels, lds); break;
    case 1: tio_import_tile<1>(p, shell, idx, s, planes, texels, lds); break;
    case 2: tio_import_tile<2>(p, shell, idx, s, planes, texels, lds); break;
    default: tio_import_tile<3>(p, shell, idx, s, planes, texels, lds); break;
  }
}

// nt_common.h's checks in this stage's order (an unsupported plan is reported before a bad resolution), then its own
// limit on the grid.
static int tio_check(const vsa_nt_plan* p) {
  if (const int rc = nt_baked_plan_counts(p)) return rc;
  if (const int rc = nt_baked_plan_supported(p)) return rc;
  if (const int rc = nt_baked_plan_resolutions(p)) return rc;
  long long blocks = (long long)p->nr_shells * tio_blocks_per_shell(*p, true);
  if (blocks >= (1ll << 31)) return VSA_ERR_UNSUPPORTED;
  return VSA_OK;
}

extern "C" long long vsa_nt_planes_bytes(const vsa_nt_plan* plan) {
  const int rc = tio_check(plan);
  if (rc) return rc;
  return nt_plane_offset(*plan, plan->nr_shells, 0);
}

extern "C" int vsa_nt_export_planes(const vsa_nt_plan* plan, const int32_t* slot_of, const int32_t* seg_start,
                                    const uint8_t* texels, uint8_t* planes, long long planes_bytes, void* stream) {
  const int rc = tio_check(plan);
  if (rc) return rc;
  if (!slot_of || !seg_start || !texels || !planes) return VSA_ERR_ARG;
  if (((uintptr_t)planes & 15) || ((uintptr_t)texels & 15)) return VSA_ERR_ARG;
  if (planes_bytes != nt_plane_offset(*plan, plan->nr_shells, 0)) return VSA_ERR_ARG;
  const int blocks = plan->nr_shells * tio_blocks_per_shell(*plan, false);
  hipLaunchKernelGGL(tio_export_kernel, dim3(blocks), dim3(TIO_THREADS), 0, (hipStream_t)stream, *plan, slot_of,
                     seg_start, texels, planes);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_nt_import_planes(const vsa_nt_plan* plan, const uint8_t* planes, long long planes_bytes,
                                    const int32_t* slot_of, const int32_t* seg_start, uint8_t* texels, void* stream) {
  const int rc = tio_check(plan);
  if (rc) return rc;
  if (!slot_of || !seg_start || !texels || !planes) return VSA_ERR_ARG;
  if (((uintptr_t)planes & 15) || ((uintptr_t)texels & 15)) return VSA_ERR_ARG;
  if (planes_bytes != nt_plane_offset(*plan, plan->nr_shells, 0)) return VSA_ERR_ARG;
  const int blocks = plan->nr_shells * tio_blocks_per_shell(*plan, true);
  hipLaunchKernelGGL(tio_import_kernel, dim3(blocks), dim3(TIO_THREADS), 0, (hipStream_t)stream, *plan, planes,
                     slot_of, seg_start, texels);
  VSA_RETURN_LAUNCH_STATUS();
}
