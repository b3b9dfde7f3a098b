// A split's decoded PNG bytes to the float stacks every consumer reads (volsurfs_amd/datasets.py): alpha over a
// background colour, box subsampling by an integer factor and the mask, in one launch.  The reference takes its images
// from mvdatasets, an empty submodule in its checkout: the rule is this library's own (include/volsurfs_hip.h "Image
// preparation"), restated in tests/datasets_restated.py, PARITY UNPINNED.
//
// One lane per OUTPUT pixel, lanes along a row: a wave reads 64 * s consecutive texels of each of its s source rows (a
// dword per RGBA texel) and writes 64 consecutive 12-byte pixels.  The sums over the s * s texels are integers (at most
// 255 * 255 * 256 < 2^24, exact in fp32 too); the only rounded operations are two divisions, one subtraction, one
// multiply and one add per channel, each rounded once (no contraction), so that numpy float32 restates them bit for bit.
// Bandwidth-bound: ch + 1 bytes read and 16 written per texel at s = 1.
#include "common.h"

namespace {

struct __attribute__((packed, aligned(4))) F3 {      // a [.,3] f32 record: 4-byte aligned, moved as one dwordx3
  float x, y, z;
};

template <int CH>
__global__ __launch_bounds__(256) void images_prepare_kernel(
    const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask, int H0, int W0, int H, int W, int s,
    int blocks_per_row, float bg0, float bg1, float bg2, float* __restrict__ rgb, float* __restrict__ out_mask) {
#pragma clang fp contract(off)
  const long long out_row = blockIdx.x / blocks_per_row;            // image * H + y: the same in every lane
  const int x = (int)(blockIdx.x % blocks_per_row) * 256 + (int)threadIdx.x;
  if (x >= W) return;
  const long long img = out_row / H;
  const int y = (int)(out_row % H);
  uint32_t A = 0, P0 = 0, P1 = 0, P2 = 0, M = 0;
  for (int dy = 0; dy < s; ++dy) {
    const long long texel0 = (img * H0 + ((long long)y * s + dy)) * W0 + (long long)x * s;
    for (int dx = 0; dx < s; ++dx) {
      const long long t = texel0 + dx;
      uint32_t c0, c1, c2, a = 255u;
      if constexpr (CH == 4) {
        const uint32_t v = reinterpret_cast<const uint32_t*>(src)[t];      // R, G, B, A from the low byte up
        c0 = v & 255u, c1 = (v >> 8) & 255u, c2 = (v >> 16) & 255u, a = v >> 24;
      } else if constexpr (CH == 3) {
        c0 = src[3 * t], c1 = src[3 * t + 1], c2 = src[3 * t + 2];
      } else {
        c0 = c1 = c2 = src[t];
      }
      A += a, P0 += c0 * a, P1 += c1 * a, P2 += c2 * a;
      if (mask) M += mask[t];
    }
  }
  const uint32_t n = (uint32_t)(s * s);
  const float alpha = __fdiv_rn((float)A, (float)(255u * n));
  const float den = (float)(65025u * n);
  const float rest = __fsub_rn(1.0f, alpha);
  F3 out;
  out.x = __fadd_rn(__fdiv_rn((float)P0, den), __fmul_rn(rest, bg0));
  out.y = __fadd_rn(__fdiv_rn((float)P1, den), __fmul_rn(rest, bg1));
  out.z = __fadd_rn(__fdiv_rn((float)P2, den), __fmul_rn(rest, bg2));
  const long long px = out_row * W + x;
  *reinterpret_cast<F3*>(rgb + 3 * px) = out;
  if (out_mask) out_mask[px] = mask ? __fdiv_rn((float)M, (float)(255u * n)) : alpha;
}

}  // namespace

extern "C" int vsa_images_prepare(const uint8_t* src, const uint8_t* mask, int C, int H0, int W0, int ch, int s,
                                  const float* bg, float* rgb, float* out_mask, void* stream) {
  if (s < 1 || s > 16 || (ch != 1 && ch != 3 && ch != 4) || C < 0 || H0 < 0 || W0 < 0) return VSA_ERR_ARG;
  if ((mask != nullptr || ch == 4) ? false : out_mask != nullptr) return VSA_ERR_ARG;   // no mask to write
  if (mask && !out_mask) return VSA_ERR_ARG;
  const int H = H0 / s, W = W0 / s;
  if (C == 0 || H == 0 || W == 0) return VSA_OK;
  if (!src || !bg || !rgb) return VSA_ERR_ARG;
  if (ch == 4 && (reinterpret_cast<uintptr_t>(src) & 3u)) return VSA_ERR_ARG;           // texels are read as dwords
  const int blocks_per_row = vsa_div_up(W, 256);
  const long long blocks = (long long)C * H * blocks_per_row;
  if (blocks > 0x7fffffffll) return VSA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks), block(256);
  const hipStream_t st = (hipStream_t)stream;
  switch (ch) {
    case 4: hipLaunchKernelGGL(images_prepare_kernel<4>, grid, block, 0, st, src, mask, H0, W0, H, W, s, blocks_per_row, bg[0], bg[1], bg[2], rgb, out_mask); break;
    case 3: hipLaunchKernelGGL(images_prepare_kernel<3>, grid, block, 0, st, src, mask, H0, W0, H, W, s, blocks_per_row, bg[0], bg[1], bg[2], rgb, out_mask); break;
    default: hipLaunchKernelGGL(images_prepare_kernel<1>, grid, block, 0, st, src, mask, H0, W0, H, W, s, blocks_per_row, bg[0], bg[1], bg[2], rgb, out_mask); break;
  }
  VSA_RETURN_LAUNCH_STATUS();
}
