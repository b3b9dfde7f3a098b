// Projective TSDF fusion of V depth maps (utils/mesh_from_depth.py:220-300; include/volsurfs_hip.h "TSDF fusion";
// DESIGN 24).  The reference runs V passes of a dozen torch ops over the whole lattice; here a query point walks the
// views i = 0 .. V-1 in order with its running (tsdf, rgb, weight) in registers and is written once.
//   tsdf_lattice_kernel  a wave is a 4 x 4 x 4 brick of the lattice (its lanes project to a few pixels of a view, so
//                        the four depth taps of the 64 lanes share cache lines), a block four bricks along k (one
//                        (i, j) row of a block is 16 consecutive floats of the output)
//   tsdf_points_kernel   one thread per given point, optionally with the colour mean (the vertex-colour pass)
//   tsdf_uncontract_kernel  the inverse contraction and the clip of the mesh vertices
// The view matrices are indexed by the loop counter only: wave-uniform loads.  A view none of a wave's lanes sees costs
// the projection and one branch.  fp32 in the order written, no contraction (-ffp-contract=off); no atomics: the same
// inputs give the same bytes.
#include "common.h"

namespace {

constexpr int TF_BLOCK = 256;
constexpr int TF_BRICK = 4;                                   // a wave: TF_BRICK^3 = 64 lattice points
constexpr int TF_BRICKS_K = TF_BLOCK / VSA_WAVE;              // bricks of a block, stacked along k
constexpr int TF_MAX_N = 4096, TF_MAX_SIDE = 1 << 15;

struct TfViews {
  const float* __restrict__ proj;     // [V, 4, 4] full_proj_transform, row-major
  const float* __restrict__ depth;    // [V, H, W]
  const float* __restrict__ rgb;      // [V, 3, H, W] or null
  int V, H, W;
  float trunc;
};

// The inverse of the scene contraction (RaySamplerGPU.cuh:595-650 without the ray part, as packed.hip's
// uncontract_kernel).  False when the point lies outside the contraction's image (|2 p| >= 2).
__device__ __forceinline__ bool tf_uncontract(float& px, float& py, float& pz) {
  const float sx = px * 2.0f, sy = py * 2.0f, sz = pz * 2.0f;
  const float norm = sqrtf((sx * sx + sy * sy) + sz * sz);
  if (!(norm < 2.0f)) return false;
  if (norm > 1.0f) {
    const float factor = 1.0f / (2.0f - norm);
    px = (factor * px) / norm;
    py = (factor * py) / norm;
    pz = (factor * pz) / norm;
  }
  return true;
}

// grid_sample(mode="bilinear", align_corners=True) of one channel at unnormalised (ix, iy) with the corner weights
// given: the four taps in ATen's order nw, ne, sw, se, a tap outside the image left out.
__device__ __forceinline__ float tf_tap(const float* __restrict__ img, int W, int H, int x0, int y0, float nw, float ne,
                                        float sw, float se) {
  const bool xa = x0 >= 0 && x0 < W, xb = x0 + 1 >= 0 && x0 + 1 < W;
  const bool ya = y0 >= 0 && y0 < H, yb = y0 + 1 >= 0 && y0 + 1 < H;
  float out = 0.0f;
  if (xa && ya) out = out + img[(long long)y0 * W + x0] * nw;
  if (xb && ya) out = out + img[(long long)y0 * W + x0 + 1] * ne;
  if (xa && yb) out = out + img[(long long)(y0 + 1) * W + x0] * sw;
  if (xb && yb) out = out + img[(long long)(y0 + 1) * W + x0 + 1] * se;
  return out;
}

template <bool RGB>
__device__ __forceinline__ void tf_fuse(const TfViews& vw, float px, float py, float pz, float& tsdf, float rgb[3]) {
  float w = 1.0f;
  tsdf = 1.0f;
  if (RGB) rgb[0] = rgb[1] = rgb[2] = 0.0f;
  const float wm1 = (float)(vw.W - 1), hm1 = (float)(vw.H - 1);
  const long long HW = (long long)vw.H * vw.W;
  for (int i = 0; i < vw.V; ++i) {
    const float* __restrict__ P = vw.proj + 16 * i;
    const float hx = ((px * P[0] + py * P[1]) + pz * P[2]) + P[3];
    const float hy = ((px * P[4] + py * P[5]) + pz * P[6]) + P[7];
    const float z = ((px * P[12] + py * P[13]) + pz * P[14]) + P[15];
    const float u = hx / z, v = hy / z;
    if (!(u > -1.0f && u < 1.0f && v > -1.0f && v < 1.0f && z > 0.0f)) continue;
    float ix = ((u + 1.0f) / 2.0f) * wm1, iy = ((v + 1.0f) / 2.0f) * hm1;
    ix = fminf(fmaxf(ix, 0.0f), wm1), iy = fminf(fmaxf(iy, 0.0f), hm1);      // border padding
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float ex = (fx + 1.0f) - ix, ey = (fy + 1.0f) - iy, dx = ix - fx, dy = iy - fy;
    const float nw = ex * ey, ne = dx * ey, sw = ex * dy, se = dx * dy;
    const float d = tf_tap(vw.depth + i * HW, vw.W, vw.H, x0, y0, nw, ne, sw, se);
    const float sdf = d - z;
    if (!(sdf > -vw.trunc)) continue;
    const float s = fminf(fmaxf(sdf / vw.trunc, -1.0f), 1.0f);
    const float wp = w + 1.0f;
    tsdf = (tsdf * w + s) / wp;
    if (RGB) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float col = tf_tap(vw.rgb + (3ll * i + c) * HW, vw.W, vw.H, x0, y0, nw, ne, sw, se);
        rgb[c] = (rgb[c] * w + col) / wp;
      }
    }
    w = wp;
  }
}

__global__ void __launch_bounds__(TF_BLOCK)
tsdf_lattice_kernel(TfViews vw, const float* __restrict__ axis, int n, int uncontract, float* __restrict__ out) {
  const int lane = threadIdx.x & (VSA_WAVE - 1), brick = threadIdx.x / VSA_WAVE;
  const int i = blockIdx.z * TF_BRICK + (lane >> 4);
  const int j = blockIdx.y * TF_BRICK + ((lane >> 2) & 3);
  const int k = (blockIdx.x * TF_BRICKS_K + brick) * TF_BRICK + (lane & 3);
  if (i >= n || j >= n || k >= n) return;
  float px = axis[i], py = axis[j], pz = axis[k];
  float tsdf = 1.0f, unused[3];
  if (!uncontract || tf_uncontract(px, py, pz)) tf_fuse<false>(vw, px, py, pz, tsdf, unused);
  out[((long long)i * n + j) * n + k] = tsdf;
}

template <bool RGB>
__global__ void __launch_bounds__(TF_BLOCK)
tsdf_points_kernel(TfViews vw, const float* __restrict__ points, long long nr_points, int uncontract,
                   float* __restrict__ out_tsdf, float* __restrict__ out_rgb) {
  const long long p = (long long)blockIdx.x * TF_BLOCK + threadIdx.x;
  if (p >= nr_points) return;
  float px = points[3 * p], py = points[3 * p + 1], pz = points[3 * p + 2];
  float tsdf = 1.0f, rgb[3] = {0.0f, 0.0f, 0.0f};
  if (!uncontract || tf_uncontract(px, py, pz)) tf_fuse<RGB>(vw, px, py, pz, tsdf, rgb);
  out_tsdf[p] = tsdf;
  if (RGB) out_rgb[3 * p] = rgb[0], out_rgb[3 * p + 1] = rgb[1], out_rgb[3 * p + 2] = rgb[2];
}

// The vertex step of the extraction: the inverse contraction, then the clip to +-max_range per component.  A point
// outside the contraction's image (the rule's factor is infinite or negative there) goes to infinity along its own
// direction before the clip: +-max_range in its non-zero components, 0 in the others.
__global__ void __launch_bounds__(TF_BLOCK)
tsdf_uncontract_kernel(const float* __restrict__ points, long long nr_points, float max_range,
                       float* __restrict__ out) {
  const long long p = (long long)blockIdx.x * TF_BLOCK + threadIdx.x;
  if (p >= nr_points) return;
  float q[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
  if (!tf_uncontract(q[0], q[1], q[2])) {
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = q[c] > 0.0f ? max_range : (q[c] < 0.0f ? -max_range : 0.0f);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * p + c] = fminf(fmaxf(q[c], -max_range), max_range);
}

bool tf_views_ok(const float* proj, const float* depth, int V, int H, int W, float trunc) {
  return proj && depth && V >= 1 && V <= (1 << 20) && H >= 1 && W >= 1 && H <= TF_MAX_SIDE && W <= TF_MAX_SIDE &&
         trunc > 0.0f && trunc < INFINITY;
}

}  // namespace

extern "C" int vsa_tsdf_fuse_lattice(const float* proj, const float* depth, int nr_views, int height, int width,
                                     const float* axis, int n, float sdf_trunc, int uncontract, float* out_tsdf,
                                     void* stream) {
  if (!tf_views_ok(proj, depth, nr_views, height, width, sdf_trunc) || !axis || !out_tsdf || n < 2 || n > TF_MAX_N)
    return VSA_ERR_ARG;
  const TfViews vw{proj, depth, nullptr, nr_views, height, width, sdf_trunc};
  const dim3 grid(vsa_div_up(n, TF_BRICK * TF_BRICKS_K), vsa_div_up(n, TF_BRICK), vsa_div_up(n, TF_BRICK));
  hipLaunchKernelGGL(tsdf_lattice_kernel, grid, dim3(TF_BLOCK), 0, (hipStream_t)stream, vw, axis, n,
                     uncontract ? 1 : 0, out_tsdf);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_tsdf_fuse_points(const float* proj, const float* depth, const float* rgb_maps, int nr_views,
                                    int height, int width, const float* points, long long nr_points, float sdf_trunc,
                                    int uncontract, float* out_tsdf, float* out_rgb, void* stream) {
  if (!tf_views_ok(proj, depth, nr_views, height, width, sdf_trunc) || nr_points < 0 ||
      nr_points > 0x7FFFFFFFll * TF_BLOCK || (out_rgb != nullptr) != (rgb_maps != nullptr))
    return VSA_ERR_ARG;
  if (nr_points == 0) return VSA_OK;
  if (!points || !out_tsdf) return VSA_ERR_ARG;
  const TfViews vw{proj, depth, rgb_maps, nr_views, height, width, sdf_trunc};
  const dim3 grid(vsa_div_up(nr_points, TF_BLOCK));
  if (out_rgb)
    hipLaunchKernelGGL(tsdf_points_kernel<true>, grid, dim3(TF_BLOCK), 0, (hipStream_t)stream, vw, points, nr_points,
                       uncontract ? 1 : 0, out_tsdf, out_rgb);
  else
    hipLaunchKernelGGL(tsdf_points_kernel<false>, grid, dim3(TF_BLOCK), 0, (hipStream_t)stream, vw, points,
                       nr_points, uncontract ? 1 : 0, out_tsdf, out_rgb);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_tsdf_uncontract_points(const float* points, long long nr_points, float max_range, float* out,
                                          void* stream) {
  if (nr_points < 0 || nr_points > 0x7FFFFFFFll * TF_BLOCK || !(max_range > 0.0f) || !(max_range < INFINITY))
    return VSA_ERR_ARG;
  if (nr_points == 0) return VSA_OK;
  if (!points || !out) return VSA_ERR_ARG;
  hipLaunchKernelGGL(tsdf_uncontract_kernel, dim3(vsa_div_up(nr_points, TF_BLOCK)), dim3(TF_BLOCK), 0,
                     (hipStream_t)stream, points, nr_points, max_range, out);
  VSA_RETURN_LAUNCH_STATUS();
}
