// This library's pinhole definition (restated in oracle/raygen.py), shared by the translation units that make camera
// rays: raygen.hip (rays to memory) and face_visibility.hip (rays in registers).  One text and one operation order (the
// library is built without contraction), so that a ray of pixel point (x, y) has the same bits wherever it is made:
//   d_cam = Kinv (x, y, 1);  d = normalise(R d_cam);  o = t           (c2w = [R | t], 3x4)
#pragma once
#include "common.h"

namespace {

struct RayOut {
  float ox, oy, oz, dx, dy, dz;
};

__device__ __forceinline__ RayOut pinhole_ray(const float* __restrict__ c2w,
                                              const float* __restrict__ kinv, float x, float y) {
  float dc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) dc[i] = (kinv[3 * i] * x + kinv[3 * i + 1] * y) + kinv[3 * i + 2];
  float d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    d[i] = (c2w[4 * i] * dc[0] + c2w[4 * i + 1] * dc[1]) + c2w[4 * i + 2] * dc[2];
  const float n = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  return RayOut{c2w[3], c2w[7], c2w[11], d[0] / n, d[1] / n, d[2] / n};
}

}  // namespace
