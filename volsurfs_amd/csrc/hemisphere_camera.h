// Virtual cameras on a hemisphere around the origin (teacher distillation, trainer.py:132-166 of the reference:
// `sample_cameras_on_hemisphere`, which lives in mvdatasets, an empty submodule of the reference checkout — PARITY
// UNPINNED: the rule below is this library's own, restated in tests/distill_restated.py).  One function makes camera
// c's camera-to-world matrix in registers from a PCG32 stream, so that a ray kernel needs no pose table in memory.
// Only + - * / sqrtf in a fixed fp32 order (the library is built without contraction, as pinhole.h relies on): a numpy
// restatement gives the same bits, which sin / cos / acos of two libraries would not.
//
//   stream    camera c owns draws [c * CAM_STRIDE, (c + 1) * CAM_STRIDE) of the call's stream, CAM_STRIDE = 2 ATTEMPTS
//   candidate (a, b) = (2u - 1, 2v - 1) of two draws, s = a a + b b; the FIRST of up to ATTEMPTS candidates with
//             s < 1 and min_height <= |1 - 2s| <= max_height is taken
//   direction (2a sqrt(1 - s), 2b sqrt(1 - s), |1 - 2s|): Marsaglia's (1972) uniform sphere point folded onto the
//             upper half, so equal areas of the band get equal probability; divided by its length (1 to a few ulp)
//   fallback  every candidate refused: height (min_height + max_height) / 2, azimuth 0.  A candidate passes with
//             probability (pi / 4)(max_height - min_height): 0.746 at the defaults [0, 0.95], so 16 attempts fail
//             3e-10 of the cameras
//   frame     height axis = up_sign * e[up_axis]; the direction's first and second component go to the axes
//             (up_axis + 1) % 3 and (up_axis + 2) % 3
//   pose      centre = radius * direction; looks at the origin with the height axis as world up, in Camera's
//             convention (columns x right, y down, z forward): z = -direction, x = normalise(-up x z), y = z x x —
//             Camera.look_at(centre, up = height axis) to rounding.  max_height < 1 keeps z off the up axis.
#pragma once
#include "common.h"
#include "pcg32.h"

namespace {

constexpr int HEMI_ATTEMPTS = 16;
constexpr int HEMI_CAM_STRIDE = 2 * HEMI_ATTEMPTS;

struct HemiParams {
  float radius, min_height, max_height;
  int up_axis, up_sign, nr_cameras;
};

// 0 <= min_height <= max_height < 1, radius > 0 and finite (negated comparisons: a NaN is refused)
inline bool hemi_params_ok(const HemiParams& p) {
  if (p.up_axis < 0 || p.up_axis > 2 || (p.up_sign != 1 && p.up_sign != -1)) return false;
  if (!(p.radius > 0.0f) || !(p.radius < INFINITY)) return false;
  return p.min_height >= 0.0f && p.min_height <= p.max_height && p.max_height < 1.0f;
}

// c2w[12]: row-major 3x4, every index a compile-time constant after unrolling (the pose stays in registers)
__device__ __forceinline__ void hemisphere_camera(unsigned long long rng_state, unsigned long long rng_inc, int c,
                                                  const HemiParams& p, float* __restrict__ c2w) {
  Pcg32 rng{rng_state, rng_inc};
  rng.advance((unsigned long long)c * (unsigned long long)HEMI_CAM_STRIDE);
  const float hm = 0.5f * (p.min_height + p.max_height);
  float dx = sqrtf(1.0f - hm * hm), dy = 0.0f, dz = hm;          // the fallback
  for (int k = 0; k < HEMI_ATTEMPTS; ++k) {
    const float a = 2.0f * rng.next_float() - 1.0f;
    const float b = 2.0f * rng.next_float() - 1.0f;
    const float s = a * a + b * b;
    const float h = fabsf(1.0f - 2.0f * s);
    if (s < 1.0f && h >= p.min_height && h <= p.max_height) {
      const float t = sqrtf(1.0f - s);
      dx = (2.0f * a) * t, dy = (2.0f * b) * t, dz = h;
      break;
    }
  }
  const float n = sqrtf((dx * dx + dy * dy) + dz * dz);
  dx = dx / n, dy = dy / n, dz = dz / n;
  const float rho = sqrtf(dx * dx + dy * dy);
  const float sg = (float)p.up_sign;
  // components along (up axis, first, second) of the three columns and the centre
  const float zu = -(sg * dz), z1 = -dx, z2 = -dy;
  const float x1 = -(sg * dy) / rho, x2 = (sg * dx) / rho;
  const float col[4][3] = {{0.0f, x1, x2},
                           {z1 * x2 - z2 * x1, -(zu * x2), zu * x1},
                           {zu, z1, z2},
                           {p.radius * (sg * dz), p.radius * dx, p.radius * dy}};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int w = (r - p.up_axis + 3) % 3;      // which component lands in world row r
#pragma unroll
    for (int j = 0; j < 4; ++j) c2w[4 * r + j] = w == 0 ? col[j][0] : (w == 1 ? col[j][1] : col[j][2]);
  }
}

}  // namespace
