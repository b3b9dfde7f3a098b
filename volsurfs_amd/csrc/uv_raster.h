// The atlas raster rule, stated once: which texel centres of an R x R atlas a uv triangle covers (include/volsurfs_hip.h
// "UV atlas", raster).  vsa_atlas_rasterize (atlas.hip) rasterizes by it and the texture transfer's owner map
// (texture_transfer.hip) puts the faces that cover a texel first by it: the two agree because this is one text.
//
//   * every corner is clamped to [0, 1] in fp32 and snapped in fp64 to 1 / UV_SNAP of a texel: rint(uv * UV_SNAP * R);
//   * a face whose snapped signed area is <= 0 (back-facing or degenerate after the snap) covers nothing;
//   * texel (i, j) has its centre at (i + 1/2, j + 1/2) texels; a face covers it when the int64 edge functions of its
//     three edges are all > 0 there, or = 0 on a top or a left edge (the top-left rule: a centre on the edge shared by
//     two faces belongs to exactly one of them).
// tests/uv_raster_restated.py restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>

constexpr long long UV_SNAP = 256;

struct UvTri {
  long long x[3], y[3];   // the snapped corners
  bool front;             // the snapped signed area is > 0
};

struct UvBox {
  int i0, i1, j0, j1;     // texels (inclusive); empty when i0 > i1 or j0 > j1
};

// Twice the signed area of the snapped triangle.
__device__ __forceinline__ long long uv_area2(const UvTri& t) {
  return (t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
}

__device__ __forceinline__ UvTri uv_snap(const float* __restrict__ uv6, int R) {
  UvTri t;
  const double q = (double)UV_SNAP * (double)R;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float u = fminf(fmaxf(uv6[2 * k], 0.f), 1.f), v = fminf(fmaxf(uv6[2 * k + 1], 0.f), 1.f);
    t.x[k] = (long long)rint((double)u * q);
    t.y[k] = (long long)rint((double)v * q);
  }
  t.front = uv_area2(t) > 0;
  return t;
}

// Is p on the inner side of the edge a -> b, or on it when it is a top or a left edge?
__device__ __forceinline__ bool uv_edge_in(long long ax, long long ay, long long bx, long long by, long long px,
                                           long long py) {
  const long long dx = bx - ax, dy = by - ay;
  const long long e = dx * (py - ay) - dy * (px - ax);
  return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx < 0)));
}

__device__ __forceinline__ long long uv_centre(int i) { return i * UV_SNAP + UV_SNAP / 2; }

// The three edge tests of the snapped point p alone: coverage for a caller that walks uv_box, which is empty unless
// the face is front.
__device__ __forceinline__ bool uv_edges_in(const UvTri& t, long long px, long long py) {
  return uv_edge_in(t.x[0], t.y[0], t.x[1], t.y[1], px, py) && uv_edge_in(t.x[1], t.y[1], t.x[2], t.y[2], px, py) &&
         uv_edge_in(t.x[2], t.y[2], t.x[0], t.y[0], px, py);
}

__device__ __forceinline__ bool uv_covers(const UvTri& t, int i, int j) {
  const long long px = uv_centre(i), py = uv_centre(j);
  return t.front && uv_edge_in(t.x[0], t.y[0], t.x[1], t.y[1], px, py) &&
         uv_edge_in(t.x[1], t.y[1], t.x[2], t.y[2], px, py) && uv_edge_in(t.x[2], t.y[2], t.x[0], t.y[0], px, py);
}

__device__ __forceinline__ long long uv_floordiv(long long a, long long b) {
  return a >= 0 ? a / b : -((-a + b - 1) / b);
}

// The texels whose centres lie within the snapped corners' bounds, cut to the atlas: every texel the face can cover.
// Empty for a face that is not front.
__device__ __forceinline__ UvBox uv_box(const UvTri& t, int R) {
  const long long a2 = uv_area2(t);
  const long long xl = min(t.x[0], min(t.x[1], t.x[2])), xh = max(t.x[0], max(t.x[1], t.x[2]));
  const long long yl = min(t.y[0], min(t.y[1], t.y[2])), yh = max(t.y[0], max(t.y[1], t.y[2]));
  const long long h = UV_SNAP / 2;
  long long i0 = -uv_floordiv(-(xl - h), UV_SNAP), i1 = uv_floordiv(xh - h, UV_SNAP);
  long long j0 = -uv_floordiv(-(yl - h), UV_SNAP), j1 = uv_floordiv(yh - h, UV_SNAP);
  i0 = i0 < 0 ? 0 : i0;
  j0 = j0 < 0 ? 0 : j0;
  i1 = i1 > R - 1 ? R - 1 : i1;
  j1 = j1 > R - 1 ? R - 1 : j1;
  if (a2 <= 0) i1 = i0 - 1;
  UvBox b;
  b.i0 = (int)i0;
  b.i1 = (int)i1;
  b.j0 = (int)j0;
  b.j1 = (int)j1;
  return b;
}
