// The closest-hit walk of the quantised (q16) BVH nodes, shared by the translation units that trace: trace.hip (rays
// from memory, hit records to memory) and face_visibility.hip (rays made in registers, hits counted per face).  One text,
// so that both give the same closest hit bit for bit: smallest t, ties -> smallest original face id, hit iff t > t_min.
#pragma once
#include "common.h"

namespace {

constexpr int TRACE_BLOCK = 64;   // one wave per workgroup: a finished wave frees its stack at once
constexpr int TRACE_STACK = 48;

struct Roots {
  int root[VSA_MAX_SHELLS];
};

struct Hit {
  float t, u, v;
  int slot;  // index into the leaf-ordered triangle array, -1 = miss
  int id;    // original face id (tie break)
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

// Moeller-Trumbore, two-sided, fixed evaluation order (mirrored by the oracle).
__device__ __forceinline__ void tri_test(const float4 v0, const float4 e1, const float4 e2,
                                         float ox, float oy, float oz, float dx, float dy,
                                         float dz, float t_min, int slot, Hit& best) {
  float px = dy * e2.z - dz * e2.y;
  float py = dz * e2.x - dx * e2.z;
  float pz = dx * e2.y - dy * e2.x;
  float det = dot3(e1.x, e1.y, e1.z, px, py, pz);
  if (fabsf(det) < 1e-20f) return;
  float inv = 1.0f / det;
  float tx = ox - v0.x, ty = oy - v0.y, tz = oz - v0.z;
  float u = dot3(tx, ty, tz, px, py, pz) * inv;
  if (!(u >= 0.0f && u <= 1.0f)) return;
  float qx = ty * e1.z - tz * e1.y;
  float qy = tz * e1.x - tx * e1.z;
  float qz = tx * e1.y - ty * e1.x;
  float v = dot3(dx, dy, dz, qx, qy, qz) * inv;
  if (!(v >= 0.0f && u + v <= 1.0f)) return;
  float t = dot3(e2.x, e2.y, e2.z, qx, qy, qz) * inv;
  if (!(t > t_min)) return;
  int id = __float_as_int(v0.w);
  if (t < best.t || (t == best.t && id < best.id)) {
    best.t = t;
    best.u = u;
    best.v = v;
    best.slot = slot;
    best.id = id;
  }
}

// Traversal state per lane: an inner node index (>= 0), a leaf code (< 0:
// ~((first << 4) | count)), or TRACE_EMPTY.  "while-while": the wave first walks
// inner nodes until every lane holds a leaf (or is done), then all lanes test their
// leaf triangles together -- lanes no longer sit idle through other lanes' triangle
// loops at every node visit.
constexpr int TRACE_EMPTY = 0x7fffffff;

// ---- quantised nodes (vsa_bvh_export_q): 32 B per node instead of 64.  The inner-node walk
// is bound by the texture-address path (every lane fetches its own node: 64 lanes x 64 B per
// visit), so halving the node halves that traffic.  The ray is moved into each mesh's
// 16-bit grid once (o_g = (o - lo) / step + 1, d_g = d / step: the slab parameter t is
// unchanged), child boxes are tested directly on their u16 coordinates; the boxes were
// rounded outward by more than the fp32 error of that test, and triangles are still tested
// with the original ray, so the closest hit is bit-identical to the fp32-node kernel.
struct Frames {
  float f[VSA_MAX_SHELLS][6];   // lo.xyz, step.xyz
};

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// Slab test on grid coordinates, ~20 VALU ops per box (the fp32-node test is ~40 and PMC
// showed the traversal VALU-bound: 68 % VALU-busy at 37 % lane utilisation): per axis ONE
// packed FMA gives both plane parameters, t = q * (1/d_g) - o_g/d_g.  The different rounding
// (and the NaN an axis-parallel ray produces, which min/max then ignore, i.e. that axis's
// constraint is dropped) can only make the test pass more often; the boxes carry a one-unit
// outward margin, so nothing reachable is pruned.
struct QRay {
  f32x2_t ix, iy, iz;   // (1/d_g, 1/d_g) per axis
  f32x2_t cx, cy, cz;   // (-o_g/d_g, -o_g/d_g)
};

__device__ __forceinline__ bool qbox_test(unsigned w0, unsigned w1, unsigned w2, const QRay& r,
                                          float t_min, float t_max, float& t_near) {
  const f32x2_t qx = {(float)(w0 & 0xffffu), (float)(w1 >> 16)};
  const f32x2_t qy = {(float)(w0 >> 16), (float)(w2 & 0xffffu)};
  const f32x2_t qz = {(float)(w1 & 0xffffu), (float)(w2 >> 16)};
  const f32x2_t tx = __builtin_elementwise_fma(qx, r.ix, r.cx);
  const f32x2_t ty = __builtin_elementwise_fma(qy, r.iy, r.cy);
  const f32x2_t tz = __builtin_elementwise_fma(qz, r.iz, r.cz);
  const float tn = fmaxf(fmaxf(fminf(tx.x, tx.y), fminf(ty.x, ty.y)), fminf(tz.x, tz.y));
  const float tf = fminf(fminf(fmaxf(tx.x, tx.y), fmaxf(ty.x, ty.y)), fmaxf(tz.x, tz.y));
  t_near = tn;
  return tn <= tf && tf >= t_min && tn <= t_max;
}

// The walk of the quantised-node kernels.  BUDGETED: stop after `budget` wave-level trips (trace_qf_kernel
// measures its cost that way; the rejected budgeted three-pass form, the 4-wide nodes and the
// persistent-lane kernel of round 3 — all bit-exact, all slower: profiles/NOTEBOOK.md A9.4 — left the
// library in round 5 and live in the history at e64f229).
template <int STACK, bool BUDGETED, bool COUNT = false>
__device__ __forceinline__ int q_walk(const uint4* __restrict__ qnodes, const float4* __restrict__ tris,
                                       const QRay& qr, float ox, float oy, float oz, float dx, float dy,
                                       float dz, float t_min, int& cur, int& sp, Hit& best,
                                       int (*s_stack)[TRACE_BLOCK], int lane, int budget,
                                       int* lane_visits = nullptr, int* lane_tests = nullptr) {
  // The loops are written on ballots, i.e. as the wave-level loops they are, so that the trip count
  // is a scalar of the WAVE (a per-lane counter would only count that lane's own trips).
  int trips = 0;
  while (__builtin_amdgcn_ballot_w64(cur != TRACE_EMPTY) != 0) {
    if (BUDGETED && trips >= budget) break;
    while (__builtin_amdgcn_ballot_w64((unsigned)cur < (unsigned)TRACE_EMPTY) != 0) {
      ++trips;
      if (!((unsigned)cur < (unsigned)TRACE_EMPTY)) continue;
      if constexpr (COUNT) ++*lane_visits;
      const uint4 a = qnodes[2 * (long long)cur], b = qnodes[2 * (long long)cur + 1];
      float tn0, tn1;
      const bool h0 = qbox_test(a.x, a.y, a.z, qr, t_min, best.t, tn0);
      const bool h1 = qbox_test(a.w, b.x, b.y, qr, t_min, best.t, tn1);
      const int c0 = (int)b.z, c1 = (int)b.w;
      if (h0 && h1) {
        const bool swap = tn1 < tn0;
        s_stack[sp++][lane] = swap ? c0 : c1;
        cur = swap ? c1 : c0;
      } else if (h0) {
        cur = c0;
      } else if (h1) {
        cur = c1;
      } else {
        cur = sp ? s_stack[--sp][lane] : TRACE_EMPTY;
      }
    }
    if (cur != TRACE_EMPTY) {
      const int code = ~cur;
      const int first = code >> 4, cnt = code & 15;
      if constexpr (COUNT) *lane_tests += cnt;
      for (int i0 = 0; i0 < cnt; i0 += 4) {
        float4 tv[4][3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long long s = first + min(i0 + i, cnt - 1);
          tv[i][0] = tris[3 * s];
          tv[i][1] = tris[3 * s + 1];
          tv[i][2] = tris[3 * s + 2];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i0 + i < cnt)
            tri_test(tv[i][0], tv[i][1], tv[i][2], ox, oy, oz, dx, dy, dz, t_min, first + i0 + i, best);
      }
      cur = sp ? s_stack[--sp][lane] : TRACE_EMPTY;
    }
  }
  return trips;
}

}  // namespace
