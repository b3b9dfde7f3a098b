// What the walkers of the quantised (q16) BVH nodes share, one text each, so that they agree bit for bit.
// Device: the ray in a mesh's 16-bit grid (make_qray), the empty hit (no_hit), the triangle and box tests, the leaf
// test with its loads up front (leaf_test), the closest-hit walk (q_walk: smallest t, ties -> smallest original face
// id, hit iff t > t_min) and the hit record's stores (write_hit): trace.hip (rays from memory, hit records to memory;
// its fp32-node kernel shares the hit, the leaf test and the stores) and face_visibility.hip (rays made in registers,
// hits counted per face).  closest_walk.h (mesh_distance.hip) walks the same nodes for the closest point.
// Host: the kernels' Roots / Frames arguments from the C ABI's arrays (make_qtree), the check of those arguments
// (check_qtree) and the choice of the stack size (with_stack), for the entry points of all three translation units.
#pragma once
#include "common.h"
#include <type_traits>

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

// "No hit yet": every triangle with t > t_min beats it.
__device__ __forceinline__ Hit no_hit() {
  Hit h;
  h.t = INFINITY;
  h.u = h.v = 0.f;
  h.slot = -1;
  h.id = 0x7fffffff;
  return h;
}

// The four stores of a hit record (t = 0 for a miss).
__device__ __forceinline__ void write_hit(const Hit& best, long long o, float* __restrict__ hit_t,
                                          int* __restrict__ hit_slot, float* __restrict__ hit_uv) {
  hit_t[o] = best.slot >= 0 ? best.t : 0.0f;
  hit_slot[o] = best.slot;
  hit_uv[2 * o] = best.u;
  hit_uv[2 * o + 1] = best.v;
}

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

// The triangles of the leaf `leaf` (a leaf code) against the ray, four at a time with the loads of the four issued
// before the first test.  Returns their number.
__device__ __forceinline__ int leaf_test(const float4* __restrict__ tris, int leaf, float ox, float oy, float oz,
                                         float dx, float dy, float dz, float t_min, Hit& best) {
  const int code = ~leaf;
  const int first = code >> 4, cnt = code & 15;
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
  return cnt;
}

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

// The ray in the 16-bit grid of the mesh whose frame (lo.xyz, step.xyz) is `fr`.  The divisions stay as written: the
// closest-point walk moves its query by the same (p - lo) / step + 1 (closest_qpoint).
__device__ __forceinline__ QRay make_qray(const float* fr, float ox, float oy, float oz, float dx, float dy,
                                          float dz) {
  const float gx = (ox - fr[0]) / fr[3] + 1.0f, gy = (oy - fr[1]) / fr[4] + 1.0f,
              gz = (oz - fr[2]) / fr[5] + 1.0f;
  const float ix = 1.0f / (dx / fr[3]), iy = 1.0f / (dy / fr[4]), iz = 1.0f / (dz / fr[5]);
  QRay qr;
  qr.ix = f32x2_t{ix, ix}, qr.iy = f32x2_t{iy, iy}, qr.iz = f32x2_t{iz, iz};
  qr.cx = f32x2_t{-(gx * ix), -(gx * ix)};
  qr.cy = f32x2_t{-(gy * iy), -(gy * iy)};
  qr.cz = f32x2_t{-(gz * iz), -(gz * iz)};
  return qr;
}

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
// library in round 5 and live in the history at e64f229).  COUNT: what the walk did, into *counts.
struct WalkCounts {
  int visits, tests;   // of this lane: inner nodes fetched, triangles tested
};

template <int STACK, bool BUDGETED, bool COUNT = false>
__device__ __forceinline__ int q_walk(const uint4* __restrict__ qnodes, const float4* __restrict__ tris,
                                       const QRay& qr, float ox, float oy, float oz, float dx, float dy,
                                       float dz, float t_min, int& cur, int& sp, Hit& best,
                                       int (*s_stack)[TRACE_BLOCK], int lane, int budget,
                                       WalkCounts* counts = nullptr) {
  // The loops are written on ballots, i.e. as the wave-level loops they are, so that the trip count
  // is a scalar of the WAVE (a per-lane counter would only count that lane's own trips).
  int trips = 0;
  while (__builtin_amdgcn_ballot_w64(cur != TRACE_EMPTY) != 0) {
    if (BUDGETED && trips >= budget) break;
    while (__builtin_amdgcn_ballot_w64((unsigned)cur < (unsigned)TRACE_EMPTY) != 0) {
      ++trips;
      if (!((unsigned)cur < (unsigned)TRACE_EMPTY)) continue;
      if constexpr (COUNT) ++counts->visits;
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
      const int cnt = leaf_test(tris, cur, ox, oy, oz, dx, dy, dz, t_min, best);
      if constexpr (COUNT) counts->tests += cnt;
      cur = sp ? s_stack[--sp][lane] : TRACE_EMPTY;
    }
  }
  return trips;
}

// ---- host: the tree arguments of the C ABI's entry points -> the kernels' arguments

// What a walking kernel takes: the node and triangle arrays, the shells' roots and quantisation frames by value.
struct QTree {
  const uint4* qnodes;
  const float4* tris;
  Roots roots;
  Frames frames;
};

inline Roots make_roots(const int32_t* mesh_roots, int nr_meshes) {
  Roots r;
  for (int i = 0; i < VSA_MAX_SHELLS; ++i) r.root[i] = i < nr_meshes ? mesh_roots[i] : 0;
  return r;
}

// (one shell: nr_meshes = 1 with pointers to its root and to the six floats of its frame)
inline QTree make_qtree(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots, const float* mesh_frames,
                        int nr_meshes) {
  QTree t;
  t.qnodes = reinterpret_cast<const uint4*>(qnodes);
  t.tris = reinterpret_cast<const float4*>(tris);
  t.roots = make_roots(mesh_roots, nr_meshes);
  for (int i = 0; i < VSA_MAX_SHELLS; ++i)
    for (int j = 0; j < 6; ++j) t.frames.f[i][j] = i < nr_meshes ? mesh_frames[6 * i + j] : 1.0f;
  return t;
}

// The status of the tree arguments.  `too_deep`: what this entry point documents for a tree deeper than the stack
// (include/volsurfs_hip.h: VSA_ERR_UNSUPPORTED from the vsa_trace* family, VSA_ERR_ARG elsewhere).  `arrays`: false
// leaves qnodes / tris unchecked (the vsa_trace* family accepts an empty launch before it looks at them).
inline int check_qtree(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots, const float* mesh_frames,
                       int nr_meshes, int max_depth, int too_deep, bool arrays = true) {
  if (!mesh_roots || !mesh_frames || nr_meshes < 1 || nr_meshes > VSA_MAX_SHELLS) return VSA_ERR_ARG;
  if (max_depth >= TRACE_STACK) return too_deep;
  if (arrays && (!qnodes || !tris)) return VSA_ERR_ARG;
  return VSA_OK;
}

// One of two template arguments by a run-time condition: f(std::integral_constant<T, A>) or <T, B>; the callable
// reads it as decltype(arg)::value.
template <auto A, auto B, class F>
inline void with_choice(bool first, F&& f) {
  if (first) f(std::integral_constant<decltype(A), A>{});
  else f(std::integral_constant<decltype(B), B>{});
}
template <class F>
inline void with_flag(bool on, F&& f) { with_choice<true, false>(on, f); }
// The traversal stack never exceeds the tree depth: shallow trees (the usual case: depth 16 for 82k-triangle shells)
// take a 24-entry stack.
template <class F>
inline void with_stack(int max_depth, F&& f) { with_choice<24, TRACE_STACK>(max_depth < 24, f); }

}  // namespace
