// The winding-number walk of the quantised (q16) BVH nodes, shared by the kernels of mesh_winding.hip: the point query,
// the signed query and the lattice field.  One text, so that all of them give the same w bit for bit.  The rule is this
// library's own (the reference has no such stage): include/volsurfs_hip.h "Mesh winding number", DESIGN §31.
//
// The nodes' boxes are not read: a subtree is judged by its entry of the moments table (vsa_mesh_winding_moments), one
// entry per child slot of every inner node (entry 2 n + c) and one per mesh root.  An entry is two float4: (N.xyz, r),
// (p.xyz, 0): N = sum 1/2 e1 x e2, p the area-weighted centroid, r a radius about p that holds every vertex.
#pragma once
#include "closest_walk.h"

namespace {

constexpr int WN_ENTRY_FLOATS = 8;
constexpr int WN_ROOT = 0x7ffffffe;           // the walk's first item: the mesh root and its own entry
constexpr float WN_INV_4PI = 0.07957747154594767f;

// The signed solid angle of the record (v0, e1, e2) seen from q (Van Oosterom & Strackee 1983), fp32, fixed order.
// atan2f(0, 0) = 0: a query on a vertex and a face without area contribute nothing.
__device__ __forceinline__ float solid_angle(const float4 v0, const float4 e1, const float4 e2, float qx, float qy,
                                             float qz) {
  const float ax = v0.x - qx, ay = v0.y - qy, az = v0.z - qz;
  const float bx = ax + e1.x, by = ay + e1.y, bz = az + e1.z;
  const float cx = ax + e2.x, cy = ay + e2.y, cz = az + e2.z;
  const float rx = by * cz - bz * cy, ry = bz * cx - bx * cz, rz = bx * cy - by * cx;
  const float num = dot3(ax, ay, az, rx, ry, rz);
  const float la = sqrtf(dot3(ax, ay, az, ax, ay, az));
  const float lb = sqrtf(dot3(bx, by, bz, bx, by, bz));
  const float lc = sqrtf(dot3(cx, cy, cz, cx, cy, cz));
  const float den = (((la * lb) * lc + dot3(ax, ay, az, bx, by, bz) * lc) + dot3(bx, by, bz, cx, cy, cz) * la) +
                    dot3(cx, cy, cz, ax, ay, az) * lb;
  return 2.0f * atan2f(num, den);
}

// w of one query: a depth-first walk, child 0 before child 1, one query per lane.  An item is an entry index; its child
// word (an inner node, a leaf code or none) is read from the node that owns the slot.  With d = p - q, L = |d|: a
// subtree with L > beta r (strict) and (d . d) L > 0 (a query within 1e-13 of a point-sized subtree would divide 0 by
// an underflowed 0) adds d . N / L^3 and is not opened; an inner node that is opened pushes its child 1
// and goes on with its child 0; a leaf that is opened has its triangles summed in slot order.  The wave-level loops are
// closest_walk's (inner items until every lane holds a leaf or is done, then the leaves together); a lane that holds a
// leaf waits with it, so that its sum is formed in its own depth-first order whatever the other lanes do.
// beta = inf: inf r is inf or NaN, nothing is far, every leaf is summed.  A NaN query: nothing is far, w is NaN.
// COUNT: entries judged and exact triangle terms of the lane.
template <int STACK, bool COUNT = false>
__device__ __forceinline__ float winding_walk(const uint4* __restrict__ qnodes, const float4* __restrict__ tris,
                                              const float4* __restrict__ moments, int root, long long root_entry,
                                              float qx, float qy, float qz, float beta, int (*s_node)[TRACE_BLOCK],
                                              int lane, int* lane_visits = nullptr, int* lane_terms = nullptr) {
  const uint32_t* words = reinterpret_cast<const uint32_t*>(qnodes);
  float acc = 0.0f;
  int sp = 0;
  int cur = root == TRACE_EMPTY ? -1 : WN_ROOT;
  int leaf = 0;                                   // a leaf code (negative) waiting for the second loop
  auto pop = [&]() { return sp ? s_node[--sp][lane] : -1; };
  while (__builtin_amdgcn_ballot_w64(cur >= 0 || leaf < 0) != 0) {
    while (__builtin_amdgcn_ballot_w64(cur >= 0) != 0) {
      if (cur < 0) continue;
      const bool first = cur == WN_ROOT;
      const long long e = first ? root_entry : (long long)cur;
      const int word = first ? root : (int)words[8 * (long long)(cur >> 1) + 6 + (cur & 1)];
      if (word == TRACE_EMPTY) {
        cur = pop();
        continue;
      }
      if constexpr (COUNT) ++*lane_visits;
      const float4 m0 = moments[2 * e], m1 = moments[2 * e + 1];
      const float dx = m1.x - qx, dy = m1.y - qy, dz = m1.z - qz;
      const float L2 = dot3(dx, dy, dz, dx, dy, dz);
      const float L = sqrtf(L2);
      const float L3 = L2 * L;
      if (L > beta * m0.w && L3 > 0.0f) {
        acc += dot3(dx, dy, dz, m0.x, m0.y, m0.z) / L3;
        cur = pop();
      } else if (word < 0) {
        leaf = word;
        cur = -1;
      } else {
        // (one push per level: the entry points refuse a tree as deep as the stack, so the guard only keeps a
        // malformed tree from writing past the LDS array)
        if (sp < STACK) s_node[sp++][lane] = 2 * word + 1;
        cur = 2 * word;
      }
    }
    if (leaf < 0) {
      const int code = ~leaf;
      const int begin = code >> 4, cnt = code & 15;
      if constexpr (COUNT) *lane_terms += cnt;
      for (int i = 0; i < cnt; ++i) {
        const long long s = begin + i;
        acc += solid_angle(tris[3 * s], tris[3 * s + 1], tris[3 * s + 2], qx, qy, qz);
      }
      leaf = 0;
      cur = pop();
    }
  }
  return acc * WN_INV_4PI;
}

// The closest-point walk's distance, negative iff w > 1/2.  No closest record (a NaN query): +inf (w is NaN there).
__device__ __forceinline__ float signed_by_winding(const Closest& best, float wn) {
  const float d = sqrtf(best.d2);
  return wn > 0.5f ? -d : d;
}

}  // namespace
