// The closest-point walk of the quantised (q16) BVH nodes, and the surface sampler, shared by the kernels of
// mesh_distance.hip: the unfused entry points (points from memory, records to memory) and the fused launch (samples made
// in registers, statistics reduced in the wave).  One text, so that all of them give the same closest point and the
// same sample bit for bit.  The nodes, their grid, the stack's shape and the host side of the tree arguments are the
// ray walk's (trace_walk.h).  The rule is this library's own (the reference has no such stage): include/volsurfs_hip.h
// "Mesh distance"; tests/mesh_distance_restated.py restates it in numpy, operation for operation.
#pragma once
#include "trace_walk.h"
// (pcg32.h uses the HIP runtime's intrinsics: after common.h)
#include "pcg32.h"

// Does a stack entry of the walk carry its bound at this tree depth?  The process-wide choice of
// vsa_closest_walk_config (csrc/mesh_distance.hip), for every unit that launches the walk.
bool closest_walk_bounds(int max_depth);

namespace {

struct Closest {
  float d2, u, v;   // squared distance; weights of v1 and v2
  int slot;         // index into the leaf-ordered triangle array, -1 = none (a NaN query)
  int id;           // original face id (tie break)
  int region;       // the region of the record that holds the closest point (CR_*)
};

// The region closest_on_triangle chose: the vertices v0 / v1 / v2, the edges v0 v1 / v0 v2 / v1 v2, the interior.  (The
// sliver whose three areas all rounded away ends at v0: CR_A.)  Only the signed distance reads it (csrc/mesh_sdf.hip).
enum { CR_A = 0, CR_B = 1, CR_C = 2, CR_AB = 3, CR_AC = 4, CR_BC = 5, CR_IN = 6, CR_REGIONS = 7 };

// "None yet": every triangle with a d2 that is not NaN beats it.
__device__ __forceinline__ Closest no_closest() {
  Closest c;
  c.d2 = INFINITY;
  c.u = c.v = 0.f;
  c.slot = -1;
  c.id = 0x7fffffff;
  c.region = CR_A;
  return c;
}

// Closest point of the triangle record (v0, e1, e2) to p: Ericson's seven regions (Real-Time Collision Detection
// 5.1.5) on the record's edges, fp32, fixed order.  Every quantity is computed for every region and the regions are
// chosen afterwards in Ericson's order of tests (A, B, AB, C, AC, BC, interior), so that a vectorised restatement
// takes the same values.  An edge region also asks for a positive denominator: a record with a zero edge falls through
// to the next region instead of dividing 0 by 0, and e1 = e2 = 0 ends in region A (u = v = 0: the point v0).
__device__ __forceinline__ void closest_on_triangle(const float4 v0, const float4 e1, const float4 e2, float px,
                                                    float py, float pz, float& d2_out, float& u_out, float& v_out,
                                                    int& region_out) {
  const float ax = px - v0.x, ay = py - v0.y, az = pz - v0.z;
  const float d1 = dot3(e1.x, e1.y, e1.z, ax, ay, az);
  const float d2 = dot3(e2.x, e2.y, e2.z, ax, ay, az);
  const float bx = ax - e1.x, by = ay - e1.y, bz = az - e1.z;
  const float d3 = dot3(e1.x, e1.y, e1.z, bx, by, bz);
  const float d4 = dot3(e2.x, e2.y, e2.z, bx, by, bz);
  const float cx = ax - e2.x, cy = ay - e2.y, cz = az - e2.z;
  const float d5 = dot3(e1.x, e1.y, e1.z, cx, cy, cz);
  const float d6 = dot3(e2.x, e2.y, e2.z, cx, cy, cz);
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  const float den_ab = d1 - d3, den_ac = d2 - d6;
  const float t43 = d4 - d3, t56 = d5 - d6;
  const float den_bc = t43 + t56;
  const float sum = (va + vb) + vc;
  float u, v;
  int region = CR_A;
  if (d1 <= 0.0f && d2 <= 0.0f) {                                    // A
    u = 0.0f, v = 0.0f;
  } else if (d3 >= 0.0f && d4 <= d3) {                               // B
    u = 1.0f, v = 0.0f, region = CR_B;
  } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f && den_ab > 0.0f) {   // AB
    u = d1 / den_ab, v = 0.0f, region = CR_AB;
  } else if (d6 >= 0.0f && d5 <= d6) {                               // C
    u = 0.0f, v = 1.0f, region = CR_C;
  } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f && den_ac > 0.0f) {   // AC
    u = 0.0f, v = d2 / den_ac, region = CR_AC;
  } else if (va <= 0.0f && t43 >= 0.0f && t56 >= 0.0f && den_bc > 0.0f) { // BC
    v = t43 / den_bc;
    u = 1.0f - v;
    region = CR_BC;
  } else if (sum > 0.0f) {                                           // interior
    const float inv = 1.0f / sum;
    u = vb * inv, v = vc * inv, region = CR_IN;
  } else {                                                           // (a sliver whose three areas all rounded away)
    u = 0.0f, v = 0.0f;
  }
  const float rx = (ax - u * e1.x) - v * e2.x;
  const float ry = (ay - u * e1.y) - v * e2.y;
  const float rz = (az - u * e1.z) - v * e2.z;
  d2_out = dot3(rx, ry, rz, rx, ry, rz);
  u_out = u;
  v_out = v;
  region_out = region;
}

// The minimum over (d2, original face id): tri_test's tie rule.  A NaN d2 never wins.
__device__ __forceinline__ void closest_tri(const float4 v0, const float4 e1, const float4 e2, float px, float py,
                                            float pz, int slot, Closest& best) {
  float d2, u, v;
  int region;
  closest_on_triangle(v0, e1, e2, px, py, pz, d2, u, v, region);
  const int id = __float_as_int(v0.w);
  if (d2 < best.d2 || (d2 == best.d2 && id < best.id)) {
    best.d2 = d2;
    best.u = u;
    best.v = v;
    best.slot = slot;
    best.id = id;
    best.region = region;
  }
}

// The query in a mesh's 16-bit grid (g = (p - lo) / step + 1, as the ray walk moves its origin) and the grid's step.
struct QPoint {
  float gx, gy, gz, sx, sy, sz;
};

__device__ __forceinline__ QPoint closest_qpoint(const float* fr, float px, float py, float pz) {
  QPoint q;
  q.gx = (px - fr[0]) / fr[3] + 1.0f;
  q.gy = (py - fr[1]) / fr[4] + 1.0f;
  q.gz = (pz - fr[2]) / fr[5] + 1.0f;
  q.sx = fr[3], q.sy = fr[4], q.sz = fr[5];
  return q;
}

// A lower bound, in fp32, of the fp32 squared distance closest_on_triangle gives for any triangle inside the child box
// (w0, w1, w2).  Per axis the gap between the query and the u16 box in grid units, times that axis's step; the squares
// summed; the sum scaled down by 1 - 2^-18.  Two allowances keep it below the true value (DESIGN §27 has the
// arithmetic): the boxes' one-unit outward margin covers the absolute errors (the query's grid coordinate and the
// residual p - closest point, both a few 2^-24 of the distance to the frame's corner plus the extent: below a
// fiftieth of a unit within an extent of the mesh, a unit at ~60 extents), the scale covers the relative ones (the
// products and sums here and in the triangle's own d2, and the same absolute errors once the gap is many units).
constexpr float CLOSEST_SLACK = 1.0f - 1.0f / 262144.0f;

__device__ __forceinline__ float qbox_dist2(unsigned w0, unsigned w1, unsigned w2, const QPoint& q) {
  const float lox = (float)(w0 & 0xffffu), loy = (float)(w0 >> 16), loz = (float)(w1 & 0xffffu);
  const float hix = (float)(w1 >> 16), hiy = (float)(w2 & 0xffffu), hiz = (float)(w2 >> 16);
  const float dx = fmaxf(fmaxf(lox - q.gx, q.gx - hix), 0.0f) * q.sx;
  const float dy = fmaxf(fmaxf(loy - q.gy, q.gy - hiy), 0.0f) * q.sy;
  const float dz = fmaxf(fmaxf(loz - q.gz, q.gz - hiz), 0.0f) * q.sz;
  return ((dx * dx + dy * dy) + dz * dz) * CLOSEST_SLACK;
}

// The walk, in q_walk's form: wave-level loops on ballots, inner nodes until every lane holds a leaf, then the leaves
// together.  A child is dropped when its bound exceeds the best d2 so far (an equal bound is walked: a triangle at the
// same distance with a smaller id wins), the nearer child is entered first and the farther one pushed.  BOUNDS: it is
// pushed with its bound (a second LDS word per entry); by the time it is popped the best d2 has usually shrunk below
// it, and the entry is dropped without fetching the node.  Without, the popped node is fetched and its children
// tested (the form for the 48-entry stack, where the second word costs half the occupancy: DESIGN §27).  `cur` is
// the root.  COUNT: node visits and triangle tests of the lane.
template <int STACK, bool BOUNDS, bool COUNT = false>
__device__ __forceinline__ void closest_walk(const uint4* __restrict__ qnodes, const float4* __restrict__ tris,
                                             const QPoint& q, float px, float py, float pz, int cur, Closest& best,
                                             int (*s_node)[TRACE_BLOCK], float (*s_bound)[TRACE_BLOCK], int lane,
                                             int* lane_visits = nullptr, int* lane_tests = nullptr) {
  int sp = 0;
  auto pop = [&]() {
    int next = TRACE_EMPTY;
    while (sp) {
      --sp;
      if (!BOUNDS || s_bound[sp][lane] <= best.d2) {
        next = s_node[sp][lane];
        break;
      }
    }
    return next;
  };
  while (__builtin_amdgcn_ballot_w64(cur != TRACE_EMPTY) != 0) {
    while (__builtin_amdgcn_ballot_w64((unsigned)cur < (unsigned)TRACE_EMPTY) != 0) {
      if (!((unsigned)cur < (unsigned)TRACE_EMPTY)) continue;
      if constexpr (COUNT) ++*lane_visits;
      const uint4 a = qnodes[2 * (long long)cur], b = qnodes[2 * (long long)cur + 1];
      const int c0 = (int)b.z, c1 = (int)b.w;
      const float b0 = qbox_dist2(a.x, a.y, a.z, q), b1 = qbox_dist2(a.w, b.x, b.y, q);
      const bool h0 = c0 != TRACE_EMPTY && b0 <= best.d2;
      const bool h1 = c1 != TRACE_EMPTY && b1 <= best.d2;
      if (h0 && h1) {
        const bool swap = b1 < b0;
        s_node[sp][lane] = swap ? c0 : c1;
        if constexpr (BOUNDS) s_bound[sp][lane] = swap ? b0 : b1;
        ++sp;
        cur = swap ? c1 : c0;
      } else if (h0) {
        cur = c0;
      } else if (h1) {
        cur = c1;
      } else {
        cur = pop();
      }
    }
    if (cur != TRACE_EMPTY) {
      const int code = ~cur;
      const int first = code >> 4, cnt = code & 15;
      if constexpr (COUNT) *lane_tests += cnt;
      for (int i = 0; i < cnt; ++i) {
        const long long s = first + i;
        closest_tri(tris[3 * s], tris[3 * s + 1], tris[3 * s + 2], px, py, pz, first + i, best);
      }
      cur = pop();
    }
  }
}

// ---- the sign by the pseudonormal (csrc/mesh_sdf.hip; csrc/shell_untangle.hip moves vertices along the same r and N)

constexpr int PN_FLOATS = 3 * CR_REGIONS;     // a face's row of the pseudonormal table [F, 7, 3]

// The residual r = p - closest point of a walk's result (best.slot >= 0), as closest_on_triangle forms it: from the
// same record and weights, the same bits.
__device__ __forceinline__ void closest_residual(const float4* __restrict__ tris, const Closest& best, float px,
                                                 float py, float pz, float& rx, float& ry, float& rz) {
  const long long s = best.slot;
  const float4 v0 = tris[3 * s], e1 = tris[3 * s + 1], e2 = tris[3 * s + 2];
  const float ax = px - v0.x, ay = py - v0.y, az = pz - v0.z;
  rx = (ax - best.u * e1.x) - best.v * e2.x;
  ry = (ay - best.u * e1.y) - best.v * e2.y;
  rz = (az - best.u * e1.z) - best.v * e2.z;
}

// The table's entry of the closest feature: (face, region) of a walk's result, `base` the mesh's first row.
__device__ __forceinline__ const float* closest_pseudonormal(const float* __restrict__ table, long long base,
                                                             const Closest& best) {
  return table + (base + best.id) * PN_FLOATS + 3 * best.region;
}

// The walk's distance with the sign of r . N: r the residual, N the table's entry of (face, region).  No closest
// record (a NaN query): +inf.
__device__ __forceinline__ float signed_distance(const float4* __restrict__ tris, const float* __restrict__ table,
                                                 long long base, const Closest& best, float px, float py, float pz) {
  const float d = sqrtf(best.d2);
  if (best.slot < 0) return d;
  float rx, ry, rz;
  closest_residual(tris, best, px, py, pz, rx, ry, rz);
  const float* n = closest_pseudonormal(table, base, best);
  return dot3(rx, ry, rz, n[0], n[1], n[2]) < 0.0f ? -d : d;
}

// ---- the surface sampler

// fp64 area of a record: 0.5 sqrt((nx nx + ny ny) + nz nz), n = e1 x e2, every operation in fp64 on the fp32 edges.
__device__ __forceinline__ double record_area(const float4 e1, const float4 e2) {
  const double nx = (double)e1.y * (double)e2.z - (double)e1.z * (double)e2.y;
  const double ny = (double)e1.z * (double)e2.x - (double)e1.x * (double)e2.z;
  const double nz = (double)e1.x * (double)e2.y - (double)e1.y * (double)e2.x;
  return 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
}

// The generator of sample i: a Pcg32 stream whose state is (seed, i) through the splitmix64 finaliser.
__device__ __forceinline__ Pcg32 sample_rng(unsigned long long seed, long long i) {
  unsigned long long h = seed + 0x9E3779B97F4A7C15ULL * ((unsigned long long)i + 1ull);
  h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ULL;
  h = (h ^ (h >> 27)) * 0x94D049BB133111EBULL;
  h ^= h >> 31;
  Pcg32 rng{h, 1442695040888963407ULL};
  rng.next_uint();
  return rng;
}

struct SurfaceSample {
  float x, y, z, u, v;
  int slot;        // global slot (first_slot + the index found)
};

// Sample i of n of the records [first_slot, first_slot + nr_slots) with the inclusive integer prefix of their weights:
// stratified position (i + xi) / n of the total in fp64, the slot by binary search (the first whose prefix exceeds the
// position: a weight-0 record is never found), (u, v) by two more draws folded into the triangle, the point in fp32.
__device__ __forceinline__ SurfaceSample surface_sample(const float4* __restrict__ tris, long long first_slot,
                                                        long long nr_slots, const long long* __restrict__ prefix,
                                                        long long i, long long n, unsigned long long seed) {
  Pcg32 rng = sample_rng(seed, i);
  const float xi = rng.next_float();
  float u = rng.next_float(), v = rng.next_float();
  const long long total = prefix[nr_slots - 1];
  const double pos = ((double)i + (double)xi) / (double)n * (double)total;
  long long target = (long long)pos;
  target = target < total - 1 ? target : total - 1;
  long long lo = 0, hi = nr_slots - 1;          // the answer lies in [lo, hi]: prefix[nr_slots - 1] = total > target
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (prefix[mid] > target) hi = mid;
    else lo = mid + 1;
  }
  if (u + v > 1.0f) {                           // (exact: u, v are multiples of 2^-23 below 1)
    u = 1.0f - u;
    v = 1.0f - v;
  }
  const long long s = first_slot + lo;
  const float4 v0 = tris[3 * s], e1 = tris[3 * s + 1], e2 = tris[3 * s + 2];
  SurfaceSample r;
  r.x = (v0.x + u * e1.x) + v * e2.x;
  r.y = (v0.y + u * e1.y) + v * e2.y;
  r.z = (v0.z + u * e1.z) + v * e2.z;
  r.u = u, r.v = v;
  r.slot = (int)s;
  return r;
}

}  // namespace
