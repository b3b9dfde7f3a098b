// Quadric edge-collapse simplification of one triangle mesh (vsa_simplify*; rules in include/volsurfs_hip.h,
// DESIGN §15).
//
// Rounds on one stream.  Each round:
//   edges:    the 3F (min, max) keys of the current faces, packed into s + s bits (s = bits of V - 1), radix-sorted;
//             head flags + an exclusive scan give every unique edge its id (its rank) and `ehead[id]`, the first
//             sorted slot of the edge, so its face count is ehead[id + 1] - ehead[id].  Vertex flags (boundary,
//             frozen) come from the counts by an atomic OR.  The (vertex, face) list is radix-sorted into a CSR
//             (vstart / vend over the sorted slots): the ring of faces of every vertex.
//   cost:     one lane per edge: placement, cost and the validity rules over the rings of both endpoints -> the
//             64-bit key (cost bits << 32 | edge id) or UINT64_MAX.
//   guard:    (vsa_simplify_guarded only) one lane per edge that is still a candidate: every face the collapse would
//             create, as triangle A, walks each guard mesh's q16 tree by box overlap (cross_walk.h) and meets the
//             faces of the leaves it reaches under the exact crossing rule; one crossing clears the edge's key.
//   select:   m1 (64-bit atomicMin over edges), m2 (64-bit atomicMin over faces), the winners' flags, a scan, the
//             winners' keys compacted in edge-id order, and {W, faces they remove} read by the host.  Only when the
//             winners would remove more than the faces still to remove are their keys sorted and a scan of their
//             face counts decides the accepted prefix.
//   collapse: one lane per accepted winner: b's ring rewritten to a (faces with both dropped), a moved, Q_a += Q_b.
//   compact:  surviving faces scanned and scattered in order into the other face buffer.
// Winners share no vertex and no face (see the header), so the lanes of one round never touch the same data.  Every
// float sum has a fixed order (no float atomics); integer atomics only form minima, ORs and counts.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cross_walk.h"
#include "mesh_topology.h"

#define SMP_BLOCK MT_BLOCK
#define SMP_BOUNDARY 1u
#define SMP_FROZEN 2u
#define SMP_DET_REL 1e-10
#define SMP_BOUNDARY_WEIGHT 10.0
#define SMP_NONE 0xFFFFFFFFFFFFFFFFull

// device counters
#define CTR_E 0
#define CTR_W 1
#define CTR_R 2
#define CTR_F 3
#define CTR_ACC 4
#define CTR_V 5
#define CTR_G 6          // (round, edge) verdicts the guard turned down; read with CTR_V
#define CTR_N 8

using mt::u64;

// ------------------------------------------------------------------------------------------------ fp64 geometry

// Plane quadric w * p p^T of p = (u, d), upper triangle in the order xx xy xz xd yy yz yd zz zd dd.
__device__ __forceinline__ void smp_plane(double w, double ux, double uy, double uz, double d, double* q) {
  const double p[4] = {ux, uy, uz, d};
  int k = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) q[k++] = w * (p[i] * p[j]);
}

__device__ __forceinline__ void smp_load(const float* P, int v, double* p) {
  p[0] = (double)P[3 * (long long)v];
  p[1] = (double)P[3 * (long long)v + 1];
  p[2] = (double)P[3 * (long long)v + 2];
}

// n = (p1 - p0) x (p2 - p0) in fp64.
__device__ __forceinline__ void smp_normal(const double* p0, const double* p1, const double* p2, double* n) {
  const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
  const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
  n[0] = e1y * e2z - e1z * e2y;
  n[1] = e1z * e2x - e1x * e2z;
  n[2] = e1x * e2y - e1y * e2x;
}

// Area-weighted plane quadric of a face: (|n| / 2) * (u, -u.p0)(u, -u.p0)^T with u = n / |n|; zero for |n| = 0.
__device__ void smp_face_quadric(const double* p0, const double* n, double* q) {
  const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  if (!(len > 0.0)) {
#pragma unroll
    for (int k = 0; k < 10; ++k) q[k] = 0.0;
    return;
  }
  const double ux = n[0] / len, uy = n[1] / len, uz = n[2] / len;
  const double d = -(ux * p0[0] + uy * p0[1] + uz * p0[2]);
  smp_plane(0.5 * len, ux, uy, uz, d, q);
}

// Boundary penalty of the edge pi -> pj of a face with normal n: the plane through the edge along n, weighted by
// SMP_BOUNDARY_WEIGHT * |pj - pi|^2; zero when (pj - pi) x n = 0.
__device__ void smp_boundary_quadric(const double* pi, const double* pj, const double* n, double* q) {
  const double ex = pj[0] - pi[0], ey = pj[1] - pi[1], ez = pj[2] - pi[2];
  const double mx = ey * n[2] - ez * n[1], my = ez * n[0] - ex * n[2], mz = ex * n[1] - ey * n[0];
  const double len = sqrt(mx * mx + my * my + mz * mz);
  if (!(len > 0.0)) {
#pragma unroll
    for (int k = 0; k < 10; ++k) q[k] = 0.0;
    return;
  }
  const double ux = mx / len, uy = my / len, uz = mz / len;
  const double d = -(ux * pi[0] + uy * pi[1] + uz * pi[2]);
  smp_plane(SMP_BOUNDARY_WEIGHT * (ex * ex + ey * ey + ez * ez), ux, uy, uz, d, q);
}

// (x, y, z, 1) Q (x, y, z, 1)^T at an fp32 position.
__device__ __forceinline__ double smp_eval(const double* q, const float* p) {
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  const double t0 = q[0] * x + q[1] * y + q[2] * z + q[3];
  const double t1 = q[1] * x + q[4] * y + q[5] * z + q[6];
  const double t2 = q[2] * x + q[5] * y + q[7] * z + q[8];
  const double t3 = q[3] * x + q[6] * y + q[8] * z + q[9];
  return t0 * x + t1 * y + t2 * z + t3;
}

// Placement of the vertex that replaces edge (a, b) and its cost (header rules).
__device__ void smp_place(const double* __restrict__ Q, const float* __restrict__ P, const unsigned* __restrict__ vflag,
                          int a, int b, float* p, double* cost) {
  double q[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) q[k] = Q[10 * (long long)a + k] + Q[10 * (long long)b + k];
  float pa[3], pb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    pa[c] = P[3 * (long long)a + c];
    pb[c] = P[3 * (long long)b + c];
  }
  const bool ba = vflag[a] & SMP_BOUNDARY, bb = vflag[b] & SMP_BOUNDARY;
  if (ba != bb) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = ba ? pa[c] : pb[c];
    *cost = smp_eval(q, p);
    return;
  }
  const double A = q[0], B = q[1], C = q[2], D = q[4], E = q[5], F = q[7];
  const double r0 = -q[3], r1 = -q[6], r2 = -q[8];
  const double c00 = D * F - E * E, c01 = C * E - B * F, c02 = B * E - C * D;
  const double c11 = A * F - C * C, c12 = B * C - A * E, c22 = A * D - B * B;
  const double det = A * c00 + B * c01 + C * c02;
  const double tr = A + D + F;
  if (det > SMP_DET_REL * (tr * tr * tr)) {
    p[0] = (float)((c00 * r0 + c01 * r1 + c02 * r2) / det);
    p[1] = (float)((c01 * r0 + c11 * r1 + c12 * r2) / det);
    p[2] = (float)((c02 * r0 + c12 * r1 + c22 * r2) / det);
    *cost = smp_eval(q, p);
    return;
  }
  float pm[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) pm[c] = (float)(((double)pa[c] + (double)pb[c]) * 0.5);
  const double ca = smp_eval(q, pa), cb = smp_eval(q, pb), cm = smp_eval(q, pm);
  double best = ca;
#pragma unroll
  for (int c = 0; c < 3; ++c) p[c] = pa[c];
  if (cb < best) {
    best = cb;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = pb[c];
  }
  if (cm < best) {
    best = cm;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = pm[c];
  }
  *cost = best;
}

// ------------------------------------------------------------------------------------------------ edges and rings

__global__ __launch_bounds__(SMP_BLOCK) void smp_heads(const u64* __restrict__ sorted, long long n3,
                                                      int32_t* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (i >= n3) return;
  flags[i] = i == 0 || sorted[i] != sorted[i - 1];
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_edge_index(const int32_t* __restrict__ flags,
                                                           const int32_t* __restrict__ rank, long long n3,
                                                           int32_t* __restrict__ ehead, long long* __restrict__ ctr) {
  const long long i = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (i >= n3) return;
  if (flags[i]) ehead[rank[i]] = (int32_t)i;
  if (i == n3 - 1) {
    const int E = rank[i] + flags[i];
    ehead[E] = (int32_t)n3;
    ctr[CTR_E] = E;
  }
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_vertex_flags(const u64* __restrict__ sorted,
                                                             const int32_t* __restrict__ ehead, long long n3, int s,
                                                             const long long* __restrict__ ctr,
                                                             unsigned* __restrict__ vflag) {
  const long long e = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (e >= ctr[CTR_E]) return;
  const int cnt = ehead[e + 1] - ehead[e];
  if (cnt == 2) return;
  const u64 k = sorted[ehead[e]];
  const int a = (int)(k >> s), b = (int)(k & ((1ull << s) - 1));
  const unsigned fl = cnt == 1 ? SMP_BOUNDARY : SMP_FROZEN;
  atomicOr(vflag + a, fl);
  atomicOr(vflag + b, fl);
}

// Init only: the face count of the edge at every face slot 3 f + c.
__global__ __launch_bounds__(SMP_BLOCK) void smp_slot_counts(const int32_t* __restrict__ flags,
                                                            const int32_t* __restrict__ rank,
                                                            const uint32_t* __restrict__ slot,
                                                            const int32_t* __restrict__ ehead, long long n3,
                                                            int32_t* __restrict__ slot_cnt) {
  const long long i = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (i >= n3) return;
  const int e = rank[i] + flags[i] - 1;
  slot_cnt[slot[i]] = ehead[e + 1] - ehead[e];
}

// Init: Q_v = sum over the faces at v in ascending face order of (face quadric, then the penalties of the face's
// boundary edges at v in corner order).
__global__ __launch_bounds__(SMP_BLOCK) void smp_quadrics(const float* __restrict__ P, const int32_t* __restrict__ faces,
                                                         const uint32_t* __restrict__ vff,
                                                         const int32_t* __restrict__ vstart,
                                                         const int32_t* __restrict__ vend,
                                                         const int32_t* __restrict__ slot_cnt, long long V,
                                                         double* __restrict__ Q) {
  const long long v = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (v >= V) return;
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;
  for (int j = vstart[v]; j < vend[v]; ++j) {
    const long long f = vff[j];
    int id[3];
    double p[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      id[c] = faces[3 * f + c];
      smp_load(P, id[c], p[c]);
    }
    double n[3], q[10];
    smp_normal(p[0], p[1], p[2], n);
    smp_face_quadric(p[0], n, q);
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] += q[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int c1 = c == 2 ? 0 : c + 1;
      if ((id[c] == v || id[c1] == v) && slot_cnt[3 * f + c] == 1) {
        smp_boundary_quadric(p[c], p[c1], n, q);
#pragma unroll
        for (int k = 0; k < 10; ++k) acc[k] += q[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) Q[10 * v + k] = acc[k];
}

// ------------------------------------------------------------------------------------------------ cost

__device__ __forceinline__ bool smp_has(const int32_t* __restrict__ faces, long long f, int x) {
  return faces[3 * f] == x || faces[3 * f + 1] == x || faces[3 * f + 2] == x;
}

__device__ __forceinline__ void smp_sort3(int* t) {
  int x;
  if (t[0] > t[1]) { x = t[0]; t[0] = t[1]; t[1] = x; }
  if (t[1] > t[2]) { x = t[1]; t[1] = t[2]; t[2] = x; }
  if (t[0] > t[1]) { x = t[0]; t[0] = t[1]; t[1] = x; }
}

// Faces of the ring of `m` (a or b) that survive the collapse: no flip allowed; returns false on a flip.
__device__ bool smp_no_flip(const float* __restrict__ P, const int32_t* __restrict__ faces,
                            const uint32_t* __restrict__ vff, int j0, int j1, int m, int other, const float* p) {
  for (int j = j0; j < j1; ++j) {
    const long long f = vff[j];
    int id[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) id[c] = faces[3 * f + c];
    if (id[0] == other || id[1] == other || id[2] == other) continue;
    double po[3][3], pn[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      smp_load(P, id[c], po[c]);
#pragma unroll
      for (int x = 0; x < 3; ++x) pn[c][x] = id[c] == m ? (double)p[x] : po[c][x];
    }
    double nb[3], na[3];
    smp_normal(po[0], po[1], po[2], nb);
    smp_normal(pn[0], pn[1], pn[2], na);
    if (nb[0] == 0.0 && nb[1] == 0.0 && nb[2] == 0.0) continue;
    if (!(nb[0] * na[0] + nb[1] * na[1] + nb[2] * na[2] > 0.0)) return false;
  }
  return true;
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_cost(const float* __restrict__ P, const double* __restrict__ Q,
                                                     const unsigned* __restrict__ vflag,
                                                     const int32_t* __restrict__ faces, const u64* __restrict__ sorted,
                                                     const int32_t* __restrict__ ehead,
                                                     const uint32_t* __restrict__ vff,
                                                     const int32_t* __restrict__ vstart,
                                                     const int32_t* __restrict__ vend, long long n3, int s,
                                                     const long long* __restrict__ ctr, u64* __restrict__ ekey) {
  const long long e = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (e >= ctr[CTR_E]) return;
  const int cnt = ehead[e + 1] - ehead[e];
  const u64 hk = sorted[ehead[e]];
  const int a = (int)(hk >> s), b = (int)(hk & ((1ull << s) - 1));
  const unsigned fa = vflag[a], fb = vflag[b];
  u64 key = SMP_NONE;
  // frozen endpoints; no pinching (an interior edge between two boundary vertices)
  if (((fa | fb) & SMP_FROZEN) || (cnt > 1 && (fa & fb & SMP_BOUNDARY))) {
    ekey[e] = key;
    return;
  }
  float p[3];
  double cost;
  smp_place(Q, P, vflag, a, b, p, &cost);
  bool ok = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && !isnan(cost);
  const int sa = vstart[a], ea = vend[a], sb = vstart[b], eb = vend[b];
  // link condition: distinct common neighbours == face count
  if (ok) {
    int common = 0;
    for (int j = sa; j < ea; ++j) {
      const long long f = vff[j];
      for (int c = 0; c < 3; ++c) {
        const int x = faces[3 * f + c];
        if (x == a || x == b) continue;
        bool seen = false;
        for (int j2 = sa; j2 < j && !seen; ++j2) seen = smp_has(faces, vff[j2], x);
        if (seen) continue;
        bool adj = false;
        for (int j3 = sb; j3 < eb && !adj; ++j3) adj = smp_has(faces, vff[j3], x);
        common += adj;
      }
    }
    ok = common == cnt;
  }
  // no flips around a or b
  if (ok) ok = smp_no_flip(P, faces, vff, sa, ea, a, b, p) && smp_no_flip(P, faces, vff, sb, eb, b, a, p);
  // no duplicated face: a surviving face at a against a surviving face at b (b -> a)
  if (ok) {
    for (int j = sa; j < ea && ok; ++j) {
      const long long f = vff[j];
      int t[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
      if (t[0] == b || t[1] == b || t[2] == b) continue;
      smp_sort3(t);
      for (int j2 = sb; j2 < eb; ++j2) {
        const long long g = vff[j2];
        int u[3] = {faces[3 * g], faces[3 * g + 1], faces[3 * g + 2]};
        if (u[0] == a || u[1] == a || u[2] == a) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = u[c] == b ? a : u[c];
        smp_sort3(u);
        if (t[0] == u[0] && t[1] == u[1] && t[2] == u[2]) {
          ok = false;
          break;
        }
      }
    }
  }
  if (ok) {
    const double c = cost < 0.0 ? 0.0 : cost;
    const float cf = (float)c;
    unsigned bits = __float_as_uint(cf);
    if ((double)cf < c) bits += 1u;          // rounded up
    key = (u64)bits << 32 | (u64)e;
  }
  ekey[e] = key;
}

// ------------------------------------------------------------------------------------------------ guard

// One lane per edge id, one wave per block.  A lane whose edge is still a candidate places the new vertex as
// smp_collapse will (recomputed: 2 x 80 bytes of Q, 2 x 12 of P and 2 x 4 of flags read per candidate, against a
// 12-byte store per edge in smp_cost, a 12-byte load here and 36 bytes per face of workspace for a position buffer --
// and smp_cost, which the unguarded entry shares, stays as it is), then takes the surviving faces of a's ring and of
// b's ring one at a time.  cross_walk loops on wave ballots, so the wave stays together: the loop over the faces runs
// to the wave's longest ring, and a lane with no face left, or with its verdict already in, walks from TRACE_EMPTY
// (cross_guards_hit of cross_walk.h, the loop over the guards that msm_guard shares).
template <int STACK>
__global__ __launch_bounds__(TRACE_BLOCK) void smp_guard(const float* __restrict__ P, const double* __restrict__ Q,
                                                        const unsigned* __restrict__ vflag,
                                                        const int32_t* __restrict__ faces,
                                                        const u64* __restrict__ sorted,
                                                        const int32_t* __restrict__ ehead,
                                                        const uint32_t* __restrict__ vff,
                                                        const int32_t* __restrict__ vstart,
                                                        const int32_t* __restrict__ vend, int s,
                                                        long long* __restrict__ ctr, u64* __restrict__ ekey,
                                                        CrossGuards G) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const long long e = (long long)blockIdx.x * TRACE_BLOCK + lane;
  const bool live = e < ctr[CTR_E] && ekey[e] != SMP_NONE;
  int a = 0, b = 0, ring = 2, j = 0;
  float p[3] = {0.f, 0.f, 0.f};
  if (live) {
    const u64 hk = sorted[ehead[e]];
    a = (int)(hk >> s), b = (int)(hk & ((1ull << s) - 1));
    double cost;
    smp_place(Q, P, vflag, a, b, p, &cost);
    ring = 0;
    j = vstart[a];
  }
  bool rejected = false;
  for (;;) {
    // the lane's next face at a without b, then at b without a
    int id[3] = {0, 0, 0}, m = 0;
    bool have = false;
    if (!rejected) {
      while (ring < 2) {
        if (j >= (ring == 0 ? vend[a] : vend[b])) {
          ++ring;
          j = vstart[b];
          continue;
        }
        const long long f = vff[j++];
        const int other = ring == 0 ? b : a;
#pragma unroll
        for (int c = 0; c < 3; ++c) id[c] = faces[3 * f + c];
        if (id[0] == other || id[1] == other || id[2] == other) continue;
        m = ring == 0 ? a : b;
        have = true;
        break;
      }
    }
    if (__builtin_amdgcn_ballot_w64(have) == 0) break;
    // the face in its corner order, the moved vertex at p
    CrossTri T;
    float x[3], y[3], z[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const bool moved = !have || id[c] == m;
      const long long v = moved ? 0 : id[c];
      x[c] = moved ? p[0] : P[3 * v];
      y[c] = moved ? p[1] : P[3 * v + 1];
      z[c] = moved ? p[2] : P[3 * v + 2];
      T.x[c] = (double)x[c], T.y[c] = (double)y[c], T.z[c] = (double)z[c];
    }
    cross_guards_hit<STACK>(G, T, x, y, z, have, rejected, s_node, lane);
  }
  if (rejected) ekey[e] = SMP_NONE;
  const unsigned long long turned_down = __builtin_amdgcn_ballot_w64(rejected);
  if (lane == 0 && turned_down)
    atomicAdd((unsigned long long*)(ctr + CTR_G), (unsigned long long)__popcll(turned_down));
}

// ------------------------------------------------------------------------------------------------ select

__global__ __launch_bounds__(SMP_BLOCK) void smp_m1(const u64* __restrict__ ekey, const u64* __restrict__ sorted,
                                                   const int32_t* __restrict__ ehead, int s,
                                                   const long long* __restrict__ ctr, u64* __restrict__ m1) {
  const long long e = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (e >= ctr[CTR_E]) return;
  const u64 key = ekey[e];
  if (key == SMP_NONE) return;
  const u64 hk = sorted[ehead[e]];
  atomicMin(m1 + (hk >> s), key);
  atomicMin(m1 + (hk & ((1ull << s) - 1)), key);
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_m2(const int32_t* __restrict__ faces, long long F,
                                                   const u64* __restrict__ m1, u64* __restrict__ m2) {
  const long long f = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (f >= F) return;
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  u64 m = m1[i0];
  m = m1[i1] < m ? m1[i1] : m;
  m = m1[i2] < m ? m1[i2] : m;
  if (m == SMP_NONE) return;
  atomicMin(m2 + i0, m);
  atomicMin(m2 + i1, m);
  atomicMin(m2 + i2, m);
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_win_flags(const u64* __restrict__ ekey, const u64* __restrict__ sorted,
                                                          const int32_t* __restrict__ ehead, long long n3, int s,
                                                          const u64* __restrict__ m2, long long* __restrict__ ctr,
                                                          int32_t* __restrict__ flags) {
  const long long e = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (e >= n3) return;
  int win = 0;
  if (e < ctr[CTR_E]) {
    const u64 key = ekey[e];
    if (key != SMP_NONE) {
      const u64 hk = sorted[ehead[e]];
      win = key == m2[hk >> s] && key == m2[hk & ((1ull << s) - 1)];
      if (win) atomicAdd((unsigned long long*)(ctr + CTR_R), (unsigned long long)(ehead[e + 1] - ehead[e]));
    }
  }
  flags[e] = win;
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_win_compact(const u64* __restrict__ ekey,
                                                            const int32_t* __restrict__ flags,
                                                            const int32_t* __restrict__ rank, long long n3,
                                                            u64* __restrict__ wkeys, long long* __restrict__ ctr) {
  const long long e = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (e >= n3) return;
  if (flags[e]) wkeys[rank[e]] = ekey[e];
  if (e == n3 - 1) ctr[CTR_W] = rank[e] + flags[e];
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_win_counts(const u64* __restrict__ wkeys, long long W,
                                                           const int32_t* __restrict__ ehead,
                                                           int32_t* __restrict__ cnt) {
  const long long i = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (i >= W) return;
  const long long e = (long long)(wkeys[i] & 0xFFFFFFFFull);
  cnt[i] = ehead[e + 1] - ehead[e];
}

// ------------------------------------------------------------------------------------------------ collapse, compact

__global__ __launch_bounds__(SMP_BLOCK) void smp_collapse(const u64* __restrict__ wkeys, long long W,
                                                         const int32_t* __restrict__ pre, long long need,
                                                         const u64* __restrict__ sorted,
                                                         const int32_t* __restrict__ ehead, int s,
                                                         const unsigned* __restrict__ vflag,
                                                         const uint32_t* __restrict__ vff,
                                                         const int32_t* __restrict__ vstart,
                                                         const int32_t* __restrict__ vend, float* P, double* Q,
                                                         int32_t* faces, long long* __restrict__ ctr) {
  const long long i = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (i >= W) return;
  if (pre && pre[i] >= need) return;
  if (pre) atomicAdd((unsigned long long*)(ctr + CTR_ACC), 1ull);
  const long long e = (long long)(wkeys[i] & 0xFFFFFFFFull);
  const u64 hk = sorted[ehead[e]];
  const int a = (int)(hk >> s), b = (int)(hk & ((1ull << s) - 1));
  float p[3];
  double cost;
  smp_place(Q, P, vflag, a, b, p, &cost);
  for (int j = vstart[b]; j < vend[b]; ++j) {
    const long long f = vff[j];
    if (smp_has(faces, f, a)) {
      faces[3 * f] = -1;
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (faces[3 * f + c] == b) faces[3 * f + c] = a;
    }
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) Q[10 * (long long)a + k] = Q[10 * (long long)a + k] + Q[10 * (long long)b + k];
#pragma unroll
  for (int c = 0; c < 3; ++c) P[3 * (long long)a + c] = p[c];
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_face_alive(const int32_t* __restrict__ faces, long long F,
                                                           int32_t* __restrict__ flags) {
  const long long f = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (f >= F) return;
  flags[f] = faces[3 * f] >= 0;
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_face_scatter(const int32_t* __restrict__ faces, long long F,
                                                             const int32_t* __restrict__ flags,
                                                             const int32_t* __restrict__ rank,
                                                             int32_t* __restrict__ out, long long* __restrict__ ctr) {
  const long long f = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (f >= F) return;
  if (flags[f]) {
    const long long o = rank[f];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * o + c] = faces[3 * f + c];
  }
  if (f == F - 1) ctr[CTR_F] = rank[f] + flags[f];
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_mark_used(const int32_t* __restrict__ faces, long long n3,
                                                          int32_t* __restrict__ used) {
  const long long i = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (i >= n3) return;
  used[faces[i]] = 1;
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_out_verts(const float* __restrict__ P, long long V,
                                                          const int32_t* __restrict__ used,
                                                          const int32_t* __restrict__ vnew, float* __restrict__ out,
                                                          long long* __restrict__ ctr) {
  const long long v = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (v >= V) return;
  if (used[v]) {
    const long long o = vnew[v];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * o + c] = P[3 * v + c];
  }
  if (v == V - 1) ctr[CTR_V] = vnew[v] + used[v];
}

__global__ __launch_bounds__(SMP_BLOCK) void smp_out_faces(const int32_t* __restrict__ faces, long long n3,
                                                          const int32_t* __restrict__ vnew,
                                                          int32_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * SMP_BLOCK + threadIdx.x;
  if (i >= n3) return;
  out[i] = vnew[faces[i]];
}

// ------------------------------------------------------------------------------------------------ host

struct SmpLayout {
  size_t pos, Q, vflag, vstart, vend, m1, m2, fa, fb, A, B, flags, rank, ehead, ekey, vfk, vff, ctr, tmp, tmp_bytes,
      total;
};

static int smp_layout(long long V, long long F, SmpLayout* l) {
  const size_t v = (size_t)V, n3 = 3 * (size_t)F, n = n3 > v ? n3 : v;
  mt::TmpCounts cnt = {};
  cnt.pairs64 = n3;
  cnt.keys64 = n3;
  cnt.pairs32 = n3;
  cnt.xscan32 = n;
  MT_TRY(mt::tmp_bytes(cnt, &l->tmp_bytes));
  mt::Bump b;
  l->pos = b.take(12 * v);
  l->Q = b.take(80 * v);
  l->vflag = b.take(4 * v);
  l->vstart = b.take(4 * v);
  l->vend = b.take(4 * v);
  l->m1 = b.take(8 * v);
  l->m2 = b.take(8 * v);
  l->fa = b.take(4 * n3);
  l->fb = b.take(4 * n3);
  l->A = b.take(8 * n3);
  l->B = b.take(8 * n3);
  l->flags = b.take(4 * n);
  l->rank = b.take(4 * n);
  l->ehead = b.take(4 * (n3 + 1));
  l->ekey = b.take(8 * n3);
  l->vfk = b.take(4 * n3);
  l->vff = b.take(4 * n3);
  l->ctr = b.take(8 * CTR_N);
  l->tmp = b.take(l->tmp_bytes);
  l->total = b.o;
  return VSA_OK;
}

extern "C" long long vsa_simplify_workspace_bytes(long long nr_verts, long long nr_faces) {
  SmpLayout l;
  int rc = mt::check_vf(nr_verts, nr_faces);
  if (rc == VSA_OK) rc = mt::abi_status(smp_layout(nr_verts, nr_faces, &l));
  return rc != VSA_OK ? rc : (long long)l.total;
}

namespace {

struct Smp {
  hipStream_t st;
  SmpLayout l;
  mt::Tmp tmp;
  long long V, F;
  int s;
  float* P;
  double* Q;
  unsigned* vflag;
  int32_t *vstart, *vend, *fcur, *fnext, *flags, *rank, *ehead;
  u64 *m1, *m2, *A, *B, *ekey;
  uint32_t *vfk, *vff;
  long long* ctr;
  mt::StageTimer timer;
};

// Unique edges of the F current faces (sorted keys in B, ids via flags / rank, ehead, E on the device); with
// `slots`, the sorted slot of every key lands in vff and the edge's face count at every face slot in slot_cnt.
int build_edges(Smp& m, bool slots, int32_t* slot_cnt) {
  const long long n3 = 3 * m.F;
  MT_TRY(mt::sorted_edges(m.fcur, m.F, m.s, m.A, m.B, slots ? m.vfk : nullptr, m.vff, m.tmp, m.st));
  hipLaunchKernelGGL(smp_heads, mt::grid(n3), dim3(SMP_BLOCK), 0, m.st, m.B, n3, m.flags);
  MT_LAUNCHED();
  MT_TRY(mt::exclusive_scan(m.tmp, m.flags, m.rank, (size_t)n3, m.st));
  hipLaunchKernelGGL(smp_edge_index, mt::grid(n3), dim3(SMP_BLOCK), 0, m.st, m.flags, m.rank, n3, m.ehead, m.ctr);
  MT_LAUNCHED();
  if (slots) {
    hipLaunchKernelGGL(smp_slot_counts, mt::grid(n3), dim3(SMP_BLOCK), 0, m.st, m.flags, m.rank, m.vff, m.ehead, n3,
                       slot_cnt);
    MT_LAUNCHED();
  }
  return VSA_OK;
}

// The (vertex, face) list sorted by vertex (stable: ascending face within a vertex) -> vff, vstart / vend.
int build_rings(Smp& m) {
  uint32_t* kin = reinterpret_cast<uint32_t*>(m.A);
  return mt::vertex_rings(m.fcur, m.F, m.V, m.s, kin, m.vfk, kin + 3 * m.F, m.vff, m.vstart, m.vend, m.tmp, m.st);
}

// The rounds.  `guards`: null (vsa_simplify) or the guard meshes of vsa_simplify_guarded, whose stage sits between cost
// and select and moves the later stages' timer slots up by one; stats then has a sixth entry.
int run(Smp& m, const float* verts, const int32_t* faces, long long target, const CrossGuards* guards, float* out_verts,
        int32_t* out_faces, long long* stats) {
  const long long V = m.V;
  const int later = guards ? 1 : 0;
  long long rounds = 0, collapses = 0, stalled = 0;
  MT_TRY(m.timer.open());
  VSA_HIP_TRY(hipMemcpyAsync(m.P, verts, 12 * (size_t)V, hipMemcpyDeviceToDevice, m.st));
  VSA_HIP_TRY(hipMemcpyAsync(m.fcur, faces, 12 * (size_t)m.F, hipMemcpyDeviceToDevice, m.st));
  VSA_HIP_TRY(hipMemsetAsync(m.ctr, 0, 8 * CTR_N, m.st));
  int32_t* slot_cnt = reinterpret_cast<int32_t*>(m.ekey);
  MT_TRY(build_edges(m, true, slot_cnt));
  MT_TRY(build_rings(m));
  hipLaunchKernelGGL(smp_quadrics, mt::grid(V), dim3(SMP_BLOCK), 0, m.st, m.P, m.fcur, m.vff, m.vstart, m.vend,
                     slot_cnt, V, m.Q);
  MT_LAUNCHED();
  MT_TRY(m.timer.close(0));
  while (m.F > target) {
    const long long n3 = 3 * m.F;
    // edges
    MT_TRY(m.timer.open());
    MT_TRY(build_edges(m, false, nullptr));
    VSA_HIP_TRY(hipMemsetAsync(m.vflag, 0, 4 * (size_t)V, m.st));
    hipLaunchKernelGGL(smp_vertex_flags, mt::grid(n3), dim3(SMP_BLOCK), 0, m.st, m.B, m.ehead, n3, m.s, m.ctr, m.vflag);
    MT_LAUNCHED();
    MT_TRY(build_rings(m));
    MT_TRY(m.timer.close(1));
    // cost
    MT_TRY(m.timer.open());
    hipLaunchKernelGGL(smp_cost, mt::grid(n3), dim3(SMP_BLOCK), 0, m.st, m.P, m.Q, m.vflag, m.fcur, m.B, m.ehead, m.vff,
                       m.vstart, m.vend, n3, m.s, m.ctr, m.ekey);
    MT_LAUNCHED();
    MT_TRY(m.timer.close(2));
    // guard
    if (guards) {
      MT_TRY(m.timer.open());
      const dim3 grid((unsigned)((n3 + TRACE_BLOCK - 1) / TRACE_BLOCK)), block(TRACE_BLOCK);
      with_stack(guards->max_depth, [&](auto sk) {
        hipLaunchKernelGGL((smp_guard<decltype(sk)::value>), grid, block, 0, m.st, m.P, m.Q, m.vflag, m.fcur, m.B,
                           m.ehead, m.vff, m.vstart, m.vend, m.s, m.ctr, m.ekey, *guards);
      });
      MT_LAUNCHED();
      MT_TRY(m.timer.close(3));
    }
    // select
    MT_TRY(m.timer.open());
    VSA_HIP_TRY(hipMemsetAsync(m.m1, 0xFF, 8 * (size_t)V, m.st));
    VSA_HIP_TRY(hipMemsetAsync(m.m2, 0xFF, 8 * (size_t)V, m.st));
    VSA_HIP_TRY(hipMemsetAsync(m.ctr + CTR_R, 0, 8, m.st));
    hipLaunchKernelGGL(smp_m1, mt::grid(n3), dim3(SMP_BLOCK), 0, m.st, m.ekey, m.B, m.ehead, m.s, m.ctr, m.m1);
    MT_LAUNCHED();
    hipLaunchKernelGGL(smp_m2, mt::grid(m.F), dim3(SMP_BLOCK), 0, m.st, m.fcur, m.F, m.m1, m.m2);
    MT_LAUNCHED();
    hipLaunchKernelGGL(smp_win_flags, mt::grid(n3), dim3(SMP_BLOCK), 0, m.st, m.ekey, m.B, m.ehead, n3, m.s, m.m2,
                       m.ctr, m.flags);
    MT_LAUNCHED();
    MT_TRY(mt::exclusive_scan(m.tmp, m.flags, m.rank, (size_t)n3, m.st));
    u64* wkeys = m.A;
    u64* wsorted = m.A + m.F;   // winners share no face: W <= F
    hipLaunchKernelGGL(smp_win_compact, mt::grid(n3), dim3(SMP_BLOCK), 0, m.st, m.ekey, m.flags, m.rank, n3, wkeys,
                       m.ctr);
    MT_LAUNCHED();
    long long wr[2];
    MT_TRY(mt::read_counters(m.st, m.ctr + CTR_W, wr, 2));
    const long long W = wr[0], R = wr[1], need = m.F - target;
    if (W < 0 || W > m.F) return VSA_ERR_UNSUPPORTED;
    if (W == 0) {
      MT_TRY(m.timer.close(3 + later));
      stalled = 1;
      break;
    }
    const u64* list = wkeys;
    const int32_t* pre = nullptr;
    if (R > need) {
      MT_TRY(mt::sort_keys(m.tmp, wkeys, wsorted, (size_t)W, 0, 64, m.st));
      hipLaunchKernelGGL(smp_win_counts, mt::grid(W), dim3(SMP_BLOCK), 0, m.st, wsorted, W, m.ehead, m.flags);
      MT_LAUNCHED();
      MT_TRY(mt::exclusive_scan(m.tmp, m.flags, m.rank, (size_t)W, m.st));
      list = wsorted;
      pre = m.rank;
    }
    MT_TRY(m.timer.close(3 + later));
    // collapse
    MT_TRY(m.timer.open());
    hipLaunchKernelGGL(smp_collapse, mt::grid(W), dim3(SMP_BLOCK), 0, m.st, list, W, pre, need, m.B, m.ehead, m.s,
                       m.vflag, m.vff, m.vstart, m.vend, m.P, m.Q, m.fcur, m.ctr);
    MT_LAUNCHED();
    MT_TRY(m.timer.close(4 + later));
    // compact
    MT_TRY(m.timer.open());
    hipLaunchKernelGGL(smp_face_alive, mt::grid(m.F), dim3(SMP_BLOCK), 0, m.st, m.fcur, m.F, m.flags);
    MT_LAUNCHED();
    MT_TRY(mt::exclusive_scan(m.tmp, m.flags, m.rank, (size_t)m.F, m.st));
    hipLaunchKernelGGL(smp_face_scatter, mt::grid(m.F), dim3(SMP_BLOCK), 0, m.st, m.fcur, m.F, m.flags, m.rank, m.fnext,
                       m.ctr);
    MT_LAUNCHED();
    int32_t* t = m.fcur;
    m.fcur = m.fnext;
    m.fnext = t;
    ++rounds;
    if (pre) {
      // the last round: read the faces left and the accepted collapses back (F <= target now)
      long long fa[2];
      MT_TRY(mt::read_counters(m.st, m.ctr + CTR_F, fa, 2));
      if (fa[0] < 0 || fa[0] > target || fa[1] < 1 || fa[1] > W) return VSA_ERR_UNSUPPORTED;
      collapses += fa[1];
      m.F = fa[0];
    } else {
      collapses += W;
      m.F -= R;
    }
    MT_TRY(m.timer.close(5 + later));
  }
  // output: the referenced vertices in ascending index, faces in order
  MT_TRY(m.timer.open());
  const long long n3 = 3 * m.F;
  VSA_HIP_TRY(hipMemsetAsync(m.flags, 0, 4 * (size_t)V, m.st));
  hipLaunchKernelGGL(smp_mark_used, mt::grid(n3), dim3(SMP_BLOCK), 0, m.st, m.fcur, n3, m.flags);
  MT_LAUNCHED();
  MT_TRY(mt::exclusive_scan(m.tmp, m.flags, m.rank, (size_t)V, m.st));
  hipLaunchKernelGGL(smp_out_verts, mt::grid(V), dim3(SMP_BLOCK), 0, m.st, m.P, V, m.flags, m.rank, out_verts, m.ctr);
  MT_LAUNCHED();
  if (n3 > 0) {
    hipLaunchKernelGGL(smp_out_faces, mt::grid(n3), dim3(SMP_BLOCK), 0, m.st, m.fcur, n3, m.rank, out_faces);
    MT_LAUNCHED();
  }
  long long vg[2];
  MT_TRY(mt::read_counters(m.st, m.ctr + CTR_V, vg, 2));
  MT_TRY(m.timer.close(5 + later));
  stats[0] = rounds;
  stats[1] = collapses;
  stats[2] = stalled;
  stats[3] = vg[0];
  stats[4] = m.F;
  if (guards) stats[5] = vg[1];
  return VSA_OK;
}

}  // namespace

namespace {

// Binds the workspace and runs: the body both entry points share.
int simplify(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces, long long target_faces,
             const CrossGuards* guards, void* workspace, long long workspace_bytes, float* out_verts,
             int32_t* out_faces, long long* stats, float* stage_ms, void* stream) {
  if (!verts || !faces || !workspace || !out_verts || !out_faces || !stats || target_faces < 0) return VSA_ERR_ARG;
  MT_TRY(mt::check_vf(nr_verts, nr_faces));
  Smp m;
  MT_TRY(mt::abi_status(smp_layout(nr_verts, nr_faces, &m.l)));
  if (workspace_bytes < (long long)m.l.total) return VSA_ERR_ARG;
  char* ws = static_cast<char*>(workspace);
  const SmpLayout& l = m.l;
  m.st = (hipStream_t)stream;
  m.tmp = {ws + l.tmp, l.tmp_bytes};
  m.V = nr_verts;
  m.F = nr_faces;
  m.s = mt::bits_of(nr_verts);
  m.P = mt::at<float>(ws, l.pos);
  m.Q = mt::at<double>(ws, l.Q);
  m.vflag = mt::at<unsigned>(ws, l.vflag);
  m.vstart = mt::at<int32_t>(ws, l.vstart);
  m.vend = mt::at<int32_t>(ws, l.vend);
  m.m1 = mt::at<u64>(ws, l.m1);
  m.m2 = mt::at<u64>(ws, l.m2);
  m.fcur = mt::at<int32_t>(ws, l.fa);
  m.fnext = mt::at<int32_t>(ws, l.fb);
  m.A = mt::at<u64>(ws, l.A);
  m.B = mt::at<u64>(ws, l.B);
  m.flags = mt::at<int32_t>(ws, l.flags);
  m.rank = mt::at<int32_t>(ws, l.rank);
  m.ehead = mt::at<int32_t>(ws, l.ehead);
  m.ekey = mt::at<u64>(ws, l.ekey);
  m.vfk = mt::at<uint32_t>(ws, l.vfk);
  m.vff = mt::at<uint32_t>(ws, l.vff);
  m.ctr = mt::at<long long>(ws, l.ctr);
  MT_TRY(m.timer.create(stage_ms, guards ? 7 : 6, m.st));
  const int rc = run(m, verts, faces, target_faces, guards, out_verts, out_faces, stats);
  m.timer.destroy();
  return rc;
}

}  // namespace

extern "C" int vsa_simplify(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                            long long target_faces, void* workspace, long long workspace_bytes, float* out_verts,
                            int32_t* out_faces, long long* stats, float* stage_ms, void* stream) {
  return simplify(verts, nr_verts, faces, nr_faces, target_faces, nullptr, workspace, workspace_bytes, out_verts,
                  out_faces, stats, stage_ms, stream);
}

// The guard stage reads the rounds' own buffers and writes the keys in place: the workspace is vsa_simplify's.
extern "C" long long vsa_simplify_guarded_workspace_bytes(long long nr_verts, long long nr_faces) {
  return vsa_simplify_workspace_bytes(nr_verts, nr_faces);
}

extern "C" int vsa_simplify_guarded(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                                    long long target_faces, int nr_guards, const uint32_t* const* guard_qnodes,
                                    const float* const* guard_tris, const int32_t* guard_roots,
                                    const float* guard_frames, const int32_t* guard_max_depths,
                                    const float* const* guard_vertices, const long long* guard_nr_verts,
                                    const int32_t* const* guard_faces, const long long* guard_nr_faces,
                                    void* workspace, long long workspace_bytes, float* out_verts, int32_t* out_faces,
                                    long long* stats, float* stage_ms, void* stream) {
  CrossGuards G;
  MT_TRY(cross_guards_bind(nr_guards, guard_qnodes, guard_tris, guard_roots, guard_frames, guard_max_depths,
                           guard_vertices, guard_nr_verts, guard_faces, guard_nr_faces, &G));
  return simplify(verts, nr_verts, faces, nr_faces, target_faces, &G, workspace, workspace_bytes, out_verts, out_faces,
                  stats, stage_ms, stream);
}
