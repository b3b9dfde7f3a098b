// Which faces of two meshes cross?  The triangle-triangle rule and the box-overlap walk of the quantised (q16) BVH
// nodes, for the kernels of mesh_cross.hip (the count pass and the emit pass walk the same text, so that they find the
// same pairs) and for the guards of simplify.hip and mesh_smooth.hip (one guard block, one loop over it).  The nodes,
// their grid, the stack's shape and the host side of the tree arguments are the ray walk's (trace_walk.h).
// The rule is this library's own (the reference has no such stage): include/volsurfs_hip.h
// "Mesh crossings"; tests/mesh_intersect_restated.py restates it in numpy, operation for operation.
#pragma once
#include "trace_walk.h"

namespace {

// A triangle as the fp32 bits of its mesh's vertex array, converted to fp64: x[i], y[i], z[i] of vertex i.
struct CrossTri {
  double x[3], y[3], z[3];
};

// orient(a, b, c, d) = det[a - d; b - d; c - d] along its first row:
//   p = a - d, q = b - d, r = c - d;  m0 = q.y r.z - q.z r.y,  m1 = q.x r.z - q.z r.x,  m2 = q.x r.y - q.y r.x;
//   (p.x m0 - p.y m1) + p.z m2.   fp64, no contraction (the Makefile's -ffp-contract=off).
__device__ __forceinline__ double cross_orient(double ax, double ay, double az, double bx, double by, double bz,
                                               double cx, double cy, double cz, double dx, double dy, double dz) {
  const double px = ax - dx, py = ay - dy, pz = az - dz;
  const double qx = bx - dx, qy = by - dy, qz = bz - dz;
  const double rx = cx - dx, ry = cy - dy, rz = cz - dz;
  const double m0 = qy * rz - qz * ry;
  const double m1 = qx * rz - qz * rx;
  const double m2 = qx * ry - qy * rx;
  return (px * m0 - py * m1) + pz * m2;
}

__device__ __forceinline__ bool cross_opposite(double s, double t) { return (s < 0.0 && t > 0.0) || (s > 0.0 && t < 0.0); }

__device__ __forceinline__ bool cross_one_sign(double x, double y, double z) {
  return (x >= 0.0 && y >= 0.0 && z >= 0.0) || (x <= 0.0 && y <= 0.0 && z <= 0.0);
}

// Do A and B cross?  The six sides, then -- only when some pair of sides is strictly opposite -- the e[i][j] that
// such an edge reads (signs only: a determinant no live condition reads is skipped).  SEG: seg[0..2] = the piercing
// point of the first piercing edge in the order A's edges 0, 1, 2, B's edges 0, 1, 2, seg[3..5] = that of the last:
// p + t (q - p), t = s_p / (s_p - s_q).
template <bool SEG>
__device__ __forceinline__ bool tri_cross(const CrossTri& A, const CrossTri& B, double* seg) {
  double sA[3], sB[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    sB[i] = cross_orient(B.x[0], B.y[0], B.z[0], B.x[1], B.y[1], B.z[1], B.x[2], B.y[2], B.z[2], A.x[i], A.y[i], A.z[i]);
    sA[i] = cross_orient(A.x[0], A.y[0], A.z[0], A.x[1], A.y[1], A.z[1], A.x[2], A.y[2], A.z[2], B.x[i], B.y[i], B.z[i]);
  }
  bool numbers = true, oa[3], ob[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    numbers = numbers && sA[i] == sA[i] && sB[i] == sB[i];
    oa[i] = cross_opposite(sB[i], sB[(i + 1) % 3]);
    ob[i] = cross_opposite(sA[i], sA[(i + 1) % 3]);
  }
  if (!numbers || !(oa[0] || oa[1] || oa[2] || ob[0] || ob[1] || ob[2])) return false;
  double e[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int i1 = (i + 1) % 3, j1 = (j + 1) % 3;
      e[i][j] = 0.0;
      if (oa[i] || ob[j])
        e[i][j] = cross_orient(A.x[i], A.y[i], A.z[i], A.x[i1], A.y[i1], A.z[i1], B.x[j], B.y[j], B.z[j], B.x[j1],
                               B.y[j1], B.z[j1]);
    }
  bool pierce[6];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    pierce[i] = oa[i] && cross_one_sign(e[i][0], e[i][1], e[i][2]);
    pierce[3 + i] = ob[i] && cross_one_sign(e[0][i], e[1][i], e[2][i]);
  }
  const bool any = pierce[0] || pierce[1] || pierce[2] || pierce[3] || pierce[4] || pierce[5];
  if constexpr (SEG) {
    if (any) {
      bool found = false;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (!pierce[k]) continue;
        const int i = k % 3, i1 = (i + 1) % 3;
        const CrossTri& T = k < 3 ? A : B;
        const double sp = k < 3 ? sB[i] : sA[i], sq = k < 3 ? sB[i1] : sA[i1];
        const double t = sp / (sp - sq);
        const double px = T.x[i] + t * (T.x[i1] - T.x[i]);
        const double py = T.y[i] + t * (T.y[i1] - T.y[i]);
        const double pz = T.z[i] + t * (T.z[i1] - T.z[i]);
        if (!found) seg[0] = px, seg[1] = py, seg[2] = pz;
        seg[3] = px, seg[4] = py, seg[5] = pz;
        found = true;
      }
    }
  }
  return any;
}

// A mesh as the walk reads it: faces [F, 3] into vertices [V, 3].  A face with an index outside 0 .. V - 1 is read
// as no face at all (it crosses nothing); nothing outside the two arrays is touched.
struct CrossMesh {
  const float* vertices;
  const int32_t* faces;
  long long V, F;
};

__device__ __forceinline__ bool cross_face_ok(const CrossMesh& m, long long f, int& i0, int& i1, int& i2) {
  i0 = i1 = i2 = 0;
  if (f < 0 || f >= m.F) return false;
  i0 = m.faces[3 * f], i1 = m.faces[3 * f + 1], i2 = m.faces[3 * f + 2];
  const bool ok = i0 >= 0 && i0 < m.V && i1 >= 0 && i1 < m.V && i2 >= 0 && i2 < m.V;
  if (!ok) i0 = i1 = i2 = 0;
  return ok;
}

__device__ __forceinline__ void cross_vertex(const CrossMesh& m, int v, int k, CrossTri& T, float* fx, float* fy,
                                             float* fz) {
  const float x = m.vertices[3 * (long long)v], y = m.vertices[3 * (long long)v + 1], z = m.vertices[3 * (long long)v + 2];
  T.x[k] = (double)x, T.y[k] = (double)y, T.z[k] = (double)z;
  if (fx) fx[k] = x, fy[k] = y, fz[k] = z;
}

// The query triangle's box in a mesh's 16-bit grid: closest_qpoint's g = (p - lo) / step + 1 of the fp32 minimum and
// maximum of its three vertices.  Each g carries three roundings, each relative to its own result: below 2^-22 |g|,
// i.e. below 2^-6 of a unit wherever g can decide a comparison with a u16 coordinate (|g| <= 65536), at any distance
// of the query from the mesh -- inside the boxes' outward margin of at least one unit.
struct CrossBox {
  float lox, loy, loz, hix, hiy, hiz;
};

__device__ __forceinline__ CrossBox cross_qbox(const float* fr, const float* x, const float* y, const float* z) {
  CrossBox q;
  q.lox = (fminf(fminf(x[0], x[1]), x[2]) - fr[0]) / fr[3] + 1.0f;
  q.loy = (fminf(fminf(y[0], y[1]), y[2]) - fr[1]) / fr[4] + 1.0f;
  q.loz = (fminf(fminf(z[0], z[1]), z[2]) - fr[2]) / fr[5] + 1.0f;
  q.hix = (fmaxf(fmaxf(x[0], x[1]), x[2]) - fr[0]) / fr[3] + 1.0f;
  q.hiy = (fmaxf(fmaxf(y[0], y[1]), y[2]) - fr[1]) / fr[4] + 1.0f;
  q.hiz = (fmaxf(fmaxf(z[0], z[1]), z[2]) - fr[2]) / fr[5] + 1.0f;
  return q;
}

// Does the child box (w0, w1, w2) overlap the query's box?  Closed on both sides.
__device__ __forceinline__ bool qbox_overlap(unsigned w0, unsigned w1, unsigned w2, const CrossBox& q) {
  const float lox = (float)(w0 & 0xffffu), loy = (float)(w0 >> 16), loz = (float)(w1 & 0xffffu);
  const float hix = (float)(w1 >> 16), hiy = (float)(w2 & 0xffffu), hiz = (float)(w2 >> 16);
  return lox <= q.hix && hix >= q.lox && loy <= q.hiy && hiy >= q.loy && loz <= q.hiz && hiz >= q.loz;
}

// The walk, in q_walk's form: wave-level loops on ballots, inner nodes until every lane holds a leaf, then the leaves
// together.  A child is entered iff its box overlaps the query's; no pruning, no order.  At a leaf: slot -> original
// face id (the record's v0.w) -> the tree mesh's faces row -> its vertices, four faces at a time with the three
// dependent gathers of the four issued before the first determinant; then the rule.  SELF: the tree mesh is the query
// mesh; face `face` against itself is skipped, the pair is evaluated with the lower face id as A whichever lane finds
// it, and UPPER_ONLY (the emit pass) evaluates only the partners above `face`.  on_cross(tree face id, seg) per crossing.
template <int STACK, bool SELF, bool UPPER_ONLY, bool SEG, class F>
__device__ __forceinline__ void cross_walk(const uint4* __restrict__ qnodes, const float4* __restrict__ tris,
                                           const CrossMesh& tree, const CrossTri& Q, const CrossBox& qb, int face,
                                           int cur, int (*s_node)[TRACE_BLOCK], int lane, F&& on_cross) {
  int sp = 0;
  while (__builtin_amdgcn_ballot_w64(cur != TRACE_EMPTY) != 0) {
    while (__builtin_amdgcn_ballot_w64((unsigned)cur < (unsigned)TRACE_EMPTY) != 0) {
      if (!((unsigned)cur < (unsigned)TRACE_EMPTY)) continue;
      const uint4 a = qnodes[2 * (long long)cur], b = qnodes[2 * (long long)cur + 1];
      const int c0 = (int)b.z, c1 = (int)b.w;
      const bool h0 = c0 != TRACE_EMPTY && qbox_overlap(a.x, a.y, a.z, qb);
      const bool h1 = c1 != TRACE_EMPTY && qbox_overlap(a.w, b.x, b.y, qb);
      if (h0 && h1) {
        s_node[sp++][lane] = c1;
        cur = c0;
      } else if (h0) {
        cur = c0;
      } else if (h1) {
        cur = c1;
      } else {
        cur = sp ? s_node[--sp][lane] : TRACE_EMPTY;
      }
    }
    if (cur != TRACE_EMPTY) {
      const int code = ~cur;
      const int first = code >> 4, cnt = code & 15;
      for (int i0 = 0; i0 < cnt; i0 += 4) {
        int id[4], vi[4][3];
        bool ok[4];
        CrossTri T[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) id[i] = __float_as_int(tris[3 * (long long)(first + min(i0 + i, cnt - 1))].w);
#pragma unroll
        for (int i = 0; i < 4; ++i) ok[i] = cross_face_ok(tree, id[i], vi[i][0], vi[i][1], vi[i][2]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int k = 0; k < 3; ++k) cross_vertex(tree, vi[i][k], k, T[i], nullptr, nullptr, nullptr);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (i0 + i >= cnt || !ok[i]) continue;
          if (SELF && (id[i] == face || (UPPER_ONLY && id[i] < face))) continue;
          double seg[6];
          const bool lower = !SELF || face < id[i];
          const CrossTri A = lower ? Q : T[i], B = lower ? T[i] : Q;
          if (tri_cross<SEG>(A, B, seg)) on_cross(id[i], seg);
        }
      }
      cur = sp ? s_node[--sp][lane] : TRACE_EMPTY;
    }
  }
}

// ------------------------------------------------------------------------------------------------ guards
// Up to CROSS_MAX_GUARDS meshes that a moving face must not cross: the guard block of vsa_simplify_guarded and
// vsa_mesh_smooth_guard (include/volsurfs_hip.h states the arrays' contract once, at vsa_simplify_guarded).

constexpr int CROSS_MAX_GUARDS = 4;

// One guard mesh: its q16 tree as cross_walk reads it, and the grid of that tree.
struct CrossGuard {
  const uint4* qnodes;
  const float4* tris;
  int root;
  float frame[6];
  CrossMesh mesh;
};

struct CrossGuards {
  int n, max_depth;
  CrossGuard g[CROSS_MAX_GUARDS];
};

// The status of the guard arrays, in the order the entry points document, and the block for the kernels.
inline int cross_guards_bind(int nr_guards, const uint32_t* const* guard_qnodes, const float* const* guard_tris,
                             const int32_t* guard_roots, const float* guard_frames, const int32_t* guard_max_depths,
                             const float* const* guard_vertices, const long long* guard_nr_verts,
                             const int32_t* const* guard_faces, const long long* guard_nr_faces, CrossGuards* out) {
  if (nr_guards < 1 || nr_guards > CROSS_MAX_GUARDS) return VSA_ERR_ARG;
  if (!guard_qnodes || !guard_tris || !guard_roots || !guard_frames || !guard_max_depths || !guard_vertices ||
      !guard_nr_verts || !guard_faces || !guard_nr_faces)
    return VSA_ERR_ARG;
  CrossGuards G = {};
  G.n = nr_guards;
  for (int g = 0; g < nr_guards; ++g) {
    if (const int rc = check_qtree(guard_qnodes[g], guard_tris[g], guard_roots + g, guard_frames + 6 * g, 1,
                                   guard_max_depths[g], VSA_ERR_ARG))
      return rc;
    if (guard_roots[g] < 0 || !guard_vertices[g] || !guard_faces[g]) return VSA_ERR_ARG;
    if (guard_nr_verts[g] < 1 || guard_nr_faces[g] < 1) return VSA_ERR_ARG;
    if (guard_nr_verts[g] > 0x7fffffffll || guard_nr_faces[g] > 0x7fffffffll / 3 - 1) return VSA_ERR_UNSUPPORTED;
    CrossGuard& d = G.g[g];
    d.qnodes = reinterpret_cast<const uint4*>(guard_qnodes[g]);
    d.tris = reinterpret_cast<const float4*>(guard_tris[g]);
    d.root = guard_roots[g];
    for (int k = 0; k < 6; ++k) d.frame[k] = guard_frames[6 * g + k];
    d.mesh = CrossMesh{guard_vertices[g], guard_faces[g], guard_nr_verts[g], guard_nr_faces[g]};
    G.max_depth = guard_max_depths[g] > G.max_depth ? guard_max_depths[g] : G.max_depth;
  }
  *out = G;
  return VSA_OK;
}

// Does the face T (fp32 corners x, y, z) cross a face of a guard?  Sets `hit`, the lane's verdict, and never clears
// it.  cross_walk loops on wave ballots, so every lane enters the walk of every guard: a lane that is not `live`, or
// that has its verdict (from an earlier face too), walks from TRACE_EMPTY.
template <int STACK>
__device__ __forceinline__ void cross_guards_hit(const CrossGuards& G, const CrossTri& T, const float* x,
                                                 const float* y, const float* z, bool live, bool& hit,
                                                 int (*s_node)[TRACE_BLOCK], int lane) {
  for (int g = 0; g < G.n; ++g) {
    const CrossGuard& gd = G.g[g];
    const CrossBox qb = cross_qbox(gd.frame, x, y, z);
    cross_walk<STACK, false, false, false>(gd.qnodes, gd.tris, gd.mesh, T, qb, 0, live && !hit ? gd.root : TRACE_EMPTY,
                                           s_node, lane, [&](int, const double*) { hit = true; });
  }
}

}  // namespace
