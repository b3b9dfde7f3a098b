// On which side of a mesh is a point?  (The reference has no such stage: the rule is this library's own --
// include/volsurfs_hip.h "Mesh signed distance", DESIGN §29: restated in tests/mesh_sdf_restated.py, unpinned.)
//
// The sign of the distance the closest-point walk finds (closest_walk.h) by the angle-weighted pseudonormal
// of the closest feature (Baerentzen & Aanaes 2005): the closest record, its region (a vertex, an edge, the interior)
// and the residual r = p - closest point come out of the walk; N is the pseudonormal of that feature; the distance is
// negative when r . N < 0.
// vsa_mesh_pseudonormals: the table [F, 7, 3] f32 indexed by original face id and region code (the three vertex, the
//   three edge pseudonormals and the face normal of every face), so that a query needs no connectivity.  Vertex rings
//   and sorted edges are mesh_topology's; one thread per vertex walks its ring in order, one thread per face corner the
//   run of its edge key in order; fp64 sums, stored as fp32.  No float atomics: the same bytes on every call.
// vsa_signed_distance_q: vsa_closest_point_q with `dist` signed: one record and one table fetch and a dot product
//   after the walk (closest_walk.h: signed_distance, shared with csrc/shell_untangle.hip).
// vsa_mesh_sdf_grid: the field on a lattice given by its three axes, clamped to a band.  A wave is a 4 x 4 x 4 brick of
//   lattice points.  With a finite band one lane per brick first asks at the brick's centre: a brick farther from the
//   surface than the band plus its own radius is filled with +-band, the others are compacted in order (flags, scan,
//   scatter) and only they are walked.
#include "closest_walk.h"
#include "mesh_topology.h"

namespace {

constexpr int SDF_BRICK = 4;                  // a wave: SDF_BRICK^3 = 64 lattice points
constexpr long long MAX_GRID = 0x7fffffffll;

struct d3 {
  double x, y, z;
};

__device__ __forceinline__ d3 vertex_d3(const float* __restrict__ P, long long v) {
  return {(double)P[3 * v], (double)P[3 * v + 1], (double)P[3 * v + 2]};
}
__device__ __forceinline__ d3 sub_d3(const d3 a, const d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ d3 cross_d3(const d3 a, const d3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double dot_d3(const d3 a, const d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// ---- tables

// fn[f] = (e1 x e2) / |e1 x e2| in fp64 on the fp32 vertices, 0 for a face without a positive finite area; the same
// vector, rounded, into the face's CR_IN entry.
__global__ __launch_bounds__(MT_BLOCK) void pn_face_kernel(const float* __restrict__ P,
                                                           const int32_t* __restrict__ faces, long long F,
                                                           double* __restrict__ fn, float* __restrict__ table) {
  const long long f = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (f >= F) return;
  const d3 a = vertex_d3(P, faces[3 * f]);
  const d3 n = cross_d3(sub_d3(vertex_d3(P, faces[3 * f + 1]), a), sub_d3(vertex_d3(P, faces[3 * f + 2]), a));
  const double len = sqrt(dot_d3(n, n));
  const bool ok = len > 0.0 && len < INFINITY;
  const d3 u = {ok ? n.x / len : 0.0, ok ? n.y / len : 0.0, ok ? n.z / len : 0.0};
  fn[3 * f] = u.x, fn[3 * f + 1] = u.y, fn[3 * f + 2] = u.z;
  float* row = table + f * PN_FLOATS + 3 * CR_IN;
  row[0] = (float)u.x, row[1] = (float)u.y, row[2] = (float)u.z;
}

// nv[v] = sum over the ring of v, in ascending face id, of alpha fn[f]: alpha the face's interior angle at v (at the
// first corner that names v), atan2(|a x b|, a . b) of the two edges leaving v.
__global__ __launch_bounds__(MT_BLOCK) void pn_vertex_kernel(const float* __restrict__ P,
                                                             const int32_t* __restrict__ faces,
                                                             const double* __restrict__ fn,
                                                             const uint32_t* __restrict__ vff,
                                                             const int32_t* __restrict__ vstart,
                                                             const int32_t* __restrict__ vend, long long V,
                                                             float* __restrict__ nv) {
  const long long v = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (v >= V) return;
  const d3 p = vertex_d3(P, v);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = vstart[v]; j < vend[v]; ++j) {
    const long long f = vff[j];
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    const int c = i0 == (int)v ? 0 : (i1 == (int)v ? 1 : 2);
    const int o1 = c == 0 ? i1 : (c == 1 ? i2 : i0), o2 = c == 0 ? i2 : (c == 1 ? i0 : i1);
    const d3 a = sub_d3(vertex_d3(P, o1), p), b = sub_d3(vertex_d3(P, o2), p);
    const d3 cr = cross_d3(a, b);
    const double alpha = atan2(sqrt(dot_d3(cr, cr)), dot_d3(a, b));
    sx += alpha * fn[3 * f], sy += alpha * fn[3 * f + 1], sz += alpha * fn[3 * f + 2];
  }
  nv[3 * v] = (float)sx, nv[3 * v + 1] = (float)sy, nv[3 * v + 2] = (float)sz;
}

// The vertex entries of every face: corner c of face f takes its vertex's sum (CR_A, CR_B, CR_C = 0, 1, 2).
__global__ __launch_bounds__(MT_BLOCK) void pn_corner_kernel(const int32_t* __restrict__ faces, long long n3,
                                                             const float* __restrict__ nv, float* __restrict__ table) {
  const long long i = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= n3) return;
  const long long f = i / 3, v = faces[i];
  const int c = (int)(i - 3 * f);
  float* row = table + f * PN_FLOATS + 3 * c;
  row[0] = nv[3 * v], row[1] = nv[3 * v + 1], row[2] = nv[3 * v + 2];
}

// The edge entries: position j of the sorted edge keys finds the run of its key and adds the face normals of the run in
// order (the sort is stable: ascending face id), for the face corner the position came from.  Corner c is the edge from
// vertex c to the next: v0 v1, v1 v2, v2 v0.
__global__ __launch_bounds__(MT_BLOCK) void pn_edge_kernel(const mt::u64* __restrict__ sorted,
                                                           const uint32_t* __restrict__ slot, long long n3,
                                                           const double* __restrict__ fn, float* __restrict__ table) {
  const long long j = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (j >= n3) return;
  const mt::u64 key = sorted[j];
  long long lo = j;
  while (lo > 0 && sorted[lo - 1] == key) --lo;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (long long k = lo; k < n3 && sorted[k] == key; ++k) {
    const long long f = slot[k] / 3;
    sx += fn[3 * f], sy += fn[3 * f + 1], sz += fn[3 * f + 2];
  }
  const long long i = slot[j], f = i / 3;
  const int c = (int)(i - 3 * f);
  const int region = c == 0 ? CR_AB : (c == 1 ? CR_BC : CR_AC);
  float* row = table + f * PN_FLOATS + 3 * region;
  row[0] = (float)sx, row[1] = (float)sy, row[2] = (float)sz;
}

struct PnLayout {
  size_t fn, nv, A, B, va, vb, vstart, vend, tmp, tmp_bytes, total;
};

int pn_layout(long long V, long long F, PnLayout* l) {
  mt::TmpCounts c = {};
  c.pairs64 = c.pairs32 = 3 * (size_t)F;
  MT_TRY(mt::tmp_bytes(c, &l->tmp_bytes));
  mt::Bump b;
  l->fn = b.take(24 * (size_t)F);
  l->nv = b.take(12 * (size_t)V);
  l->A = b.take(24 * (size_t)F);
  l->B = b.take(24 * (size_t)F);
  l->va = b.take(12 * (size_t)F);
  l->vb = b.take(12 * (size_t)F);
  l->vstart = b.take(4 * (size_t)V);
  l->vend = b.take(4 * (size_t)V);
  l->tmp = b.take(l->tmp_bytes);
  l->total = b.o;
  return VSA_OK;
}

// ---- the sign

struct TableBase {
  long long face[VSA_MAX_SHELLS];   // first row of each mesh's faces in the table
};

template <int STACK, bool BOUNDS>
__global__ __launch_bounds__(TRACE_BLOCK) void signed_distance_kernel(
    const uint4* __restrict__ qnodes, const float4* __restrict__ tris, Roots roots, Frames frames,
    const float* __restrict__ table, TableBase base, const float* __restrict__ points, long long nr_points,
    float* __restrict__ dist, int* __restrict__ slot, float* __restrict__ bary) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  __shared__ float s_bound[BOUNDS ? STACK : 1][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const int mesh = blockIdx.y;
  const long long i = (long long)blockIdx.x * TRACE_BLOCK + lane;
  const bool alive = i < nr_points;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (alive) px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
  const QPoint q = closest_qpoint(frames.f[mesh], px, py, pz);
  Closest best = no_closest();
  closest_walk<STACK, BOUNDS>(qnodes, tris, q, px, py, pz, alive ? roots.root[mesh] : TRACE_EMPTY, best, s_node, s_bound,
                              lane);
  if (!alive) return;
  const long long o = (long long)mesh * nr_points + i;
  dist[o] = signed_distance(tris, table, base.face[mesh], best, px, py, pz);
  slot[o] = best.slot;
  if (bary) {
    bary[2 * o] = best.u;
    bary[2 * o + 1] = best.v;
  }
}

// ---- the lattice

struct Lattice {
  const float *x, *y, *z;
  int nx, ny, nz;      // points
  int bx, by, bz;      // bricks: ceil(n / 4)
};

// One lane per brick: the signed distance d_c at the brick's centre (the mean of its first and last axis value, per
// axis) and the brick's radius rho, the distance from the centre to its farthest lattice point.  near[b] = 0 when
// |d_c| > band + (4/3) rho: the distance is 1-Lipschitz, so every point of such a brick lies beyond the band on the
// centre's side.
template <int STACK, bool BOUNDS>
__global__ __launch_bounds__(TRACE_BLOCK) void brick_classify_kernel(
    const uint4* __restrict__ qnodes, const float4* __restrict__ tris, Roots roots, Frames frames,
    const float* __restrict__ table, long long base, Lattice g, long long nr_bricks, float band,
    int32_t* __restrict__ near, float* __restrict__ centre_dist) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  __shared__ float s_bound[BOUNDS ? STACK : 1][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const long long b = (long long)blockIdx.x * TRACE_BLOCK + lane;
  const bool alive = b < nr_bricks;
  float c[3] = {0.f, 0.f, 0.f}, h[3] = {0.f, 0.f, 0.f};
  if (alive) {
    const int k0 = (int)(b % g.bz) * SDF_BRICK, j0 = (int)((b / g.bz) % g.by) * SDF_BRICK;
    const int i0 = (int)(b / ((long long)g.bz * g.by)) * SDF_BRICK;
    const float* axis[3] = {g.x, g.y, g.z};
    const int first[3] = {i0, j0, k0}, n[3] = {g.nx, g.ny, g.nz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int last = min(first[a] + SDF_BRICK - 1, n[a] - 1);
      c[a] = 0.5f * (axis[a][first[a]] + axis[a][last]);
      for (int t = first[a]; t <= last; ++t) h[a] = fmaxf(h[a], fabsf(axis[a][t] - c[a]));
    }
  }
  const QPoint q = closest_qpoint(frames.f[0], c[0], c[1], c[2]);
  Closest best = no_closest();
  closest_walk<STACK, BOUNDS>(qnodes, tris, q, c[0], c[1], c[2], alive ? roots.root[0] : TRACE_EMPTY, best, s_node,
                              s_bound, lane);
  if (!alive) return;
  const float dc = signed_distance(tris, table, base, best, c[0], c[1], c[2]);
  const float rho = sqrtf((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]);
  centre_dist[b] = dc;
  near[b] = fabsf(dc) > band + (4.0f / 3.0f) * rho ? 0 : 1;     // (a NaN anywhere: near)
}

// A wave per brick: a near brick goes to its rank in the list (ascending brick index), a far one is filled with
// copysignf(band, d_c).  The last brick's wave also writes the two counts.
constexpr int FILL_BLOCK = 256;

__global__ __launch_bounds__(FILL_BLOCK) void brick_fill_kernel(Lattice g, long long nr_bricks, float band,
                                                                const int32_t* __restrict__ near,
                                                                const int32_t* __restrict__ rank,
                                                                const float* __restrict__ centre_dist,
                                                                int32_t* __restrict__ list, float* __restrict__ out,
                                                                long long* __restrict__ counts) {
  const int lane = threadIdx.x & (VSA_WAVE - 1);
  const long long b = (long long)blockIdx.x * (FILL_BLOCK / VSA_WAVE) + threadIdx.x / VSA_WAVE;
  if (b >= nr_bricks) return;
  const int is_near = near[b];
  if (lane == 0 && b == nr_bricks - 1) {
    const long long n = (long long)rank[b] + is_near;
    counts[0] = n;
    counts[1] = nr_bricks - n;
  }
  if (is_near) {
    if (lane == 0) list[rank[b]] = (int32_t)b;
    return;
  }
  const int k = (int)(b % g.bz) * SDF_BRICK + (lane & 3), j = (int)((b / g.bz) % g.by) * SDF_BRICK + ((lane >> 2) & 3);
  const int i = (int)(b / ((long long)g.bz * g.by)) * SDF_BRICK + (lane >> 4);
  if (i < g.nx && j < g.ny && k < g.nz) out[((long long)i * g.ny + j) * g.nz + k] = copysignf(band, centre_dist[b]);
}

// A wave per brick of the list (of every brick without one), a lane per lattice point; points beyond n are masked.
template <int STACK, bool BOUNDS>
__global__ __launch_bounds__(TRACE_BLOCK) void sdf_grid_kernel(
    const uint4* __restrict__ qnodes, const float4* __restrict__ tris, Roots roots, Frames frames,
    const float* __restrict__ table, long long base, Lattice g, const int32_t* __restrict__ list, float band,
    float* __restrict__ out) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  __shared__ float s_bound[BOUNDS ? STACK : 1][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const long long b = list ? list[blockIdx.x] : blockIdx.x;
  const int k = (int)(b % g.bz) * SDF_BRICK + (lane & 3), j = (int)((b / g.bz) % g.by) * SDF_BRICK + ((lane >> 2) & 3);
  const int i = (int)(b / ((long long)g.bz * g.by)) * SDF_BRICK + (lane >> 4);
  const bool alive = i < g.nx && j < g.ny && k < g.nz;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (alive) px = g.x[i], py = g.y[j], pz = g.z[k];
  const QPoint q = closest_qpoint(frames.f[0], px, py, pz);
  Closest best = no_closest();
  closest_walk<STACK, BOUNDS>(qnodes, tris, q, px, py, pz, alive ? roots.root[0] : TRACE_EMPTY, best, s_node, s_bound,
                              lane);
  if (!alive) return;
  const float d = signed_distance(tris, table, base, best, px, py, pz);
  out[((long long)i * g.ny + j) * g.nz + k] = fminf(fmaxf(d, -band), band);
}

struct GridLayout {
  size_t near, rank, list, centre, counts, tmp, tmp_bytes, total;
};

int grid_layout(long long nr_bricks, GridLayout* l) {
  mt::TmpCounts c = {};
  c.xscan32 = (size_t)nr_bricks;
  MT_TRY(mt::tmp_bytes(c, &l->tmp_bytes));
  mt::Bump b;
  l->near = b.take(4 * (size_t)nr_bricks);
  l->rank = b.take(4 * (size_t)nr_bricks);
  l->list = b.take(4 * (size_t)nr_bricks);
  l->centre = b.take(4 * (size_t)nr_bricks);
  l->counts = b.take(16);
  l->tmp = b.take(l->tmp_bytes);
  l->total = b.o;
  return VSA_OK;
}

// VSA_OK with *nr_bricks, or the status of a lattice no launch can take.
int check_lattice(int nx, int ny, int nz, long long* nr_bricks) {
  if (nx < 1 || ny < 1 || nz < 1) return VSA_ERR_ARG;
  const long long bx = vsa_div_up(nx, SDF_BRICK), by = vsa_div_up(ny, SDF_BRICK), bz = vsa_div_up(nz, SDF_BRICK);
  if (bx * by > MAX_GRID || bx * by * bz > MAX_GRID) return VSA_ERR_UNSUPPORTED;
  *nr_bricks = bx * by * bz;
  return VSA_OK;
}

}  // namespace

extern "C" long long vsa_mesh_pseudonormals_workspace_bytes(long long nr_verts, long long nr_faces) {
  if (const int rc = mt::check_vf(nr_verts, nr_faces)) return rc;
  PnLayout l;
  const int rc = pn_layout(nr_verts, nr_faces, &l);
  if (rc != VSA_OK) return mt::abi_status(rc);
  return (long long)l.total;
}

extern "C" int vsa_mesh_pseudonormals(const float* vertices, long long nr_verts, const int32_t* faces,
                                      long long nr_faces, void* workspace, long long workspace_bytes, float* table,
                                      void* stream) {
  if (!vertices || !faces || !workspace || !table) return VSA_ERR_ARG;
  if (const int rc = mt::check_vf(nr_verts, nr_faces)) return rc;
  const long long V = nr_verts, F = nr_faces, n3 = 3 * F;
  PnLayout l;
  MT_TRY(mt::abi_status(pn_layout(V, F, &l)));
  if (workspace_bytes < (long long)l.total) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  const mt::Tmp tmp = {ws + l.tmp, l.tmp_bytes};
  const int s = mt::bits_of(V);
  double* fn = mt::at<double>(ws, l.fn);
  float* nv = mt::at<float>(ws, l.nv);
  hipLaunchKernelGGL(pn_face_kernel, mt::grid(F), dim3(MT_BLOCK), 0, st, vertices, faces, F, fn, table);
  MT_LAUNCHED();
  uint32_t* vin = mt::at<uint32_t>(ws, l.va);
  uint32_t* vff = mt::at<uint32_t>(ws, l.vb);
  int32_t* vstart = mt::at<int32_t>(ws, l.vstart);
  int32_t* vend = mt::at<int32_t>(ws, l.vend);
  MT_TRY(mt::vertex_rings(faces, F, V, s, mt::at<uint32_t>(ws, l.A), mt::at<uint32_t>(ws, l.B), vin, vff, vstart, vend,
                          tmp, st));
  hipLaunchKernelGGL(pn_vertex_kernel, mt::grid(V), dim3(MT_BLOCK), 0, st, vertices, faces, fn, vff, vstart, vend, V, nv);
  MT_LAUNCHED();
  hipLaunchKernelGGL(pn_corner_kernel, mt::grid(n3), dim3(MT_BLOCK), 0, st, faces, n3, nv, table);
  MT_LAUNCHED();
  mt::u64* sorted = mt::at<mt::u64>(ws, l.B);
  uint32_t* slot = vff;                                       // (the rings are read: their buffer takes the slots)
  MT_TRY(mt::sorted_edges(faces, F, s, mt::at<mt::u64>(ws, l.A), sorted, vin, slot, tmp, st));
  hipLaunchKernelGGL(pn_edge_kernel, mt::grid(n3), dim3(MT_BLOCK), 0, st, sorted, slot, n3, fn, table);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_signed_distance_q(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                                     const float* mesh_frames, int nr_meshes, int max_depth, const float* table,
                                     const long long* table_face_base, const float* points, long long nr_points,
                                     float* dist, int32_t* slot, float* bary, void* stream) {
  if (const int rc = check_qtree(qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth, VSA_ERR_ARG)) return rc;
  if (!table || !table_face_base || !points || !dist || !slot || nr_points < 1) return VSA_ERR_ARG;
  TableBase base = {};
  for (int k = 0; k < nr_meshes; ++k) {
    if (table_face_base[k] < 0) return VSA_ERR_ARG;
    base.face[k] = table_face_base[k];
  }
  const long long waves = (nr_points + TRACE_BLOCK - 1) / TRACE_BLOCK;
  if (waves > MAX_GRID) return VSA_ERR_UNSUPPORTED;
  const QTree t = make_qtree(qnodes, tris, mesh_roots, mesh_frames, nr_meshes);
  const dim3 grid((unsigned)waves, nr_meshes), block(TRACE_BLOCK);
  with_stack(max_depth, [&](auto sk) {
    with_flag(closest_walk_bounds(max_depth), [&](auto bd) {
      hipLaunchKernelGGL((signed_distance_kernel<decltype(sk)::value, decltype(bd)::value>), grid, block, 0,
                         (hipStream_t)stream, t.qnodes, t.tris, t.roots, t.frames, table, base, points, nr_points, dist,
                         slot, bary);
    });
  });
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" long long vsa_mesh_sdf_grid_workspace_bytes(int nx, int ny, int nz) {
  long long nr_bricks = 0;
  if (const int rc = check_lattice(nx, ny, nz, &nr_bricks)) return rc;
  GridLayout l;
  const int rc = grid_layout(nr_bricks, &l);
  if (rc != VSA_OK) return mt::abi_status(rc);
  return (long long)l.total;
}

extern "C" int vsa_mesh_sdf_grid(const uint32_t* qnodes, const float* tris, int root, const float* frame, int max_depth,
                                 const float* table, long long table_face_base, const float* x, const float* y,
                                 const float* z, int nx, int ny, int nz, float band, float* grid, void* workspace,
                                 long long workspace_bytes, long long* brick_counts, void* stream) {
  if (const int rc = check_qtree(qnodes, tris, &root, frame, 1, max_depth, VSA_ERR_ARG)) return rc;
  if (!table || !x || !y || !z || !grid || !brick_counts || root < 0 || table_face_base < 0) return VSA_ERR_ARG;
  if (!(band > 0.0f)) return VSA_ERR_ARG;                       // zero, negative or NaN
  long long nr_bricks = 0;
  if (const int rc = check_lattice(nx, ny, nz, &nr_bricks)) return rc;
  const bool banded = band < INFINITY;
  if (banded && !workspace) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const QTree t = make_qtree(qnodes, tris, &root, frame, 1);
  const Lattice g = {x, y, z, nx, ny, nz, vsa_div_up(nx, SDF_BRICK), vsa_div_up(ny, SDF_BRICK), vsa_div_up(nz, SDF_BRICK)};
  const int32_t* list = nullptr;
  brick_counts[0] = nr_bricks, brick_counts[1] = 0;
  if (banded) {
    GridLayout l;
    MT_TRY(mt::abi_status(grid_layout(nr_bricks, &l)));
    if (workspace_bytes < (long long)l.total) return VSA_ERR_ARG;
    char* ws = static_cast<char*>(workspace);
    int32_t* near = mt::at<int32_t>(ws, l.near);
    int32_t* rank = mt::at<int32_t>(ws, l.rank);
    float* centre = mt::at<float>(ws, l.centre);
    long long* counts = mt::at<long long>(ws, l.counts);
    const unsigned waves = (unsigned)((nr_bricks + TRACE_BLOCK - 1) / TRACE_BLOCK);
    with_stack(max_depth, [&](auto sk) {
      with_flag(closest_walk_bounds(max_depth), [&](auto bd) {
        hipLaunchKernelGGL((brick_classify_kernel<decltype(sk)::value, decltype(bd)::value>), dim3(waves),
                           dim3(TRACE_BLOCK), 0, st, t.qnodes, t.tris, t.roots, t.frames, table, table_face_base, g,
                           nr_bricks, band, near, centre);
      });
    });
    MT_LAUNCHED();
    MT_TRY(mt::exclusive_scan({ws + l.tmp, l.tmp_bytes}, near, rank, (size_t)nr_bricks, st));
    const unsigned blocks = (unsigned)((nr_bricks + FILL_BLOCK / VSA_WAVE - 1) / (FILL_BLOCK / VSA_WAVE));
    hipLaunchKernelGGL(brick_fill_kernel, dim3(blocks), dim3(FILL_BLOCK), 0, st, g, nr_bricks, band, near, rank, centre,
                       mt::at<int32_t>(ws, l.list), grid, counts);
    MT_LAUNCHED();
    MT_TRY(mt::read_counters(st, counts, brick_counts, 2));     // the one blocking read: the second pass's size
    list = mt::at<int32_t>(ws, l.list);
  }
  if (brick_counts[0] < 1) return VSA_OK;
  with_stack(max_depth, [&](auto sk) {
    with_flag(closest_walk_bounds(max_depth), [&](auto bd) {
      hipLaunchKernelGGL((sdf_grid_kernel<decltype(sk)::value, decltype(bd)::value>), dim3((unsigned)brick_counts[0]),
                         dim3(TRACE_BLOCK), 0, st, t.qnodes, t.tris, t.roots, t.frames, table, table_face_base, g, list,
                         band, grid);
    });
  });
  VSA_RETURN_LAUNCH_STATUS();
}
