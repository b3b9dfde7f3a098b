// A sign for meshes that are not closed: the generalised winding number (Jacobson et al. 2013) with the far field of
// Barill et al. 2018 at order 0.  (The reference has no such stage: the rule is this library's own --
// include/volsurfs_hip.h "Mesh winding number", DESIGN §31: the exact sum is restated in tests/mesh_sdf_restated.py,
// unpinned.)
//
// vsa_mesh_winding_moments: per subtree of the q16 trees N = sum 1/2 e1 x e2, the area-weighted centroid p and a radius
//   r about p that holds every vertex of the subtree: one entry per child slot of every inner node and one per mesh
//   root.  A leaf has no node of its own, so a lane per child slot starts at the leaves and climbs through parent
//   pointers; at an inner node an integer arrival counter lets the second arriver combine child 0 then child 1 (fp64
//   sums, stored once as fp32).  Nobody waits for anybody; no float atomics: the same bytes on every call.
// vsa_winding_number_q: w for N points x K meshes (winding_walk.h), one query per lane.
// vsa_signed_distance_w_q: vsa_closest_point_q's outputs with the sign from w: negative iff w > 1/2.
// vsa_mesh_sdf_grid_w: that field on a lattice, clamped to a band.  Bricks are classified on the unsigned distance at
//   their centre as in vsa_mesh_sdf_grid; a far brick skips the closest-point walk but still takes w at every one of
//   its points: w crosses 1/2 on the membrane that closes a hole, away from the surface.
// vsa_mesh_edge_census: boundary, non-manifold and inconsistently wound edges from the sorted edge keys.
#include "mesh_topology.h"
#include "winding_walk.h"

namespace {

constexpr long long MAX_GRID = 0x7fffffffll;
constexpr int SDF_BRICK = 4;                  // a wave: SDF_BRICK^3 = 64 lattice points (vsa_mesh_sdf_grid's brick)
constexpr int WN_ACC = 7;                     // fp64 per entry while building: N.xyz, sum area * centroid .xyz, sum area

// ---- moments

struct Acc {
  double n[3], s[3], a;
};

__device__ __forceinline__ void store_acc(double* acc, long long e, const Acc& v) {
  double* o = acc + WN_ACC * e;
  o[0] = v.n[0], o[1] = v.n[1], o[2] = v.n[2], o[3] = v.s[0], o[4] = v.s[1], o[5] = v.s[2], o[6] = v.a;
}

__device__ __forceinline__ Acc load_acc(const double* acc, long long e) {
  const double* o = acc + WN_ACC * e;
  return {{o[0], o[1], o[2]}, {o[3], o[4], o[5]}, o[6]};
}

// r as stored: rounded up, and a millionth larger, so that it also holds the vertices as the walk's fp32 forms them.
__device__ __forceinline__ float radius_up(double r) { return __double2float_ru(r * (1.0 + 1e-6)); }

__device__ __forceinline__ double dist_d(const float p[3], double x, double y, double z) {
  const double dx = x - (double)p[0], dy = y - (double)p[1], dz = z - (double)p[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

__device__ __forceinline__ void store_entry(float* moments, long long e, const Acc& v, const float p[3], float r) {
  float4* o = reinterpret_cast<float4*>(moments + WN_ENTRY_FLOATS * e);
  o[0] = make_float4((float)v.n[0], (float)v.n[1], (float)v.n[2], r);
  o[1] = make_float4(p[0], p[1], p[2], 0.0f);
}

// The centroid as stored: sum area * centroid / sum area, or `fallback` for a subtree without area.
__device__ __forceinline__ void centroid_of(const Acc& v, const float fallback[3], float p[3]) {
  const bool ok = v.a > 0.0 && v.a < INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = ok ? (float)(v.s[k] / v.a) : fallback[k];
}

// parent[child] = the entry (2 n + c) that names the inner node `child`.
__global__ __launch_bounds__(MT_BLOCK) void wn_parent_kernel(const uint32_t* __restrict__ words, long long nr_nodes,
                                                             int32_t* __restrict__ parent) {
  const long long e = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (e >= 2 * nr_nodes) return;
  const int word = (int)words[8 * (e >> 1) + 6 + (e & 1)];
  if (word >= 0 && word != TRACE_EMPTY && word < nr_nodes) parent[word] = (int32_t)e;
}

// parent[root of mesh m] = -1 - m.
__global__ void wn_roots_kernel(Roots roots, int nr_meshes, long long nr_nodes, int32_t* __restrict__ parent) {
  const int m = threadIdx.x;
  if (m < nr_meshes && roots.root[m] >= 0 && roots.root[m] < nr_nodes) parent[roots.root[m]] = -1 - m;
}

// A lane per child slot.  A slot that names an inner node has nothing to start.  A leaf sums its triangles in slot
// order, a missing child is a zero entry; both then arrive at their node.  The first arriver leaves; the second, after
// a device-scope fence, reads both children's sums, writes the node's own entry (into the slot that names the node, or
// the mesh's root entry) and arrives one level up.  (A counter answers 1 once: no node is combined twice.)  An inner
// subtree's r is the composed bound, the largest |p - p_c| + r_c over its children.
__global__ __launch_bounds__(MT_BLOCK) void wn_moments_kernel(const uint32_t* __restrict__ words,
                                                              const float4* __restrict__ tris, long long nr_nodes,
                                                              long long nr_tris, int nr_meshes,
                                                              const int32_t* parent, int* arrived, double* acc,
                                                              float* moments) {
  const long long e0 = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (e0 >= 2 * nr_nodes) return;
  const int word = (int)words[8 * (e0 >> 1) + 6 + (e0 & 1)];
  if (word >= 0 && word != TRACE_EMPTY) return;
  Acc v = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0};
  float p[3] = {0.f, 0.f, 0.f};
  float r = 0.0f;
  const int code = ~word;
  const long long begin = code >> 4;
  const int cnt = word == TRACE_EMPTY ? 0 : (code & 15);
  if (cnt > 0 && begin + cnt <= nr_tris) {
    for (int i = 0; i < cnt; ++i) {
      const float4 v0 = tris[3 * (begin + i)], e1 = tris[3 * (begin + i) + 1], e2 = tris[3 * (begin + i) + 2];
      const double ax = e1.x, ay = e1.y, az = e1.z, bx = e2.x, by = e2.y, bz = e2.z;
      const double nx = 0.5 * (ay * bz - az * by), ny = 0.5 * (az * bx - ax * bz), nz = 0.5 * (ax * by - ay * bx);
      const double area = sqrt((nx * nx + ny * ny) + nz * nz);
      v.n[0] += nx, v.n[1] += ny, v.n[2] += nz;
      if (area > 0.0 && area < INFINITY) {
        v.s[0] += area * ((double)v0.x + (ax + bx) / 3.0);
        v.s[1] += area * ((double)v0.y + (ay + by) / 3.0);
        v.s[2] += area * ((double)v0.z + (az + bz) / 3.0);
        v.a += area;
      }
    }
    const float4 f0 = tris[3 * begin];
    const float fallback[3] = {f0.x, f0.y, f0.z};
    centroid_of(v, fallback, p);
    double far = 0.0;
    for (int i = 0; i < cnt; ++i) {
      const float4 v0 = tris[3 * (begin + i)], e1 = tris[3 * (begin + i) + 1], e2 = tris[3 * (begin + i) + 2];
      far = fmax(far, dist_d(p, v0.x, v0.y, v0.z));
      far = fmax(far, dist_d(p, (double)v0.x + (double)e1.x, (double)v0.y + (double)e1.y, (double)v0.z + (double)e1.z));
      far = fmax(far, dist_d(p, (double)v0.x + (double)e2.x, (double)v0.y + (double)e2.y, (double)v0.z + (double)e2.z));
    }
    r = radius_up(far);
  }
  store_acc(acc, e0, v);
  store_entry(moments, e0, v, p, r);

  long long node = e0 >> 1;
  while (true) {
    __threadfence();
    if (atomicAdd(&arrived[node], 1) != 1) return;
    __threadfence();
    const int up = parent[node];
    const long long dst = up >= 0 ? (long long)up : 2 * nr_nodes + (-1 - (long long)up);
    if (dst >= 2 * nr_nodes + nr_meshes) return;            // (a node nobody names and no root: not part of a tree)
    const Acc c0 = load_acc(acc, 2 * node), c1 = load_acc(acc, 2 * node + 1);
    Acc s;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.n[k] = c0.n[k] + c1.n[k], s.s[k] = c0.s[k] + c1.s[k];
    s.a = c0.a + c1.a;
    const float4* ch = reinterpret_cast<const float4*>(moments + WN_ENTRY_FLOATS * 2 * node);
    const float4 m00 = ch[0], m01 = ch[1], m10 = ch[2], m11 = ch[3];
    const bool has0 = (int)words[8 * node + 6] != TRACE_EMPTY, has1 = (int)words[8 * node + 7] != TRACE_EMPTY;
    const float fallback[3] = {has0 ? m01.x : m11.x, has0 ? m01.y : m11.y, has0 ? m01.z : m11.z};
    float pc[3];
    centroid_of(s, fallback, pc);
    double far = 0.0;
    if (has0) far = fmax(far, dist_d(pc, m01.x, m01.y, m01.z) + (double)m00.w);
    if (has1) far = fmax(far, dist_d(pc, m11.x, m11.y, m11.z) + (double)m10.w);
    store_acc(acc, dst, s);
    store_entry(moments, dst, s, pc, radius_up(far));
    if (up < 0) return;
    node = up >> 1;
  }
}

struct MomentsLayout {
  size_t acc, parent, arrived, total;
};

MomentsLayout moments_layout(long long nr_nodes, int nr_meshes) {
  MomentsLayout l;
  mt::Bump b;
  l.acc = b.take(8 * (size_t)WN_ACC * (size_t)(2 * nr_nodes + nr_meshes));
  l.parent = b.take(4 * (size_t)nr_nodes);
  l.arrived = b.take(4 * (size_t)nr_nodes);
  l.total = b.o;
  return l;
}

int check_moments_sizes(long long nr_nodes, int nr_meshes) {
  if (nr_nodes < 1 || nr_meshes < 1 || nr_meshes > VSA_MAX_SHELLS) return VSA_ERR_ARG;
  if (2 * nr_nodes + nr_meshes > 0x7ffffff0ll) return VSA_ERR_UNSUPPORTED;      // an entry index is an int
  return VSA_OK;
}

// ---- queries

struct MomentRoots {
  long long entry[VSA_MAX_SHELLS];
};

template <int STACK, bool COUNT>
__global__ __launch_bounds__(TRACE_BLOCK) void winding_number_kernel(
    const uint4* __restrict__ qnodes, const float4* __restrict__ tris, const float4* __restrict__ moments, Roots roots,
    MomentRoots mroots, float beta, const float* __restrict__ points, long long nr_points, float* __restrict__ w,
    unsigned long long* __restrict__ counters) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const int mesh = blockIdx.y;
  const long long i = (long long)blockIdx.x * TRACE_BLOCK + lane;
  const bool alive = i < nr_points;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (alive) px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
  int visits = 0, terms = 0;
  const float wn = winding_walk<STACK, COUNT>(qnodes, tris, moments, alive ? roots.root[mesh] : TRACE_EMPTY,
                                              mroots.entry[mesh], px, py, pz, beta, s_node, lane, &visits, &terms);
  if constexpr (COUNT) {
    atomicAdd(&counters[0], (unsigned long long)visits);
    atomicAdd(&counters[1], (unsigned long long)terms);
    if (alive) atomicAdd(&counters[2], 1ull);
    return;
  }
  if (alive) w[(long long)mesh * nr_points + i] = wn;
}

template <int STACK, bool BOUNDS>
__global__ __launch_bounds__(TRACE_BLOCK) void signed_distance_w_kernel(
    const uint4* __restrict__ qnodes, const float4* __restrict__ tris, Roots roots, Frames frames,
    const float4* __restrict__ moments, MomentRoots mroots, float beta, const float* __restrict__ points,
    long long nr_points, float* __restrict__ dist, int* __restrict__ slot, float* __restrict__ bary) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  __shared__ float s_bound[BOUNDS ? STACK : 1][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const int mesh = blockIdx.y;
  const long long i = (long long)blockIdx.x * TRACE_BLOCK + lane;
  const bool alive = i < nr_points;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (alive) px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
  const int root = alive ? roots.root[mesh] : TRACE_EMPTY;
  const QPoint q = closest_qpoint(frames.f[mesh], px, py, pz);
  Closest best = no_closest();
  closest_walk<STACK, BOUNDS>(qnodes, tris, q, px, py, pz, root, best, s_node, s_bound, lane);
  const float wn = winding_walk<STACK>(qnodes, tris, moments, root, mroots.entry[mesh], px, py, pz, beta, s_node, lane);
  if (!alive) return;
  const long long o = (long long)mesh * nr_points + i;
  dist[o] = signed_by_winding(best, wn);
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

// One lane per brick: the unsigned distance d_c at the brick's centre and the brick's radius rho, as
// vsa_mesh_sdf_grid's classification forms them; near[b] = 0 when d_c > band + (4/3) rho.  counts[0] += the near
// bricks of the wave (an integer atomic).
template <int STACK, bool BOUNDS>
__global__ __launch_bounds__(TRACE_BLOCK) void brick_classify_w_kernel(
    const uint4* __restrict__ qnodes, const float4* __restrict__ tris, Roots roots, Frames frames, Lattice g,
    long long nr_bricks, float band, int32_t* __restrict__ near, unsigned long long* __restrict__ counts) {
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
  const float rho = sqrtf((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]);
  const bool is_near = alive && !(sqrtf(best.d2) > band + (4.0f / 3.0f) * rho);     // (a NaN anywhere: near)
  if (alive) near[b] = is_near ? 1 : 0;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(is_near);
  if (lane == 0 && m) atomicAdd(&counts[0], (unsigned long long)__builtin_popcountll(m));
}

// A wave per brick, a lane per lattice point; points beyond n are masked.  A near brick (every brick without `near`)
// walks the closest point and w; a far one walks w alone and writes -band or +band.
template <int STACK, bool BOUNDS>
__global__ __launch_bounds__(TRACE_BLOCK) void sdf_grid_w_kernel(
    const uint4* __restrict__ qnodes, const float4* __restrict__ tris, Roots roots, Frames frames,
    const float4* __restrict__ moments, long long root_entry, float beta, Lattice g, const int32_t* __restrict__ near,
    float band, float* __restrict__ out) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  __shared__ float s_bound[BOUNDS ? STACK : 1][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const long long b = blockIdx.x;
  const int k = (int)(b % g.bz) * SDF_BRICK + (lane & 3), j = (int)((b / g.bz) % g.by) * SDF_BRICK + ((lane >> 2) & 3);
  const int i = (int)(b / ((long long)g.bz * g.by)) * SDF_BRICK + (lane >> 4);
  const bool alive = i < g.nx && j < g.ny && k < g.nz;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (alive) px = g.x[i], py = g.y[j], pz = g.z[k];
  const int root = alive ? roots.root[0] : TRACE_EMPTY;
  const bool is_near = near ? near[b] != 0 : true;                  // (the same for the whole wave)
  Closest best = no_closest();
  if (is_near) {
    const QPoint q = closest_qpoint(frames.f[0], px, py, pz);
    closest_walk<STACK, BOUNDS>(qnodes, tris, q, px, py, pz, root, best, s_node, s_bound, lane);
  }
  const float wn = winding_walk<STACK>(qnodes, tris, moments, root, root_entry, px, py, pz, beta, s_node, lane);
  if (!alive) return;
  const float d = is_near ? fminf(fmaxf(signed_by_winding(best, wn), -band), band) : (wn > 0.5f ? -band : band);
  out[((long long)i * g.ny + j) * g.nz + k] = d;
}

struct GridLayout {
  size_t near, counts, total;
};

GridLayout grid_layout(long long nr_bricks) {
  GridLayout l;
  mt::Bump b;
  l.near = b.take(4 * (size_t)nr_bricks);
  l.counts = b.take(16);
  l.total = b.o;
  return l;
}

// VSA_OK with *nr_bricks, or the status of a lattice no launch can take.
int check_lattice(int nx, int ny, int nz, long long* nr_bricks) {
  if (nx < 1 || ny < 1 || nz < 1) return VSA_ERR_ARG;
  const long long bx = vsa_div_up(nx, SDF_BRICK), by = vsa_div_up(ny, SDF_BRICK), bz = vsa_div_up(nz, SDF_BRICK);
  if (bx * by > MAX_GRID || bx * by * bz > MAX_GRID) return VSA_ERR_UNSUPPORTED;
  *nr_bricks = bx * by * bz;
  return VSA_OK;
}

// ---- census

// live[f] = the face has a positive finite area (fp64 on the fp32 vertices: vsa_mesh_pseudonormals' rule).
__global__ __launch_bounds__(MT_BLOCK) void census_live_kernel(const float* __restrict__ P,
                                                               const int32_t* __restrict__ faces, long long F,
                                                               uint8_t* __restrict__ live) {
  const long long f = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (f >= F) return;
  const long long i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  const double ax = (double)P[3 * i1] - (double)P[3 * i0], ay = (double)P[3 * i1 + 1] - (double)P[3 * i0 + 1],
               az = (double)P[3 * i1 + 2] - (double)P[3 * i0 + 2];
  const double bx = (double)P[3 * i2] - (double)P[3 * i0], by = (double)P[3 * i2 + 1] - (double)P[3 * i0 + 1],
               bz = (double)P[3 * i2 + 2] - (double)P[3 * i0 + 2];
  const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  live[f] = len > 0.0 && len < INFINITY ? 1 : 0;
}

// The lane at the start of a run of equal keys counts the run's live faces: one -> a boundary edge, more than two -> a
// non-manifold one, two whose corners leave the same vertex -> the two faces traverse the edge in the same direction.
__global__ __launch_bounds__(MT_BLOCK) void census_kernel(const mt::u64* __restrict__ sorted,
                                                          const uint32_t* __restrict__ slot, long long n3,
                                                          const int32_t* __restrict__ faces,
                                                          const uint8_t* __restrict__ live,
                                                          unsigned long long* __restrict__ counts) {
  const long long j = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (j >= n3) return;
  const mt::u64 key = sorted[j];
  if (j > 0 && sorted[j - 1] == key) return;
  int n = 0, from[2] = {0, 0};
  for (long long k = j; k < n3 && sorted[k] == key; ++k) {
    const long long i = slot[k];
    if (!live[i / 3]) continue;
    if (n < 2) from[n] = faces[i];
    ++n;
  }
  if (n == 1) atomicAdd(&counts[0], 1ull);
  else if (n > 2) atomicAdd(&counts[1], 1ull);
  else if (n == 2 && from[0] == from[1]) atomicAdd(&counts[2], 1ull);
}

struct CensusLayout {
  size_t keys, sorted, vals, slot, live, counts, tmp, tmp_bytes, total;
};

int census_layout(long long F, CensusLayout* l) {
  mt::TmpCounts c = {};
  c.pairs64 = 3 * (size_t)F;
  MT_TRY(mt::tmp_bytes(c, &l->tmp_bytes));
  mt::Bump b;
  l->keys = b.take(24 * (size_t)F);
  l->sorted = b.take(24 * (size_t)F);
  l->vals = b.take(12 * (size_t)F);
  l->slot = b.take(12 * (size_t)F);
  l->live = b.take((size_t)F);
  l->counts = b.take(24);
  l->tmp = b.take(l->tmp_bytes);
  l->total = b.o;
  return VSA_OK;
}

// The tree arguments of the w queries (no frames: the boxes are not read) and the table's.
int check_wtree(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots, int nr_meshes, int max_depth,
                const float* moments, const long long* moment_roots, float beta) {
  if (!qnodes || !tris || !mesh_roots || !moments || !moment_roots) return VSA_ERR_ARG;
  if (nr_meshes < 1 || nr_meshes > VSA_MAX_SHELLS || max_depth >= TRACE_STACK) return VSA_ERR_ARG;
  if (!(beta > 1.0f)) return VSA_ERR_ARG;                         // <= 1 or NaN
  for (int k = 0; k < nr_meshes; ++k)
    if (moment_roots[k] < 0) return VSA_ERR_ARG;
  return VSA_OK;
}

MomentRoots make_moment_roots(const long long* moment_roots, int nr_meshes) {
  MomentRoots r = {};
  for (int k = 0; k < nr_meshes; ++k) r.entry[k] = moment_roots[k];
  return r;
}

int winding_launch(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots, int nr_meshes, int max_depth,
                   const float* moments, const long long* moment_roots, float beta, const float* points,
                   long long nr_points, float* w, long long* counters, void* stream) {
  if (const int rc = check_wtree(qnodes, tris, mesh_roots, nr_meshes, max_depth, moments, moment_roots, beta)) return rc;
  if (!points || nr_points < 1 || (counters ? false : !w)) return VSA_ERR_ARG;
  const long long waves = (nr_points + TRACE_BLOCK - 1) / TRACE_BLOCK;
  if (waves > MAX_GRID) return VSA_ERR_UNSUPPORTED;
  const Roots roots = make_roots(mesh_roots, nr_meshes);
  const MomentRoots mroots = make_moment_roots(moment_roots, nr_meshes);
  const dim3 grid((unsigned)waves, nr_meshes), block(TRACE_BLOCK);
  if (counters) VSA_HIP_TRY(hipMemsetAsync(counters, 0, 3 * sizeof(long long), (hipStream_t)stream));
  with_stack(max_depth, [&](auto sk) {
    with_flag(counters != nullptr, [&](auto cn) {
      hipLaunchKernelGGL((winding_number_kernel<decltype(sk)::value, decltype(cn)::value>), grid, block, 0,
                         (hipStream_t)stream, reinterpret_cast<const uint4*>(qnodes),
                         reinterpret_cast<const float4*>(tris), reinterpret_cast<const float4*>(moments), roots, mroots,
                         beta, points, nr_points, w, reinterpret_cast<unsigned long long*>(counters));
    });
  });
  VSA_RETURN_LAUNCH_STATUS();
}

}  // namespace

extern "C" long long vsa_mesh_winding_moments_workspace_bytes(long long nr_nodes, int nr_meshes) {
  if (const int rc = check_moments_sizes(nr_nodes, nr_meshes)) return rc;
  return (long long)moments_layout(nr_nodes, nr_meshes).total;
}

extern "C" int vsa_mesh_winding_moments(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                                        int nr_meshes, long long nr_nodes, long long nr_tris, void* workspace,
                                        long long workspace_bytes, float* moments, void* stream) {
  if (!qnodes || !tris || !mesh_roots || !workspace || !moments) return VSA_ERR_ARG;
  if (const int rc = check_moments_sizes(nr_nodes, nr_meshes)) return rc;
  if (nr_tris < 1) return VSA_ERR_ARG;
  if (nr_tris > 0x7ffffffll) return VSA_ERR_UNSUPPORTED;             // a leaf code holds 27 bits of the first slot
  for (int k = 0; k < nr_meshes; ++k)
    if (mesh_roots[k] < 0 || mesh_roots[k] >= nr_nodes) return VSA_ERR_ARG;
  const Roots roots = make_roots(mesh_roots, nr_meshes);
  const MomentsLayout l = moments_layout(nr_nodes, nr_meshes);
  if (workspace_bytes < (long long)l.total) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  int32_t* parent = mt::at<int32_t>(ws, l.parent);
  int* arrived = mt::at<int>(ws, l.arrived);
  VSA_HIP_TRY(hipMemsetAsync(parent, 0x80, 4 * (size_t)nr_nodes, st));      // (no parent: far below every root mark)
  VSA_HIP_TRY(hipMemsetAsync(arrived, 0, 4 * (size_t)nr_nodes, st));
  hipLaunchKernelGGL(wn_parent_kernel, mt::grid(2 * nr_nodes), dim3(MT_BLOCK), 0, st, qnodes, nr_nodes, parent);
  MT_LAUNCHED();
  hipLaunchKernelGGL(wn_roots_kernel, dim3(1), dim3(64), 0, st, roots, nr_meshes, nr_nodes, parent);
  MT_LAUNCHED();
  hipLaunchKernelGGL(wn_moments_kernel, mt::grid(2 * nr_nodes), dim3(MT_BLOCK), 0, st, qnodes,
                     reinterpret_cast<const float4*>(tris), nr_nodes, nr_tris, nr_meshes, parent, arrived,
                     mt::at<double>(ws, l.acc), moments);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_winding_number_q(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots, int nr_meshes,
                                    int max_depth, const float* moments, const long long* moment_roots, float beta,
                                    const float* points, long long nr_points, float* w, void* stream) {
  return winding_launch(qnodes, tris, mesh_roots, nr_meshes, max_depth, moments, moment_roots, beta, points, nr_points,
                        w, nullptr, stream);
}

extern "C" int vsa_winding_number_q_stats(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                                          int nr_meshes, int max_depth, const float* moments,
                                          const long long* moment_roots, float beta, const float* points,
                                          long long nr_points, long long* counters, void* stream) {
  if (!counters) return VSA_ERR_ARG;
  return winding_launch(qnodes, tris, mesh_roots, nr_meshes, max_depth, moments, moment_roots, beta, points, nr_points,
                        nullptr, counters, stream);
}

extern "C" int vsa_signed_distance_w_q(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                                       const float* mesh_frames, int nr_meshes, int max_depth, const float* moments,
                                       const long long* moment_roots, float beta, const float* points,
                                       long long nr_points, float* dist, int32_t* slot, float* bary, void* stream) {
  if (const int rc = check_qtree(qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth, VSA_ERR_ARG)) return rc;
  if (const int rc = check_wtree(qnodes, tris, mesh_roots, nr_meshes, max_depth, moments, moment_roots, beta)) return rc;
  if (!points || !dist || !slot || nr_points < 1) return VSA_ERR_ARG;
  const long long waves = (nr_points + TRACE_BLOCK - 1) / TRACE_BLOCK;
  if (waves > MAX_GRID) return VSA_ERR_UNSUPPORTED;
  const QTree t = make_qtree(qnodes, tris, mesh_roots, mesh_frames, nr_meshes);
  const MomentRoots mroots = make_moment_roots(moment_roots, nr_meshes);
  const dim3 grid((unsigned)waves, nr_meshes), block(TRACE_BLOCK);
  with_stack(max_depth, [&](auto sk) {
    with_flag(closest_walk_bounds(max_depth), [&](auto bd) {
      hipLaunchKernelGGL((signed_distance_w_kernel<decltype(sk)::value, decltype(bd)::value>), grid, block, 0,
                         (hipStream_t)stream, t.qnodes, t.tris, t.roots, t.frames,
                         reinterpret_cast<const float4*>(moments), mroots, beta, points, nr_points, dist, slot, bary);
    });
  });
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" long long vsa_mesh_sdf_grid_w_workspace_bytes(int nx, int ny, int nz) {
  long long nr_bricks = 0;
  if (const int rc = check_lattice(nx, ny, nz, &nr_bricks)) return rc;
  return (long long)grid_layout(nr_bricks).total;
}

extern "C" int vsa_mesh_sdf_grid_w(const uint32_t* qnodes, const float* tris, int root, const float* frame,
                                   int max_depth, const float* moments, long long moment_root, float beta,
                                   const float* x, const float* y, const float* z, int nx, int ny, int nz, float band,
                                   float* grid, void* workspace, long long workspace_bytes, long long* brick_counts,
                                   void* stream) {
  if (const int rc = check_qtree(qnodes, tris, &root, frame, 1, max_depth, VSA_ERR_ARG)) return rc;
  if (const int rc = check_wtree(qnodes, tris, &root, 1, max_depth, moments, &moment_root, beta)) return rc;
  if (!x || !y || !z || !grid || !brick_counts || root < 0) return VSA_ERR_ARG;
  if (!(band > 0.0f)) return VSA_ERR_ARG;                       // zero, negative or NaN
  long long nr_bricks = 0;
  if (const int rc = check_lattice(nx, ny, nz, &nr_bricks)) return rc;
  const bool banded = band < INFINITY;
  if (banded && !workspace) return VSA_ERR_ARG;
  const GridLayout l = grid_layout(nr_bricks);
  if (banded && workspace_bytes < (long long)l.total) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const QTree t = make_qtree(qnodes, tris, &root, frame, 1);
  const Lattice g = {x, y, z, nx, ny, nz, vsa_div_up(nx, SDF_BRICK), vsa_div_up(ny, SDF_BRICK), vsa_div_up(nz, SDF_BRICK)};
  const float4* mo = reinterpret_cast<const float4*>(moments);
  const int32_t* near = nullptr;
  long long* counts = nullptr;
  brick_counts[0] = nr_bricks, brick_counts[1] = 0;
  if (banded) {
    char* ws = static_cast<char*>(workspace);
    int32_t* flags = mt::at<int32_t>(ws, l.near);
    counts = mt::at<long long>(ws, l.counts);
    VSA_HIP_TRY(hipMemsetAsync(counts, 0, 16, st));
    const unsigned waves = (unsigned)((nr_bricks + TRACE_BLOCK - 1) / TRACE_BLOCK);
    with_stack(max_depth, [&](auto sk) {
      with_flag(closest_walk_bounds(max_depth), [&](auto bd) {
        hipLaunchKernelGGL((brick_classify_w_kernel<decltype(sk)::value, decltype(bd)::value>), dim3(waves),
                           dim3(TRACE_BLOCK), 0, st, t.qnodes, t.tris, t.roots, t.frames, g, nr_bricks, band, flags,
                           reinterpret_cast<unsigned long long*>(counts));
      });
    });
    MT_LAUNCHED();
    near = flags;
  }
  with_stack(max_depth, [&](auto sk) {
    with_flag(closest_walk_bounds(max_depth), [&](auto bd) {
      hipLaunchKernelGGL((sdf_grid_w_kernel<decltype(sk)::value, decltype(bd)::value>), dim3((unsigned)nr_bricks),
                         dim3(TRACE_BLOCK), 0, st, t.qnodes, t.tris, t.roots, t.frames, mo, moment_root, beta, g, near,
                         band, grid);
    });
  });
  MT_LAUNCHED();
  if (banded) {
    MT_TRY(mt::read_counters(st, counts, brick_counts, 1));      // the one blocking read
    brick_counts[1] = nr_bricks - brick_counts[0];
  }
  return VSA_OK;
}

extern "C" long long vsa_mesh_edge_census_workspace_bytes(long long nr_verts, long long nr_faces) {
  if (const int rc = mt::check_vf(nr_verts, nr_faces)) return rc;
  CensusLayout l;
  const int rc = census_layout(nr_faces, &l);
  if (rc != VSA_OK) return mt::abi_status(rc);
  return (long long)l.total;
}

extern "C" int vsa_mesh_edge_census(const float* vertices, long long nr_verts, const int32_t* faces, long long nr_faces,
                                    void* workspace, long long workspace_bytes, long long* counts, void* stream) {
  if (!vertices || !faces || !workspace || !counts) return VSA_ERR_ARG;
  if (const int rc = mt::check_vf(nr_verts, nr_faces)) return rc;
  const long long F = nr_faces, n3 = 3 * F;
  CensusLayout l;
  MT_TRY(mt::abi_status(census_layout(F, &l)));
  if (workspace_bytes < (long long)l.total) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  const mt::Tmp tmp = {ws + l.tmp, l.tmp_bytes};
  uint8_t* live = mt::at<uint8_t>(ws, l.live);
  long long* dcounts = mt::at<long long>(ws, l.counts);
  mt::u64* sorted = mt::at<mt::u64>(ws, l.sorted);
  uint32_t* slot = mt::at<uint32_t>(ws, l.slot);
  VSA_HIP_TRY(hipMemsetAsync(dcounts, 0, 24, st));
  hipLaunchKernelGGL(census_live_kernel, mt::grid(F), dim3(MT_BLOCK), 0, st, vertices, faces, F, live);
  MT_LAUNCHED();
  MT_TRY(mt::sorted_edges(faces, F, mt::bits_of(nr_verts), mt::at<mt::u64>(ws, l.keys), sorted, mt::at<uint32_t>(ws, l.vals),
                          slot, tmp, st));
  hipLaunchKernelGGL(census_kernel, mt::grid(n3), dim3(MT_BLOCK), 0, st, sorted, slot, n3, faces, live,
                     reinterpret_cast<unsigned long long*>(dcounts));
  MT_LAUNCHED();
  return mt::read_counters(st, dcounts, counts, 3);
}
