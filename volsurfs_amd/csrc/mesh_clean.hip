// Floater removal: connected triangle clusters of a plain mesh and the removals built on them (vsa_mesh_clusters,
// vsa_mesh_filter, vsa_mesh_compact_rows; rules in include/volsurfs_hip.h "Mesh cleaning").
//
// One stream.  Clusters:
//   edges:    the 3F (min, max) edge keys of 2 s bits (s = the bits of V - 1) with their corner slots.
//   sort:     one radix sort of the pairs (rocPRIM).
//   hook:     one lane per sorted slot joins its face with the previous slot's when their keys are equal: chaining
//             neighbours joins every face of an edge, however many there are.  CAS hooks of the larger root under the
//             smaller (mesh_topology.h): a root is its cluster's minimum face, whatever the order.
//   roots:    one lane per face walks to its root without writing.
//   number:   roots flagged and scanned into cluster numbers (ascending minimum face); the face counts by integer
//             atomics, one per wave and cluster.  The host reads C here.
//   areas:    (cluster, face) radix-sorted by cluster (stable: ascending face within a cluster), the fp64 face areas
//             laid out in that order, summed per cluster in chunks of 2048 by a segmented scan of fixed shape, and the
//             chunks of a cluster that spans several added by one wave in a fixed shape.  No float atomics.
// Filter:
//   threshold: the C counts radix-sorted descending; one lane writes max(k-th largest, floor) and the number of
//             clusters at or above it to device memory.
//   mask:     one lane per face: kept by the mask, flags its corners' vertices, and is emitted unless it names a
//             vertex twice and degenerate faces are dropped.
//   compact:  scans of the face and vertex flags; faces renumbered and written in order, vertices written in order,
//             both old -> new maps written.  The host reads the totals once.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mesh_topology.h"

#define MC_BLOCK MT_BLOCK
#define MC_ITEMS 8
#define MC_CHUNK (MC_BLOCK * MC_ITEMS)

// device counters
#define MCT_C 0
#define MCT_THR 1
#define MCT_KEPT 2
#define MCT_VOUT 3
#define MCT_FOUT 4
#define MCT_FMASK 5
#define MCT_N 8

#define MC_STAGES 9
enum { ST_EDGES, ST_SORT, ST_HOOK, ST_ROOTS, ST_NUMBER, ST_AREAS, ST_THRESHOLD, ST_MASK, ST_COMPACT };

using mt::at;
using mt::u64;

// ------------------------------------------------------------------------------------------------ clusters

__global__ __launch_bounds__(MC_BLOCK) void mcl_hook(const u64* __restrict__ sorted, const uint32_t* __restrict__ slot,
                                                    long long n3, int32_t* par) {
  const long long i = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i < 1 || i >= n3 || sorted[i] != sorted[i - 1]) return;
  fu_union(par, (int)(slot[i - 1] / 3), (int)(slot[i] / 3));
}

// cluster[f] = rank[root[f]]; counts[c] += 1 with one atomic per wave and distinct cluster in it (integer sums do not
// depend on the order).
// `cluster` holds the roots on entry (each lane reads and writes its own entry only).
__global__ __launch_bounds__(MC_BLOCK) void mcl_number(const int32_t* __restrict__ flags,
                                                      const int32_t* __restrict__ rank, long long F,
                                                      int32_t* cluster, int32_t* __restrict__ counts,
                                                      long long* __restrict__ ctr) {
  const long long f = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  bool active = f < F;
  int c = 0;
  if (active) {
    c = rank[cluster[f]];
    cluster[f] = c;
    if (f == F - 1) ctr[MCT_C] = rank[f] + flags[f];
  }
  const int lane = threadIdx.x & (VSA_WAVE - 1);
  while (true) {
    const u64 m = __ballot(active);
    if (!m) break;
    const int leader = __ffsll((long long)m) - 1;
    const int lc = __shfl(c, leader, VSA_WAVE);
    const bool same = active && c == lc;
    const u64 sm = __ballot(same);
    if (lane == leader) atomicAdd(counts + lc, (int)__popcll(sm));
    if (same) active = false;
  }
}

__global__ __launch_bounds__(MC_BLOCK) void mcl_sort_pairs(const int32_t* __restrict__ cluster, long long F,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const long long f = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (f >= F) return;
  keys[f] = (uint32_t)cluster[f];
  vals[f] = (uint32_t)f;
}

// 0.5 |(p1 - p0) x (p2 - p0)| in fp64 from the fp32 vertices, no contraction.
__device__ __forceinline__ double mcl_face_area(const float* __restrict__ P, const int32_t* __restrict__ faces,
                                                long long f) {
  const long long a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  const double ax = P[3 * a], ay = P[3 * a + 1], az = P[3 * a + 2];
  const double e1x = (double)P[3 * b] - ax, e1y = (double)P[3 * b + 1] - ay, e1z = (double)P[3 * b + 2] - az;
  const double e2x = (double)P[3 * c] - ax, e2y = (double)P[3 * c + 1] - ay, e2z = (double)P[3 * c + 2] - az;
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  return 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
}

// Sorted position i holds face sface[i] of cluster skey[i].  start[c] = the first position of cluster c.
__global__ __launch_bounds__(MC_BLOCK) void mcl_starts(const uint32_t* __restrict__ skey, long long F,
                                                      int32_t* __restrict__ start) {
  const long long i = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i >= F) return;
  if (i == 0 || skey[i] != skey[i - 1]) start[skey[i]] = (int32_t)i;
}

// One block per chunk of MC_CHUNK sorted positions: the segmented inclusive sum of the areas in a fixed shape (each
// lane adds its MC_ITEMS consecutive items in order, then a Hillis-Steele scan of the lanes' sums in LDS).  A cluster
// that lies inside the chunk gets its area; head[b] = the sum of the chunk's first piece, tail[b] of its last.
__global__ __launch_bounds__(MC_BLOCK) void mcl_area_chunks(const float* __restrict__ P,
                                                           const int32_t* __restrict__ faces,
                                                           const uint32_t* __restrict__ skey,
                                                           const uint32_t* __restrict__ sface, long long F,
                                                           const int32_t* __restrict__ start,
                                                           const int32_t* __restrict__ counts,
                                                           double* __restrict__ areas, double* __restrict__ head,
                                                           double* __restrict__ tail) {
  __shared__ double sv[2][MC_BLOCK];
  __shared__ int sf[2][MC_BLOCK];
  const long long lo = (long long)blockIdx.x * MC_CHUNK;
  const long long hi = lo + MC_CHUNK < F ? lo + MC_CHUNK : F;
  const long long base = lo + (long long)threadIdx.x * MC_ITEMS;
  double run[MC_ITEMS];
  uint32_t key[MC_ITEMS];
  double acc = 0.0;
  int has_start = 0;       // a segment starts inside this lane's items
#pragma unroll
  for (int k = 0; k < MC_ITEMS; ++k) {
    const long long i = base + k;
    run[k] = 0.0;
    key[k] = 0u;
    if (i >= hi) continue;
    key[k] = skey[i];
    const bool st = i == lo || key[k] != skey[i - 1];
    if (st) {
      has_start = 1;
      acc = 0.0;
    }
    acc = acc + mcl_face_area(P, faces, sface[i]);
    run[k] = acc;
  }
  // segmented inclusive scan over the lanes of (acc, has_start): after it, sv = the sum of the open segment up to and
  // including this lane
  int cur = 0;
  sv[0][threadIdx.x] = acc;
  sf[0][threadIdx.x] = has_start;
  __syncthreads();
  for (int d = 1; d < MC_BLOCK; d <<= 1) {
    double v = sv[cur][threadIdx.x];
    int fl = sf[cur][threadIdx.x];
    if ((int)threadIdx.x >= d && !fl) {
      v = sv[cur][threadIdx.x - d] + v;
      fl = sf[cur][threadIdx.x - d];
    }
    sv[cur ^ 1][threadIdx.x] = v;
    sf[cur ^ 1][threadIdx.x] = fl;
    cur ^= 1;
    __syncthreads();
  }
  const double carry = threadIdx.x > 0 ? sv[cur][threadIdx.x - 1] : 0.0;   // the open segment's sum before this lane
  bool seen = false;
#pragma unroll
  for (int k = 0; k < MC_ITEMS; ++k) {
    const long long i = base + k;
    if (i >= hi) continue;
    const bool st = i == lo || key[k] != skey[i - 1];
    seen = seen || st;
    const bool last = i + 1 == hi;
    const bool end = last || skey[i + 1] != key[k];
    if (!end) continue;
    const double sum = seen ? run[k] : carry + run[k];
    const long long s0 = start[key[k]], s1 = s0 + counts[key[k]];
    if (s0 >= lo && s1 <= hi) areas[key[k]] = sum;
    if (key[k] == skey[lo]) head[blockIdx.x] = sum;
    if (last) tail[blockIdx.x] = sum;
  }
}

// A cluster that spans chunks b0 < b1: tail[b0] + (head[b0 + 1] + ... + head[b1]).  One wave per cluster: lane l adds
// head[b0 + 1 + l], head[b0 + 1 + l + 64], ... in ascending order, then a shuffle tree of fixed shape joins the lanes.
__global__ __launch_bounds__(VSA_WAVE) void mcl_area_spans(const int32_t* __restrict__ start,
                                                          const int32_t* __restrict__ counts, long long C,
                                                          const double* __restrict__ head,
                                                          const double* __restrict__ tail,
                                                          double* __restrict__ areas) {
  const long long c = blockIdx.x;
  if (c >= C) return;
  const long long s0 = start[c], s1 = s0 + counts[c];
  const long long b0 = s0 / MC_CHUNK, b1 = (s1 - 1) / MC_CHUNK;
  if (b0 == b1) return;
  double sum = 0.0;
  for (long long b = b0 + 1 + threadIdx.x; b <= b1; b += VSA_WAVE) sum = sum + head[b];
#pragma unroll
  for (int d = VSA_WAVE / 2; d > 0; d >>= 1) sum = sum + __shfl_down(sum, d, VSA_WAVE);
  if (threadIdx.x == 0) areas[c] = tail[b0] + sum;
}

// ------------------------------------------------------------------------------------------------ filter

// sorted: the C counts, descending.  thr = max(sorted[min(k, C) - 1], floor); kept = the counts >= thr.
__global__ void mcl_threshold(const int32_t* __restrict__ sorted, long long k, long long floor_faces,
                              long long* __restrict__ ctr) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long C = ctr[MCT_C];
  const long long kk = k < C ? k : C;
  long long thr = sorted[kk - 1];
  thr = thr > floor_faces ? thr : floor_faces;
  long long lo = 0, hi = C;   // the first index with sorted[i] < thr
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (sorted[mid] >= thr) lo = mid + 1;
    else hi = mid;
  }
  ctr[MCT_THR] = thr;
  ctr[MCT_KEPT] = lo;
}

// mode 0: every face passes; 1: keep_mask[f] != 0; 2: counts[cluster[f]] >= thr.  A passing face flags its vertices
// (every lane stores the same 1); it is emitted unless drop_degenerate and it names a vertex twice.
__global__ __launch_bounds__(MC_BLOCK) void mcl_mask(const int32_t* __restrict__ faces, long long F, int mode,
                                                    const uint8_t* __restrict__ keep_mask,
                                                    const int32_t* __restrict__ cluster,
                                                    const int32_t* __restrict__ counts,
                                                    const long long* __restrict__ ctr, int drop_degenerate,
                                                    int32_t* __restrict__ fflag, int32_t* __restrict__ pflag,
                                                    int32_t* __restrict__ vflag) {
  const long long f = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (f >= F) return;
  bool pass = true;
  if (mode == 1) pass = keep_mask[f] != 0;
  else if (mode == 2) pass = (long long)counts[cluster[f]] >= ctr[MCT_THR];
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (pass && vflag) {
    vflag[a] = 1;
    vflag[b] = 1;
    vflag[c] = 1;
  }
  pflag[f] = pass;
  fflag[f] = pass && !(drop_degenerate && (a == b || b == c || c == a));
}

__global__ __launch_bounds__(MC_BLOCK) void mcl_fill(int32_t* __restrict__ x, long long n, int32_t v) {
  const long long i = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i < n) x[i] = v;
}

// Vertices in order; vrank is the exclusive scan of vflag.
__global__ __launch_bounds__(MC_BLOCK) void mcl_emit_verts(const float* __restrict__ P, long long V,
                                                          const int32_t* __restrict__ vflag,
                                                          const int32_t* __restrict__ vrank,
                                                          float* __restrict__ out_verts, int32_t* __restrict__ vmap,
                                                          long long* __restrict__ ctr) {
  const long long v = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (v >= V) return;
  const int r = vrank[v];
  if (vflag[v]) {
    out_verts[3 * (long long)r] = P[3 * v];
    out_verts[3 * (long long)r + 1] = P[3 * v + 1];
    out_verts[3 * (long long)r + 2] = P[3 * v + 2];
  }
  vmap[v] = vflag[v] ? r : -1;
  if (v == V - 1) ctr[MCT_VOUT] = r + vflag[v];
}

__global__ __launch_bounds__(MC_BLOCK) void mcl_emit_faces(const int32_t* __restrict__ faces, long long F,
                                                          const int32_t* __restrict__ fflag,
                                                          const int32_t* __restrict__ frank,
                                                          const int32_t* __restrict__ pflag,
                                                          const int32_t* __restrict__ vrank,
                                                          int32_t* __restrict__ out_faces, int32_t* __restrict__ fmap,
                                                          long long* __restrict__ ctr) {
  const long long f = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  const bool in = f < F;
  const int r = in ? frank[f] : 0;
  const bool keep = in && fflag[f];
  if (keep) {
    out_faces[3 * (long long)r] = vrank[faces[3 * f]];
    out_faces[3 * (long long)r + 1] = vrank[faces[3 * f + 1]];
    out_faces[3 * (long long)r + 2] = vrank[faces[3 * f + 2]];
  }
  if (in) {
    fmap[f] = keep ? r : -1;
    if (f == F - 1) ctr[MCT_FOUT] = r + fflag[f];
  }
  // the faces that passed the mask, degenerate ones included (one atomic per wave)
  const u64 m = __ballot(in && pflag[f]);
  if ((threadIdx.x & (VSA_WAVE - 1)) == 0 && m)
    atomicAdd((unsigned long long*)(ctr + MCT_FMASK), (unsigned long long)__popcll(m));
}

// out[map[i]] = rows[i] for map[i] >= 0; rows of `words` 32-bit words.
__global__ __launch_bounds__(MC_BLOCK) void mcl_compact_rows(const uint32_t* __restrict__ rows, long long n, int words,
                                                            const int32_t* __restrict__ map,
                                                            uint32_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i >= n * words) return;
  const long long r = i / words;
  const int m = map[r];
  if (m >= 0) out[(long long)m * words + (i - r * words)] = rows[i];
}

// ------------------------------------------------------------------------------------------------ host

struct MclLayout {
  size_t A, B, va, vb, par, cluster, flags, rank, counts, sorted, start, head, tail, pflag, vflag, ctr, tmp, tmp_bytes,
      total;
};

static int mcl_layout(long long V, long long F, MclLayout* l) {
  const size_t v = (size_t)V, f = (size_t)F, n3 = 3 * f, n = f > v ? f : v;
  const size_t chunks = (f + MC_CHUNK - 1) / MC_CHUNK;
  mt::TmpCounts cnt = {};
  cnt.pairs64 = n3;
  cnt.pairs32 = f;
  cnt.keys_desc32 = f;
  cnt.xscan32 = n;
  MT_TRY(mt::tmp_bytes(cnt, &l->tmp_bytes));
  mt::Bump b;
  l->ctr = b.take(8 * MCT_N);
  l->A = b.take(8 * n3);        // edge keys; then the cluster sort's keys and faces (4 x F u32)
  l->B = b.take(8 * n3);        // sorted edge keys
  l->va = b.take(4 * n3);
  l->vb = b.take(4 * n3);
  l->par = b.take(4 * f);
  l->cluster = b.take(4 * f);
  l->flags = b.take(4 * n);     // root flags; then the emitted-face flags
  l->rank = b.take(4 * n);
  l->counts = b.take(4 * f);
  l->sorted = b.take(4 * f);
  l->start = b.take(4 * f);
  l->head = b.take(8 * chunks);
  l->tail = b.take(8 * chunks);
  l->pflag = b.take(4 * f);
  l->vflag = b.take(4 * v);
  l->tmp = b.take(l->tmp_bytes);
  l->total = b.o;
  return VSA_OK;
}

extern "C" long long vsa_mesh_clusters_workspace_bytes(long long nr_verts, long long nr_faces) {
  MclLayout l;
  int rc = mt::check_vf(nr_verts, nr_faces);
  if (rc == VSA_OK) rc = mt::abi_status(mcl_layout(nr_verts, nr_faces, &l));
  return rc != VSA_OK ? rc : (long long)l.total;
}

namespace {

struct Mcl {
  hipStream_t st;
  char* ws;
  MclLayout l;
  mt::Tmp tmp;
  long long V, F, C;
  int s_bits;
  const float* P;
  const int32_t* faces;
  long long* ctr;
  mt::StageTimer timer;
};

// triangle_clusters and counts (the first C written; counts is zeroed up to F); reads C to the host.
int cluster_stages(Mcl& m, int32_t* cluster, int32_t* counts) {
  const long long F = m.F, n3 = 3 * F;
  char* ws = m.ws;
  const MclLayout& l = m.l;
  u64* ek = at<u64>(ws, l.A);
  u64* es = at<u64>(ws, l.B);
  uint32_t* vin = at<uint32_t>(ws, l.va);
  uint32_t* slot = at<uint32_t>(ws, l.vb);
  int32_t* par = at<int32_t>(ws, l.par);
  int32_t* flags = at<int32_t>(ws, l.flags);
  int32_t* rank = at<int32_t>(ws, l.rank);
  VSA_HIP_TRY(hipMemsetAsync(m.ctr, 0, 8 * MCT_N, m.st));
  // (the two halves of mt::sorted_edges, timed apart)
  MT_TRY(m.timer.open());
  MT_TRY(mt::edge_keys(m.faces, F, m.s_bits, ek, vin, m.st));
  MT_TRY(m.timer.close(ST_EDGES));
  MT_TRY(m.timer.open());
  MT_TRY(mt::sort_pairs(m.tmp, ek, es, vin, slot, (size_t)n3, 0, 2 * m.s_bits, m.st));
  MT_TRY(m.timer.close(ST_SORT));
  MT_TRY(m.timer.open());
  MT_TRY(mt::iota(par, F, m.st));
  hipLaunchKernelGGL(mcl_hook, mt::grid(n3), dim3(MC_BLOCK), 0, m.st, es, slot, n3, par);
  MT_LAUNCHED();
  MT_TRY(m.timer.close(ST_HOOK));
  MT_TRY(m.timer.open());
  // the roots go to `cluster` and are replaced by the numbers in place
  MT_TRY(mt::roots(par, F, cluster, flags, m.st));
  MT_TRY(m.timer.close(ST_ROOTS));
  MT_TRY(m.timer.open());
  MT_TRY(mt::exclusive_scan(m.tmp, flags, rank, (size_t)F, m.st));
  VSA_HIP_TRY(hipMemsetAsync(counts, 0, 4 * (size_t)F, m.st));
  hipLaunchKernelGGL(mcl_number, mt::grid(F), dim3(MC_BLOCK), 0, m.st, flags, rank, F, cluster, counts, m.ctr);
  MT_LAUNCHED();
  MT_TRY(mt::read_counters(m.st, m.ctr + MCT_C, &m.C));
  MT_TRY(m.timer.close(ST_NUMBER));
  if (m.C < 1 || m.C > F) return VSA_ERR_UNSUPPORTED;
  return VSA_OK;
}

int area_stage(Mcl& m, const int32_t* cluster, const int32_t* counts, double* areas) {
  const long long F = m.F;
  char* ws = m.ws;
  const MclLayout& l = m.l;
  uint32_t* kin = at<uint32_t>(ws, l.A);
  uint32_t* kout = kin + F;
  uint32_t* fin = kin + 2 * F;
  uint32_t* fout = kin + 3 * F;
  int32_t* start = at<int32_t>(ws, l.start);
  double* head = at<double>(ws, l.head);
  double* tail = at<double>(ws, l.tail);
  MT_TRY(m.timer.open());
  hipLaunchKernelGGL(mcl_sort_pairs, mt::grid(F), dim3(MC_BLOCK), 0, m.st, cluster, F, kin, fin);
  MT_LAUNCHED();
  MT_TRY(mt::sort_pairs(m.tmp, kin, kout, fin, fout, (size_t)F, 0, mt::bits_of(m.C), m.st));
  hipLaunchKernelGGL(mcl_starts, mt::grid(F), dim3(MC_BLOCK), 0, m.st, kout, F, start);
  MT_LAUNCHED();
  const long long chunks = (F + MC_CHUNK - 1) / MC_CHUNK;
  hipLaunchKernelGGL(mcl_area_chunks, dim3((unsigned)chunks), dim3(MC_BLOCK), 0, m.st, m.P, m.faces, kout, fout, F,
                     start, counts, areas, head, tail);
  MT_LAUNCHED();
  hipLaunchKernelGGL(mcl_area_spans, dim3((unsigned)m.C), dim3(VSA_WAVE), 0, m.st, start, counts, m.C, head, tail, areas);
  MT_LAUNCHED();
  MT_TRY(m.timer.close(ST_AREAS));
  return VSA_OK;
}

int setup(Mcl& m, const float* verts, long long V, const int32_t* faces, long long F, void* workspace,
          long long workspace_bytes, float* stage_ms, void* stream) {
  MT_TRY(mt::abi_status(mcl_layout(V, F, &m.l)));
  if (workspace_bytes < (long long)m.l.total) return VSA_ERR_ARG;
  m.st = (hipStream_t)stream;
  m.ws = static_cast<char*>(workspace);
  m.tmp = {m.ws + m.l.tmp, m.l.tmp_bytes};
  m.V = V;
  m.F = F;
  m.C = 0;
  m.P = verts;
  m.faces = faces;
  m.s_bits = mt::bits_of(V);
  m.ctr = at<long long>(m.ws, m.l.ctr);
  return m.timer.create(stage_ms, MC_STAGES, m.st);
}

int run_filter(Mcl& m, int mode, const uint8_t* keep_mask, long long cluster_to_keep, long long min_cluster_faces,
               int drop_unreferenced, int drop_degenerate, float* out_verts, int32_t* out_faces, int32_t* out_vmap,
               int32_t* out_fmap, long long* stats) {
  const long long F = m.F, V = m.V;
  char* ws = m.ws;
  const MclLayout& l = m.l;
  int32_t* cluster = at<int32_t>(ws, l.cluster);
  int32_t* counts = at<int32_t>(ws, l.counts);
  if (mode == 2) {
    MT_TRY(cluster_stages(m, cluster, counts));
    MT_TRY(m.timer.open());
    int32_t* sorted = at<int32_t>(ws, l.sorted);
    MT_TRY(mt::sort_keys_desc(m.tmp, counts, sorted, (size_t)m.C, 0, 32, m.st));
    hipLaunchKernelGGL(mcl_threshold, dim3(1), dim3(1), 0, m.st, sorted, cluster_to_keep, min_cluster_faces, m.ctr);
    MT_LAUNCHED();
    MT_TRY(m.timer.close(ST_THRESHOLD));
  } else {
    VSA_HIP_TRY(hipMemsetAsync(m.ctr, 0, 8 * MCT_N, m.st));
  }
  int32_t* fflag = at<int32_t>(ws, l.flags);
  int32_t* pflag = at<int32_t>(ws, l.pflag);
  int32_t* vflag = at<int32_t>(ws, l.vflag);
  int32_t* rank = at<int32_t>(ws, l.rank);
  MT_TRY(m.timer.open());
  if (drop_unreferenced) {
    VSA_HIP_TRY(hipMemsetAsync(vflag, 0, 4 * (size_t)V, m.st));
  } else {
    hipLaunchKernelGGL(mcl_fill, mt::grid(V), dim3(MC_BLOCK), 0, m.st, vflag, V, 1);
    MT_LAUNCHED();
  }
  hipLaunchKernelGGL(mcl_mask, mt::grid(F), dim3(MC_BLOCK), 0, m.st, m.faces, F, mode, keep_mask, cluster, counts,
                     m.ctr, drop_degenerate, fflag, pflag, drop_unreferenced ? vflag : (int32_t*)nullptr);
  MT_LAUNCHED();
  MT_TRY(m.timer.close(ST_MASK));
  MT_TRY(m.timer.open());
  // vertices first: `rank` holds the vertex ranks while the faces are renumbered, so the face ranks go to `start`
  MT_TRY(mt::exclusive_scan(m.tmp, vflag, rank, (size_t)V, m.st));
  hipLaunchKernelGGL(mcl_emit_verts, mt::grid(V), dim3(MC_BLOCK), 0, m.st, m.P, V, vflag, rank, out_verts, out_vmap,
                     m.ctr);
  MT_LAUNCHED();
  int32_t* frank = at<int32_t>(ws, l.start);
  MT_TRY(mt::exclusive_scan(m.tmp, fflag, frank, (size_t)F, m.st));
  hipLaunchKernelGGL(mcl_emit_faces, mt::grid(F), dim3(MC_BLOCK), 0, m.st, m.faces, F, fflag, frank, pflag, rank,
                     out_faces, out_fmap, m.ctr);
  MT_LAUNCHED();
  long long host[MCT_N];
  MT_TRY(mt::read_counters(m.st, m.ctr, host, MCT_N));
  MT_TRY(m.timer.close(ST_COMPACT));
  stats[0] = host[MCT_VOUT];
  stats[1] = host[MCT_FOUT];
  stats[2] = mode == 2 ? host[MCT_C] : 0;
  stats[3] = mode == 2 ? host[MCT_THR] : 0;
  stats[4] = mode == 2 ? host[MCT_KEPT] : 0;
  stats[5] = host[MCT_FMASK];
  return VSA_OK;
}

}  // namespace

extern "C" int vsa_mesh_clusters(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                                 void* workspace, long long workspace_bytes, int32_t* out_triangle_clusters,
                                 int32_t* out_cluster_n_triangles, double* out_cluster_area,
                                 long long* out_nr_clusters, float* stage_ms, void* stream) {
  if (!verts || !faces || !workspace || !out_triangle_clusters || !out_cluster_n_triangles || !out_cluster_area ||
      !out_nr_clusters)
    return VSA_ERR_ARG;
  int rc = mt::check_vf(nr_verts, nr_faces);
  if (rc != VSA_OK) return rc;
  Mcl m;
  rc = setup(m, verts, nr_verts, faces, nr_faces, workspace, workspace_bytes, stage_ms, stream);
  if (rc != VSA_OK) return rc;
  rc = cluster_stages(m, out_triangle_clusters, out_cluster_n_triangles);
  if (rc == VSA_OK) rc = area_stage(m, out_triangle_clusters, out_cluster_n_triangles, out_cluster_area);
  if (rc == VSA_OK) {
    const hipError_t e = hipStreamSynchronize(m.st);
    rc = e == hipSuccess ? VSA_OK : (int)e;
  }
  m.timer.destroy();
  if (rc == VSA_OK) *out_nr_clusters = m.C;
  return rc;
}

extern "C" int vsa_mesh_filter(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                               int mode, const uint8_t* keep_mask, long long cluster_to_keep,
                               long long min_cluster_faces, int drop_unreferenced, int drop_degenerate,
                               void* workspace, long long workspace_bytes, float* out_verts, int32_t* out_faces,
                               int32_t* out_vertex_map, int32_t* out_face_map, long long* stats, float* stage_ms,
                               void* stream) {
  if (!verts || !faces || !workspace || !out_verts || !out_faces || !out_vertex_map || !out_face_map || !stats)
    return VSA_ERR_ARG;
  if (mode < 0 || mode > 2 || (mode == 1 && !keep_mask)) return VSA_ERR_ARG;
  if (mode == 2 && (cluster_to_keep < 1 || min_cluster_faces < 0)) return VSA_ERR_ARG;
  int rc = mt::check_vf(nr_verts, nr_faces);
  if (rc != VSA_OK) return rc;
  Mcl m;
  rc = setup(m, verts, nr_verts, faces, nr_faces, workspace, workspace_bytes, stage_ms, stream);
  if (rc != VSA_OK) return rc;
  rc = run_filter(m, mode, keep_mask, cluster_to_keep, min_cluster_faces, drop_unreferenced != 0, drop_degenerate != 0,
                  out_verts, out_faces, out_vertex_map, out_face_map, stats);
  m.timer.destroy();
  return rc;
}

extern "C" int vsa_mesh_compact_rows(const void* rows, long long nr_rows, int row_words, const int32_t* map, void* out,
                                     void* stream) {
  if (nr_rows < 0 || row_words < 1) return VSA_ERR_ARG;
  if (nr_rows == 0) return VSA_OK;
  if (!rows || !map || !out) return VSA_ERR_ARG;
  if (nr_rows > 0x7FFFFFFFll) return VSA_ERR_UNSUPPORTED;
  const long long n = nr_rows * (long long)row_words;
  hipLaunchKernelGGL(mcl_compact_rows, dim3((unsigned)((n + MC_BLOCK - 1) / MC_BLOCK)), dim3(MC_BLOCK), 0,
                     (hipStream_t)stream, static_cast<const uint32_t*>(rows), nr_rows, row_words, map,
                     static_cast<uint32_t*>(out));
  VSA_RETURN_LAUNCH_STATUS();
}
