// Mesh repair: welding vertices and orienting faces (vsa_mesh_weld, vsa_mesh_orient; rules in include/volsurfs_hip.h
// "Mesh repair").  One stream, built on csrc/mesh_topology.h.
//
// Grouping rows of three words (welding at tol = 0 and the duplicate faces share it):
//   rep[i] = the lowest index whose row equals row i.  Three stable radix sorts of (word, index) over 32 bits, last
//   word first, from iota: equal rows end up adjacent in ascending index, so the head of a run is its minimum.  A
//   run-head kernel flags the heads, a scan numbers the runs, one scatter writes each run's head and one hands it to
//   the run's members.
// Weld:
//   rows:     tol = 0: the coordinate bits with -0.0 -> +0.0, grouped (a row with a NaN is a run of its own).
//   cells:    tol > 0: the cell floor(p / tol) per axis in fp64, 21 bits each, packed; (cell, vertex) sorted; a lane per
//             vertex searches the 27 neighbouring cells (9 searches of 3 consecutive cells) and hooks itself to every
//             lower vertex within tol; a read-only root walk gives the lowest vertex of the cluster.
//   vertices: the representatives flagged, scanned and written with their own bits; vertex_map = the new index of the
//             representative.
//   faces:    remapped; degenerate and duplicate faces (the sorted triples, grouped) flagged; scanned and written in order.
// Orient:
//   live:     the faces with a positive finite area (the census' rule).
//   edges:    the sorted edge keys with their corner slots.
//   hook:     the head of a run with exactly two live faces hooks the double cover: node 2 f + s = face f kept / flipped.
//   roots:    component = root(2 f) >> 1, relative flip = root(2 f) & 1, not orientable iff root(2 f) = root(2 f + 1).
//   sums:     (component, face) sorted by component; per component, in mesh_clean's fixed shape (chunks of 2048, then a
//             wave per component that spans chunks): sum A c and sum A, then S and U about the centroid.  No float atomics.
//   flip:     a component is decided iff |S| > 2^-20 U; a decided one with the wrong sign is flipped whole.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mesh_topology.h"

#define MR_BLOCK MT_BLOCK
#define MR_ITEMS 8
#define MR_CHUNK (MR_BLOCK * MR_ITEMS)
#define MR_CELL_BITS 21
#define MR_CELL_HALF (1ll << (MR_CELL_BITS - 1))
#define MR_NO_CELL (~0ull)

// device counters
#define MRC_VOUT 0
#define MRC_FOUT 1
#define MRC_DEGENERATE 2
#define MRC_DUPLICATE 3
#define MRC_RANGE 4       // vertices whose cell index leaves +-2^20
#define MRC_COMPONENTS 0
#define MRC_FLIPPED 1
#define MRC_UNORIENTABLE 2
#define MRC_UNDECIDED 3
#define MRC_UNDECIDED_FACES 4
#define MRC_N 8

#define MRW_STAGES 4
enum { SW_GROUP, SW_VERTICES, SW_DUPLICATES, SW_FACES };
#define MRO_STAGES 5
enum { SO_EDGES, SO_HOOK, SO_ROOTS, SO_SUMS, SO_FLIP };

using mt::at;
using mt::u64;

// ------------------------------------------------------------------------------------------------ shared

// ctr[k] += the wave's sum of x (integers: the order does not matter), one atomic per wave.
__device__ __forceinline__ void mrp_wave_add(long long* ctr, long long x) {
#pragma unroll
  for (int d = VSA_WAVE / 2; d > 0; d >>= 1) x += __shfl_down(x, d, VSA_WAVE);
  if ((threadIdx.x & (VSA_WAVE - 1)) == 0 && x) atomicAdd((unsigned long long*)ctr, (unsigned long long)x);
}

__global__ __launch_bounds__(MR_BLOCK) void mrp_iota(uint32_t* __restrict__ x, long long n) {
  const long long i = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i < n) x[i] = (uint32_t)i;
}

// keys[i] = word w of row idx[i].
__global__ __launch_bounds__(MR_BLOCK) void mrp_gather_word(const uint32_t* __restrict__ rows,
                                                           const uint32_t* __restrict__ idx, long long n, int w,
                                                           uint32_t* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i < n) keys[i] = rows[3 * (long long)idx[i] + w];
}

__device__ __forceinline__ bool mrp_nan_bits(uint32_t b) { return (b & 0x7FFFFFFFu) > 0x7F800000u; }

// head[i] = sorted position i opens a run.  With nan_alone, a row that holds a NaN is a run of its own.
__global__ __launch_bounds__(MR_BLOCK) void mrp_run_heads(const uint32_t* __restrict__ rows,
                                                         const uint32_t* __restrict__ idx, long long n, int nan_alone,
                                                         int32_t* __restrict__ head) {
  const long long i = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= n) return;
  bool h = i == 0;
  if (!h) {
    const uint32_t* a = rows + 3 * (long long)idx[i];
    const uint32_t* b = rows + 3 * (long long)idx[i - 1];
    h = a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
    if (nan_alone && (mrp_nan_bits(a[0]) || mrp_nan_bits(a[1]) || mrp_nan_bits(a[2]))) h = true;
  }
  head[i] = h;
}

// run_head[r] = the index at the head of run r (rank = the exclusive scan of head).
__global__ __launch_bounds__(MR_BLOCK) void mrp_scatter_heads(const uint32_t* __restrict__ idx,
                                                             const int32_t* __restrict__ head,
                                                             const int32_t* __restrict__ rank, long long n,
                                                             uint32_t* __restrict__ run_head) {
  const long long i = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i < n && head[i]) run_head[rank[i]] = idx[i];
}

__global__ __launch_bounds__(MR_BLOCK) void mrp_scatter_rep(const uint32_t* __restrict__ idx,
                                                           const int32_t* __restrict__ head,
                                                           const int32_t* __restrict__ rank,
                                                           const uint32_t* __restrict__ run_head, long long n,
                                                           int32_t* __restrict__ rep) {
  const long long i = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i < n) rep[idx[i]] = (int32_t)run_head[rank[i] + head[i] - 1];
}

namespace {

// The buffers of one grouping: four u32 [n] for the sorts, two i32 [n] for the heads and their scan.
struct GroupBufs {
  uint32_t *ka, *kb, *va, *vb;
  int32_t *head, *rank;
};

// rep[i] = the lowest index whose row of three words equals row i.
int group_rows(const uint32_t* rows, long long n, int nan_alone, const GroupBufs& g, int32_t* rep, mt::Tmp tmp,
               hipStream_t st) {
  uint32_t *vin = g.va, *vout = g.vb;
  hipLaunchKernelGGL(mrp_iota, mt::grid(n), dim3(MR_BLOCK), 0, st, vin, n);
  MT_LAUNCHED();
  for (int w = 2; w >= 0; --w) {
    hipLaunchKernelGGL(mrp_gather_word, mt::grid(n), dim3(MR_BLOCK), 0, st, rows, vin, n, w, g.ka);
    MT_LAUNCHED();
    MT_TRY(mt::sort_pairs(tmp, g.ka, g.kb, vin, vout, (size_t)n, 0, 32, st));
    uint32_t* t = vin;
    vin = vout;
    vout = t;
  }
  hipLaunchKernelGGL(mrp_run_heads, mt::grid(n), dim3(MR_BLOCK), 0, st, rows, vin, n, nan_alone, g.head);
  MT_LAUNCHED();
  MT_TRY(mt::exclusive_scan(tmp, g.head, g.rank, (size_t)n, st));
  hipLaunchKernelGGL(mrp_scatter_heads, mt::grid(n), dim3(MR_BLOCK), 0, st, vin, g.head, g.rank, n, g.ka);
  MT_LAUNCHED();
  hipLaunchKernelGGL(mrp_scatter_rep, mt::grid(n), dim3(MR_BLOCK), 0, st, vin, g.head, g.rank, g.ka, n, rep);
  MT_LAUNCHED();
  return VSA_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ weld

// rows[v] = the coordinate bits of vertex v with -0.0 -> +0.0.
__global__ __launch_bounds__(MR_BLOCK) void mrw_vertex_rows(const float* __restrict__ P, long long n3,
                                                           uint32_t* __restrict__ rows) {
  const long long i = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= n3) return;
  const uint32_t b = __float_as_uint(P[i]);
  rows[i] = b == 0x80000000u ? 0u : b;
}

// keys[v] = the packed cell of vertex v (x << 42 | y << 21 | z, each floor(p / tol) + 2^20), vals[v] = v.  A vertex with
// a NaN has no cell; one whose cell leaves +-2^20 has none either and is counted.
__global__ __launch_bounds__(MR_BLOCK) void mrw_cells(const float* __restrict__ P, long long V, double tol,
                                                     u64* __restrict__ keys, uint32_t* __restrict__ vals,
                                                     long long* __restrict__ ctr) {
  const long long v = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  bool bad = false;
  if (v < V) {
    u64 key = 0;
    bool nan = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double x = (double)P[3 * v + a];
      const double c = floor(x / tol);
      if (x != x) nan = true;
      else if (!(c >= (double)-MR_CELL_HALF && c < (double)MR_CELL_HALF)) bad = true;
      else key = key << MR_CELL_BITS | (u64)((long long)c + MR_CELL_HALF);
    }
    bad = bad && !nan;
    keys[v] = nan || bad ? MR_NO_CELL : key;
    vals[v] = (uint32_t)v;
  }
  mrp_wave_add(ctr + MRC_RANGE, bad ? 1 : 0);
}

// A lane per vertex: every lower vertex of the 27 neighbouring cells within tol (fp64, ((dx dx + dy dy) + dz dz) <=
// tol tol) is hooked to it.  The cells (x, y, z - 1 .. z + 1) are consecutive keys: nine searches.  Many vertices in
// one cell cost the square of their number.
__global__ __launch_bounds__(MR_BLOCK) void mrw_neighbours(const float* __restrict__ P, long long V, double tol2,
                                                          const u64* __restrict__ keys,
                                                          const u64* __restrict__ sorted,
                                                          const uint32_t* __restrict__ order, int32_t* par) {
  const long long v = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (v >= V) return;
  const u64 key = keys[v];
  if (key == MR_NO_CELL) return;
  const long long top = (1ll << MR_CELL_BITS) - 1;
  const long long cx = (long long)(key >> (2 * MR_CELL_BITS)), cy = (long long)(key >> MR_CELL_BITS) & top,
                  cz = (long long)key & top;
  const double px = P[3 * v], py = P[3 * v + 1], pz = P[3 * v + 2];
  const long long z0 = cz > 0 ? cz - 1 : 0, z1 = cz < top ? cz + 1 : top;
  for (int dx = -1; dx <= 1; ++dx) {
    const long long x = cx + dx;
    if (x < 0 || x > top) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const long long y = cy + dy;
      if (y < 0 || y > top) continue;
      const u64 base = (u64)x << (2 * MR_CELL_BITS) | (u64)y << MR_CELL_BITS;
      const u64 klo = base | (u64)z0, khi = base | (u64)z1;
      long long lo = 0, hi = V;          // the first position with sorted >= klo
      while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (sorted[mid] < klo) lo = mid + 1;
        else hi = mid;
      }
      for (long long k = lo; k < V && sorted[k] <= khi; ++k) {
        const long long j = order[k];
        if (j >= v) continue;
        const double ex = px - (double)P[3 * j], ey = py - (double)P[3 * j + 1], ez = pz - (double)P[3 * j + 2];
        if ((ex * ex + ey * ey) + ez * ez <= tol2) fu_union(par, (int)j, (int)v);
      }
    }
  }
}

__global__ __launch_bounds__(MR_BLOCK) void mrw_rep_flags(const int32_t* __restrict__ rep, long long n,
                                                         int32_t* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i < n) flag[i] = rep[i] == (int32_t)i;
}

// The representatives in order with their own bits; vmap[v] = the new index of v's representative.
__global__ __launch_bounds__(MR_BLOCK) void mrw_emit_verts(const float* __restrict__ P, long long V,
                                                          const int32_t* __restrict__ rep,
                                                          const int32_t* __restrict__ flag,
                                                          const int32_t* __restrict__ rank,
                                                          float* __restrict__ out_verts, int32_t* __restrict__ vmap,
                                                          long long* __restrict__ ctr) {
  const long long v = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (v >= V) return;
  const long long r = rank[v];
  if (flag[v]) {
    out_verts[3 * r] = P[3 * v];
    out_verts[3 * r + 1] = P[3 * v + 1];
    out_verts[3 * r + 2] = P[3 * v + 2];
  }
  vmap[v] = rank[rep[v]];
  if (v == V - 1) ctr[MRC_VOUT] = r + flag[v];
}

// nf[f] = the face through vmap; rows[f] = its three new indices in ascending order.
__global__ __launch_bounds__(MR_BLOCK) void mrw_remap_faces(const int32_t* __restrict__ faces, long long F,
                                                           const int32_t* __restrict__ vmap,
                                                           int32_t* __restrict__ nf, uint32_t* __restrict__ rows) {
  const long long f = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (f >= F) return;
  const int a = vmap[faces[3 * f]], b = vmap[faces[3 * f + 1]], c = vmap[faces[3 * f + 2]];
  nf[3 * f] = a;
  nf[3 * f + 1] = b;
  nf[3 * f + 2] = c;
  const int lo = min(a, min(b, c)), hi = max(a, max(b, c));
  rows[3 * f] = (uint32_t)lo;
  rows[3 * f + 1] = (uint32_t)((long long)a + b + c - lo - hi);
  rows[3 * f + 2] = (uint32_t)hi;
}

// keep[f]: not dropped as degenerate (first) nor as the duplicate of a lower face; both kinds counted.
__global__ __launch_bounds__(MR_BLOCK) void mrw_keep_faces(const int32_t* __restrict__ nf, long long F,
                                                          const int32_t* __restrict__ rep, int drop_degenerate,
                                                          int32_t* __restrict__ keep, long long* __restrict__ ctr) {
  const long long f = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  bool deg = false, dup = false;
  if (f < F) {
    const int a = nf[3 * f], b = nf[3 * f + 1], c = nf[3 * f + 2];
    deg = drop_degenerate && (a == b || b == c || c == a);
    dup = !deg && rep && rep[f] != (int32_t)f;
    keep[f] = !deg && !dup;
  }
  mrp_wave_add(ctr + MRC_DEGENERATE, deg ? 1 : 0);
  mrp_wave_add(ctr + MRC_DUPLICATE, dup ? 1 : 0);
}

__global__ __launch_bounds__(MR_BLOCK) void mrw_emit_faces(const int32_t* __restrict__ nf, long long F,
                                                          const int32_t* __restrict__ keep,
                                                          const int32_t* __restrict__ rank,
                                                          int32_t* __restrict__ out_faces, int32_t* __restrict__ fmap,
                                                          long long* __restrict__ ctr) {
  const long long f = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (f >= F) return;
  const long long r = rank[f];
  if (keep[f]) {
    out_faces[3 * r] = nf[3 * f];
    out_faces[3 * r + 1] = nf[3 * f + 1];
    out_faces[3 * r + 2] = nf[3 * f + 2];
  }
  fmap[f] = keep[f] ? (int32_t)r : -1;
  if (f == F - 1) ctr[MRC_FOUT] = r + keep[f];
}

struct WeldLayout {
  size_t ctr, ka, kb, va, vb, rows, ckey, csorted, rep, flag, rank, par, nf, tmp, tmp_bytes, total;
};

// The buffers before rocPRIM's temporary storage (no HIP call: a workspace below l->tmp + 16 is too small whatever the
// size query says); weld_layout adds the storage.
static void weld_buffers(long long V, long long F, WeldLayout* l) {
  const size_t v = (size_t)V, f = (size_t)F, n = f > v ? f : v;
  mt::Bump b;
  l->ctr = b.take(8 * MRC_N);
  l->ka = b.take(4 * n);
  l->kb = b.take(4 * n);
  l->va = b.take(4 * n);
  l->vb = b.take(4 * n);
  l->rows = b.take(12 * n);
  l->ckey = b.take(8 * v);
  l->csorted = b.take(8 * v);
  l->rep = b.take(4 * n);
  l->flag = b.take(4 * n);
  l->rank = b.take(4 * n);
  l->par = b.take(4 * v);
  l->nf = b.take(12 * f);
  l->tmp = b.o;
}

static int weld_layout(long long V, long long F, WeldLayout* l) {
  const size_t v = (size_t)V, f = (size_t)F, n = f > v ? f : v;
  weld_buffers(V, F, l);
  mt::TmpCounts cnt = {};
  cnt.pairs64 = v;
  cnt.pairs32 = n;
  cnt.xscan32 = n;
  MT_TRY(mt::tmp_bytes(cnt, &l->tmp_bytes));
  l->total = l->tmp + mt::align(l->tmp_bytes);
  return VSA_OK;
}

extern "C" long long vsa_mesh_weld_workspace_bytes(long long nr_verts, long long nr_faces) {
  WeldLayout l;
  int rc = mt::check_vf(nr_verts, nr_faces);
  if (rc == VSA_OK) rc = mt::abi_status(weld_layout(nr_verts, nr_faces, &l));
  return rc != VSA_OK ? rc : (long long)l.total;
}

extern "C" int vsa_mesh_weld(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                             double tol, int drop_degenerate, int drop_duplicates, void* workspace,
                             long long workspace_bytes, float* out_verts, int32_t* out_faces, int32_t* out_vertex_map,
                             int32_t* out_face_map, long long* stats, float* stage_ms, void* stream) {
  if (!verts || !faces || !workspace || !out_verts || !out_faces || !out_vertex_map || !out_face_map || !stats)
    return VSA_ERR_ARG;
  if (!(tol >= 0.0) || !(tol < INFINITY)) return VSA_ERR_ARG;      // negative, NaN or infinite
  int rc = mt::check_vf(nr_verts, nr_faces);
  if (rc != VSA_OK) return rc;
  WeldLayout l;
  weld_buffers(nr_verts, nr_faces, &l);
  if (workspace_bytes < (long long)l.tmp + 16) return VSA_ERR_ARG;
  MT_TRY(mt::abi_status(weld_layout(nr_verts, nr_faces, &l)));
  if (workspace_bytes < (long long)l.total) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const long long V = nr_verts, F = nr_faces;
  char* ws = static_cast<char*>(workspace);
  const mt::Tmp tmp = {ws + l.tmp, l.tmp_bytes};
  long long* ctr = at<long long>(ws, l.ctr);
  const GroupBufs g = {at<uint32_t>(ws, l.ka), at<uint32_t>(ws, l.kb), at<uint32_t>(ws, l.va), at<uint32_t>(ws, l.vb),
                       at<int32_t>(ws, l.flag), at<int32_t>(ws, l.rank)};
  uint32_t* rows = at<uint32_t>(ws, l.rows);
  int32_t* rep = at<int32_t>(ws, l.rep);
  int32_t* flag = at<int32_t>(ws, l.flag);
  int32_t* rank = at<int32_t>(ws, l.rank);
  int32_t* nf = at<int32_t>(ws, l.nf);
  mt::StageTimer timer;
  MT_TRY(timer.create(stage_ms, MRW_STAGES, st));
  auto run = [&]() -> int {
    VSA_HIP_TRY(hipMemsetAsync(ctr, 0, 8 * MRC_N, st));
    MT_TRY(timer.open());
    if (tol == 0.0) {
      hipLaunchKernelGGL(mrw_vertex_rows, mt::grid(3 * V), dim3(MR_BLOCK), 0, st, verts, 3 * V, rows);
      MT_LAUNCHED();
      MT_TRY(group_rows(rows, V, 1, g, rep, tmp, st));
      hipLaunchKernelGGL(mrw_rep_flags, mt::grid(V), dim3(MR_BLOCK), 0, st, rep, V, flag);
      MT_LAUNCHED();
    } else {
      u64* ckey = at<u64>(ws, l.ckey);
      u64* csorted = at<u64>(ws, l.csorted);
      int32_t* par = at<int32_t>(ws, l.par);
      hipLaunchKernelGGL(mrw_cells, mt::grid(V), dim3(MR_BLOCK), 0, st, verts, V, tol, ckey, g.va, ctr);
      MT_LAUNCHED();
      MT_TRY(mt::sort_pairs(tmp, ckey, csorted, g.va, g.vb, (size_t)V, 0, 64, st));
      MT_TRY(mt::iota(par, V, st));
      hipLaunchKernelGGL(mrw_neighbours, mt::grid(V), dim3(MR_BLOCK), 0, st, verts, V, tol * tol, ckey, csorted, g.vb,
                         par);
      MT_LAUNCHED();
      MT_TRY(mt::roots(par, V, rep, flag, st));
    }
    MT_TRY(timer.close(SW_GROUP));
    MT_TRY(timer.open());
    MT_TRY(mt::exclusive_scan(tmp, flag, rank, (size_t)V, st));
    hipLaunchKernelGGL(mrw_emit_verts, mt::grid(V), dim3(MR_BLOCK), 0, st, verts, V, rep, flag, rank, out_verts,
                       out_vertex_map, ctr);
    MT_LAUNCHED();
    hipLaunchKernelGGL(mrw_remap_faces, mt::grid(F), dim3(MR_BLOCK), 0, st, faces, F, out_vertex_map, nf, rows);
    MT_LAUNCHED();
    MT_TRY(timer.close(SW_VERTICES));
    MT_TRY(timer.open());
    if (drop_duplicates) MT_TRY(group_rows(rows, F, 0, g, rep, tmp, st));
    MT_TRY(timer.close(SW_DUPLICATES));
    MT_TRY(timer.open());
    hipLaunchKernelGGL(mrw_keep_faces, mt::grid(F), dim3(MR_BLOCK), 0, st, nf, F,
                       drop_duplicates ? rep : (const int32_t*)nullptr, drop_degenerate, flag, ctr);
    MT_LAUNCHED();
    MT_TRY(mt::exclusive_scan(tmp, flag, rank, (size_t)F, st));
    hipLaunchKernelGGL(mrw_emit_faces, mt::grid(F), dim3(MR_BLOCK), 0, st, nf, F, flag, rank, out_faces, out_face_map,
                       ctr);
    MT_LAUNCHED();
    long long host[MRC_N];
    MT_TRY(mt::read_counters(st, ctr, host, MRC_N));      // the one blocking read
    MT_TRY(timer.close(SW_FACES));
    if (host[MRC_RANGE]) return VSA_ERR_UNSUPPORTED;
    stats[0] = host[MRC_VOUT];
    stats[1] = host[MRC_FOUT];
    stats[2] = host[MRC_DEGENERATE];
    stats[3] = host[MRC_DUPLICATE];
    return VSA_OK;
  };
  rc = run();
  timer.destroy();
  return rc;
}

// ------------------------------------------------------------------------------------------------ orient

// live[f] = the face has a positive finite area (fp64 on the fp32 vertices: vsa_mesh_edge_census' rule).
__global__ __launch_bounds__(MR_BLOCK) void mro_live(const float* __restrict__ P, const int32_t* __restrict__ faces,
                                                    long long F, uint8_t* __restrict__ live) {
  const long long f = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
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

// The lane at the head of a run of equal edge keys: exactly two live, different faces f and g give a constraint.  par =
// both corners leave the same vertex (the two faces traverse the edge in the same direction).  Node 2 f + s: face f kept
// (s = 0) or flipped (s = 1); 2 f joins 2 g + par and 2 f + 1 joins 2 g + 1 - par.
__global__ __launch_bounds__(MR_BLOCK) void mro_hook(const u64* __restrict__ sorted, const uint32_t* __restrict__ slot,
                                                    long long n3, const int32_t* __restrict__ faces,
                                                    const uint8_t* __restrict__ live, int32_t* par) {
  const long long j = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (j >= n3) return;
  const u64 key = sorted[j];
  if (j > 0 && sorted[j - 1] == key) return;
  int n = 0, from[2] = {0, 0};
  long long face[2] = {0, 0};
  for (long long k = j; k < n3 && sorted[k] == key; ++k) {
    const long long i = slot[k];
    if (!live[i / 3]) continue;
    if (n < 2) {
      from[n] = faces[i];
      face[n] = i / 3;
    }
    ++n;
  }
  if (n != 2 || face[0] == face[1]) return;
  const int same = from[0] == from[1];
  fu_union(par, (int)(2 * face[0]), (int)(2 * face[1] + same));
  fu_union(par, (int)(2 * face[0] + 1), (int)(2 * face[1] + 1 - same));
}

// cflag[f] = f is the lowest face of its component (root holds the roots of the 2 F nodes).
__global__ __launch_bounds__(MR_BLOCK) void mro_component_flags(const int32_t* __restrict__ root, long long F,
                                                               int32_t* __restrict__ cflag) {
  const long long f = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (f < F) cflag[f] = (root[2 * f] >> 1) == (int32_t)f;
}

// The sort's pairs: (the component's number in ascending lowest face, face); component[f] = its lowest face.
__global__ __launch_bounds__(MR_BLOCK) void mro_sort_pairs(const int32_t* __restrict__ root,
                                                          const int32_t* __restrict__ cflag,
                                                          const int32_t* __restrict__ rank, long long F,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                          int32_t* __restrict__ component,
                                                          long long* __restrict__ ctr) {
  const long long f = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (f >= F) return;
  const int m = root[2 * f] >> 1;
  component[f] = m;
  keys[f] = (uint32_t)rank[m];
  vals[f] = (uint32_t)f;
  if (f == F - 1) ctr[MRC_COMPONENTS] = rank[f] + cflag[f];
}

// Sorted position i holds face sface[i] of component skey[i]: its positions are [start[c], end[c]).
__global__ __launch_bounds__(MR_BLOCK) void mro_ranges(const uint32_t* __restrict__ skey, long long F,
                                                      int32_t* __restrict__ start, int32_t* __restrict__ end) {
  const long long i = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  if (i >= F) return;
  if (i == 0 || skey[i] != skey[i - 1]) start[skey[i]] = (int32_t)i;
  if (i == F - 1 || skey[i] != skey[i + 1]) end[skey[i]] = (int32_t)(i + 1);
}

// The terms of face f in fp64 from the fp32 vertices, no contraction.  N = 1/2 (v1 - v0) x (v2 - v0), negated for a face
// the relative orientation flips; A = |N|; c = ((v0 + v1) + v2) / 3.
//   PASS 1 (4 values): A c.xyz, A.
//   PASS 2 (2 values): N . (c - cbar) = (Nx dx + Ny dy) + Nz dz, and A (|c|_1 + |cbar|_1); cbar = first[0..2] / first[3]
//     (0 for a component without area).
// A face without a finite area contributes nothing.
template <int PASS>
__device__ __forceinline__ void mro_terms(const float* __restrict__ P, const int32_t* __restrict__ faces,
                                          const int32_t* __restrict__ root, const double* __restrict__ first,
                                          long long f, long long c, double* out) {
  const long long i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  const double ax = P[3 * i0], ay = P[3 * i0 + 1], az = P[3 * i0 + 2];
  const double bx = P[3 * i1], by = P[3 * i1 + 1], bz = P[3 * i1 + 2];
  const double cx = P[3 * i2], cy = P[3 * i2 + 1], cz = P[3 * i2 + 2];
  const double e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
  double nx = 0.5 * (e1y * e2z - e1z * e2y), ny = 0.5 * (e1z * e2x - e1x * e2z), nz = 0.5 * (e1x * e2y - e1y * e2x);
  const double A = sqrt((nx * nx + ny * ny) + nz * nz);
  const double mx = ((ax + bx) + cx) / 3.0, my = ((ay + by) + cy) / 3.0, mz = ((az + bz) + cz) / 3.0;
  const bool ok = A < INFINITY;      // (false for NaN too)
  if constexpr (PASS == 1) {
    out[0] = ok ? A * mx : 0.0;
    out[1] = ok ? A * my : 0.0;
    out[2] = ok ? A * mz : 0.0;
    out[3] = ok ? A : 0.0;
  } else {
    if (root[2 * f] & 1) {
      nx = -nx;
      ny = -ny;
      nz = -nz;
    }
    const double sa = first[4 * c + 3];
    const double qx = sa > 0.0 ? first[4 * c] / sa : 0.0, qy = sa > 0.0 ? first[4 * c + 1] / sa : 0.0,
                 qz = sa > 0.0 ? first[4 * c + 2] / sa : 0.0;
    const double s = (nx * (mx - qx) + ny * (my - qy)) + nz * (mz - qz);
    const double u = A * (((fabs(mx) + fabs(my)) + fabs(mz)) + ((fabs(qx) + fabs(qy)) + fabs(qz)));
    out[0] = ok ? s : 0.0;
    out[1] = ok ? u : 0.0;
  }
}

// mesh_clean's mcl_area_chunks with NV values per face: one block per chunk of MR_CHUNK sorted positions, the segmented
// inclusive sums in a fixed shape (each lane adds its MR_ITEMS consecutive items in order, then a Hillis-Steele scan of
// the lanes' sums in LDS).  A component inside the chunk gets its sums; head[b] = the sums of the chunk's first piece,
// tail[b] of its last.
template <int PASS, int NV>
__global__ __launch_bounds__(MR_BLOCK) void mro_sum_chunks(const float* __restrict__ P,
                                                          const int32_t* __restrict__ faces,
                                                          const int32_t* __restrict__ root,
                                                          const double* __restrict__ first,
                                                          const uint32_t* __restrict__ skey,
                                                          const uint32_t* __restrict__ sface, long long F,
                                                          const int32_t* __restrict__ start,
                                                          const int32_t* __restrict__ end, double* __restrict__ sums,
                                                          double* __restrict__ head, double* __restrict__ tail) {
  __shared__ double sv[2][NV][MR_BLOCK];
  __shared__ int sf[2][MR_BLOCK];
  const long long lo = (long long)blockIdx.x * MR_CHUNK;
  const long long hi = lo + MR_CHUNK < F ? lo + MR_CHUNK : F;
  const long long base = lo + (long long)threadIdx.x * MR_ITEMS;
  double run[MR_ITEMS][NV];
  uint32_t key[MR_ITEMS];
  double acc[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) acc[q] = 0.0;
  int has_start = 0;
#pragma unroll
  for (int k = 0; k < MR_ITEMS; ++k) {
    const long long i = base + k;
    key[k] = 0u;
#pragma unroll
    for (int q = 0; q < NV; ++q) run[k][q] = 0.0;
    if (i >= hi) continue;
    key[k] = skey[i];
    if (i == lo || key[k] != skey[i - 1]) {
      has_start = 1;
#pragma unroll
      for (int q = 0; q < NV; ++q) acc[q] = 0.0;
    }
    double t[NV];
    mro_terms<PASS>(P, faces, root, first, sface[i], key[k], t);
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      acc[q] = acc[q] + t[q];
      run[k][q] = acc[q];
    }
  }
  int cur = 0;
#pragma unroll
  for (int q = 0; q < NV; ++q) sv[0][q][threadIdx.x] = acc[q];
  sf[0][threadIdx.x] = has_start;
  __syncthreads();
  for (int d = 1; d < MR_BLOCK; d <<= 1) {
    double v[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = sv[cur][q][threadIdx.x];
    int fl = sf[cur][threadIdx.x];
    if ((int)threadIdx.x >= d && !fl) {
#pragma unroll
      for (int q = 0; q < NV; ++q) v[q] = sv[cur][q][threadIdx.x - d] + v[q];
      fl = sf[cur][threadIdx.x - d];
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) sv[cur ^ 1][q][threadIdx.x] = v[q];
    sf[cur ^ 1][threadIdx.x] = fl;
    cur ^= 1;
    __syncthreads();
  }
  double carry[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) carry[q] = threadIdx.x > 0 ? sv[cur][q][threadIdx.x - 1] : 0.0;
  bool seen = false;
#pragma unroll
  for (int k = 0; k < MR_ITEMS; ++k) {
    const long long i = base + k;
    if (i >= hi) continue;
    const bool st = i == lo || key[k] != skey[i - 1];
    seen = seen || st;
    const bool last = i + 1 == hi;
    const bool fin = last || skey[i + 1] != key[k];
    if (!fin) continue;
    const long long s0 = start[key[k]], s1 = end[key[k]];
    const bool inside = s0 >= lo && s1 <= hi, first_piece = key[k] == skey[lo];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const double sum = seen ? run[k][q] : carry[q] + run[k][q];
      if (inside) sums[(long long)NV * key[k] + q] = sum;
      if (first_piece) head[(long long)NV * blockIdx.x + q] = sum;
      if (last) tail[(long long)NV * blockIdx.x + q] = sum;
    }
  }
}

// A component that spans the chunks b0 < b1: tail[b0] + (head[b0 + 1] + ... + head[b1]).  One wave per chunk b >= 1
// takes the component that crosses into it from chunk b - 1 where it starts: lane l adds head[b + l], head[b + l + 64],
// ... in ascending order, then a shuffle tree of fixed shape joins the lanes.
template <int NV>
__global__ __launch_bounds__(VSA_WAVE) void mro_sum_spans(const uint32_t* __restrict__ skey,
                                                         const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ end,
                                                         const double* __restrict__ head,
                                                         const double* __restrict__ tail, double* __restrict__ sums) {
  const long long b = (long long)blockIdx.x + 1, lo = b * MR_CHUNK;
  const uint32_t c = skey[lo];
  if (skey[lo - 1] != c) return;
  const long long s0 = start[c];
  if (s0 < lo - MR_CHUNK) return;          // it starts earlier: the wave of that chunk's successor has it
  const long long b1 = ((long long)end[c] - 1) / MR_CHUNK;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double sum = 0.0;
    for (long long k = b + threadIdx.x; k <= b1; k += VSA_WAVE) sum = sum + head[NV * k + q];
#pragma unroll
    for (int d = VSA_WAVE / 2; d > 0; d >>= 1) sum = sum + __shfl_down(sum, d, VSA_WAVE);
    if (threadIdx.x == 0) sums[(long long)NV * c + q] = tail[NV * (b - 1) + q] + sum;
  }
}

// A lane per component: orientable iff the two nodes of its lowest face have different roots; decided iff
// |S| > 2^-20 U; flipc = a decided component whose S has the wrong sign.
__global__ __launch_bounds__(MR_BLOCK) void mro_decide(const int32_t* __restrict__ root,
                                                      const uint32_t* __restrict__ sface,
                                                      const int32_t* __restrict__ start,
                                                      const int32_t* __restrict__ end,
                                                      const double* __restrict__ second, long long F, int outward,
                                                      uint8_t* __restrict__ flipc, long long* __restrict__ ctr) {
  const long long c = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  long long unorientable = 0, undecided = 0, faces_left = 0;
  if (c < F && c < ctr[MRC_COMPONENTS]) {
    const long long m = sface[start[c]];
    const double S = second[2 * c], U = second[2 * c + 1];
    const bool orientable = root[2 * m] != root[2 * m + 1];
    const bool decided = orientable && fabs(S) > 0x1p-20 * U;
    flipc[c] = decided && (outward ? S < 0.0 : S > 0.0);
    unorientable = !orientable;
    undecided = orientable && !decided;
    faces_left = undecided ? end[c] - start[c] : 0;
  }
  mrp_wave_add(ctr + MRC_UNORIENTABLE, unorientable);
  mrp_wave_add(ctr + MRC_UNDECIDED, undecided);
  mrp_wave_add(ctr + MRC_UNDECIDED_FACES, faces_left);
}

// flipped[f] = the relative flip xor its component's; a flipped face swaps its corners 1 and 2 (and their UVs).
__global__ __launch_bounds__(MR_BLOCK) void mro_flip(const int32_t* __restrict__ faces, long long F,
                                                    const int32_t* __restrict__ root,
                                                    const int32_t* __restrict__ rank,
                                                    const uint8_t* __restrict__ flipc, const float* __restrict__ uvs,
                                                    int32_t* __restrict__ out_faces, float* __restrict__ out_uvs,
                                                    uint8_t* __restrict__ flipped, long long* __restrict__ ctr) {
  const long long f = (long long)blockIdx.x * MR_BLOCK + threadIdx.x;
  bool fl = false;
  if (f < F) {
    const int r = root[2 * f];
    const bool orientable = r != root[2 * f + 1];
    fl = orientable && ((r & 1) != 0) != (flipc[rank[r >> 1]] != 0);
    flipped[f] = fl;
    out_faces[3 * f] = faces[3 * f];
    out_faces[3 * f + 1] = faces[3 * f + (fl ? 2 : 1)];
    out_faces[3 * f + 2] = faces[3 * f + (fl ? 1 : 2)];
    if (uvs) {
      const float2* in = reinterpret_cast<const float2*>(uvs) + 3 * f;
      float2* out = reinterpret_cast<float2*>(out_uvs) + 3 * f;
      out[0] = in[0];
      out[1] = in[fl ? 2 : 1];
      out[2] = in[fl ? 1 : 2];
    }
  }
  mrp_wave_add(ctr + MRC_FLIPPED, fl ? 1 : 0);
}

struct OrientLayout {
  size_t ctr, keys, sorted, vals, slot, live, par, root, rflags, cflag, rank, start, end, first, second, head, tail,
      flipc, tmp, tmp_bytes, total;
};

static void orient_buffers(long long F, OrientLayout* l) {     // (as weld_buffers)
  const size_t f = (size_t)F, n3 = 3 * f;
  const size_t chunks = (f + MR_CHUNK - 1) / MR_CHUNK;
  mt::Bump b;
  l->ctr = b.take(8 * MRC_N);
  l->keys = b.take(8 * n3);         // edge keys; then the component sort's keys and faces (4 x F u32)
  l->sorted = b.take(8 * n3);
  l->vals = b.take(4 * n3);
  l->slot = b.take(4 * n3);
  l->live = b.take(f);
  l->par = b.take(8 * f);
  l->root = b.take(8 * f);
  l->rflags = b.take(8 * f);
  l->cflag = b.take(4 * f);
  l->rank = b.take(4 * f);
  l->start = b.take(4 * f);
  l->end = b.take(4 * f);
  l->first = b.take(32 * f);
  l->second = b.take(16 * f);
  l->head = b.take(32 * chunks);
  l->tail = b.take(32 * chunks);
  l->flipc = b.take(f);
  l->tmp = b.o;
}

static int orient_layout(long long F, OrientLayout* l) {
  orient_buffers(F, l);
  mt::TmpCounts cnt = {};
  cnt.pairs64 = 3 * (size_t)F;
  cnt.pairs32 = (size_t)F;
  cnt.xscan32 = (size_t)F;
  MT_TRY(mt::tmp_bytes(cnt, &l->tmp_bytes));
  l->total = l->tmp + mt::align(l->tmp_bytes);
  return VSA_OK;
}

// The (V, F) of the orient entry: the 2 F nodes of the double cover are what has to fit.
static int orient_check_vf(long long V, long long F) {
  if (V < 1 || F < 1) return VSA_ERR_ARG;
  if (F > 0x3FFFFFFFll) return VSA_ERR_UNSUPPORTED;
  return mt::check_vf(V, 2 * F);
}

extern "C" long long vsa_mesh_orient_workspace_bytes(long long nr_verts, long long nr_faces) {
  OrientLayout l;
  int rc = orient_check_vf(nr_verts, nr_faces);
  if (rc == VSA_OK) rc = mt::abi_status(orient_layout(nr_faces, &l));
  return rc != VSA_OK ? rc : (long long)l.total;
}

extern "C" int vsa_mesh_orient(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                               int outward, const float* faces_uvs, void* workspace, long long workspace_bytes,
                               int32_t* out_faces, float* out_faces_uvs, uint8_t* out_flipped, int32_t* out_component,
                               long long* stats, float* stage_ms, void* stream) {
  if (!verts || !faces || !workspace || !out_faces || !out_flipped || !out_component || !stats) return VSA_ERR_ARG;
  if (faces_uvs && !out_faces_uvs) return VSA_ERR_ARG;
  int rc = orient_check_vf(nr_verts, nr_faces);
  if (rc != VSA_OK) return rc;
  OrientLayout l;
  orient_buffers(nr_faces, &l);
  if (workspace_bytes < (long long)l.tmp + 16) return VSA_ERR_ARG;
  MT_TRY(mt::abi_status(orient_layout(nr_faces, &l)));
  if (workspace_bytes < (long long)l.total) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const long long F = nr_faces, n3 = 3 * F;
  char* ws = static_cast<char*>(workspace);
  const mt::Tmp tmp = {ws + l.tmp, l.tmp_bytes};
  long long* ctr = at<long long>(ws, l.ctr);
  u64* sorted = at<u64>(ws, l.sorted);
  uint32_t* slot = at<uint32_t>(ws, l.slot);
  uint8_t* live = at<uint8_t>(ws, l.live);
  int32_t* par = at<int32_t>(ws, l.par);
  int32_t* root = at<int32_t>(ws, l.root);
  int32_t* cflag = at<int32_t>(ws, l.cflag);
  int32_t* rank = at<int32_t>(ws, l.rank);
  int32_t* start = at<int32_t>(ws, l.start);
  int32_t* end = at<int32_t>(ws, l.end);
  double* first = at<double>(ws, l.first);
  double* second = at<double>(ws, l.second);
  double* head = at<double>(ws, l.head);
  double* tail = at<double>(ws, l.tail);
  uint8_t* flipc = at<uint8_t>(ws, l.flipc);
  uint32_t* kin = at<uint32_t>(ws, l.keys);
  uint32_t *kout = kin + F, *fin = kin + 2 * F, *fout = kin + 3 * F;
  mt::StageTimer timer;
  MT_TRY(timer.create(stage_ms, MRO_STAGES, st));
  auto run = [&]() -> int {
    VSA_HIP_TRY(hipMemsetAsync(ctr, 0, 8 * MRC_N, st));
    MT_TRY(timer.open());
    hipLaunchKernelGGL(mro_live, mt::grid(F), dim3(MR_BLOCK), 0, st, verts, faces, F, live);
    MT_LAUNCHED();
    MT_TRY(mt::sorted_edges(faces, F, mt::bits_of(nr_verts), at<u64>(ws, l.keys), sorted, at<uint32_t>(ws, l.vals), slot,
                            tmp, st));
    MT_TRY(timer.close(SO_EDGES));
    MT_TRY(timer.open());
    MT_TRY(mt::iota(par, 2 * F, st));
    hipLaunchKernelGGL(mro_hook, mt::grid(n3), dim3(MR_BLOCK), 0, st, sorted, slot, n3, faces, live, par);
    MT_LAUNCHED();
    MT_TRY(timer.close(SO_HOOK));
    MT_TRY(timer.open());
    MT_TRY(mt::roots(par, 2 * F, root, at<int32_t>(ws, l.rflags), st));
    hipLaunchKernelGGL(mro_component_flags, mt::grid(F), dim3(MR_BLOCK), 0, st, root, F, cflag);
    MT_LAUNCHED();
    MT_TRY(mt::exclusive_scan(tmp, cflag, rank, (size_t)F, st));
    hipLaunchKernelGGL(mro_sort_pairs, mt::grid(F), dim3(MR_BLOCK), 0, st, root, cflag, rank, F, kin, fin, out_component,
                       ctr);
    MT_LAUNCHED();
    MT_TRY(timer.close(SO_ROOTS));
    MT_TRY(timer.open());
    MT_TRY(mt::sort_pairs(tmp, kin, kout, fin, fout, (size_t)F, 0, mt::bits_of(F), st));
    hipLaunchKernelGGL(mro_ranges, mt::grid(F), dim3(MR_BLOCK), 0, st, kout, F, start, end);
    MT_LAUNCHED();
    const long long chunks = (F + MR_CHUNK - 1) / MR_CHUNK;
    hipLaunchKernelGGL((mro_sum_chunks<1, 4>), dim3((unsigned)chunks), dim3(MR_BLOCK), 0, st, verts, faces, root,
                       (const double*)nullptr, kout, fout, F, start, end, first, head, tail);
    MT_LAUNCHED();
    if (chunks > 1) {
      hipLaunchKernelGGL((mro_sum_spans<4>), dim3((unsigned)(chunks - 1)), dim3(VSA_WAVE), 0, st, kout, start, end, head,
                         tail, first);
      MT_LAUNCHED();
    }
    hipLaunchKernelGGL((mro_sum_chunks<2, 2>), dim3((unsigned)chunks), dim3(MR_BLOCK), 0, st, verts, faces, root, first,
                       kout, fout, F, start, end, second, head, tail);
    MT_LAUNCHED();
    if (chunks > 1) {
      hipLaunchKernelGGL((mro_sum_spans<2>), dim3((unsigned)(chunks - 1)), dim3(VSA_WAVE), 0, st, kout, start, end, head,
                         tail, second);
      MT_LAUNCHED();
    }
    MT_TRY(timer.close(SO_SUMS));
    MT_TRY(timer.open());
    hipLaunchKernelGGL(mro_decide, mt::grid(F), dim3(MR_BLOCK), 0, st, root, fout, start, end, second, F,
                       outward != 0, flipc, ctr);
    MT_LAUNCHED();
    hipLaunchKernelGGL(mro_flip, mt::grid(F), dim3(MR_BLOCK), 0, st, faces, F, root, rank, flipc, faces_uvs, out_faces,
                       out_faces_uvs, out_flipped, ctr);
    MT_LAUNCHED();
    long long host[MRC_N];
    MT_TRY(mt::read_counters(st, ctr, host, MRC_N));      // the one blocking read
    MT_TRY(timer.close(SO_FLIP));
    stats[0] = host[MRC_COMPONENTS];
    stats[1] = host[MRC_FLIPPED];
    stats[2] = host[MRC_UNORIENTABLE];
    stats[3] = host[MRC_UNDECIDED];
    stats[4] = host[MRC_UNDECIDED_FACES];
    return VSA_OK;
  };
  rc = run();
  timer.destroy();
  return rc;
}
