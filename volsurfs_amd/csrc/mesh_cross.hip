// Which faces of two meshes cross, exactly?  (The reference has no such stage: the rule is this library's own --
// include/volsurfs_hip.h "Mesh crossings", DESIGN §33: restated in tests/mesh_intersect_restated.py, unpinned.)
//
// vsa_mesh_cross_count: one lane per query face walks the other mesh's q16 tree by box overlap (cross_walk.h) and
// applies the triangle-triangle rule in fp64 to every face of the leaves it reaches: the number of faces it crosses
// per query face (one store), the number of query faces that cross it per tree face (one integer atomicAdd per
// crossing), the exclusive scan of the numbers of pairs the emit pass will write, and their total.
// vsa_mesh_cross_emit: the same walk, writing (query face, tree face) -- and the pair's segment -- at the query's
// offset; then a radix sort of the 64-bit keys (csrc/mesh_topology.hip) and a gather, so that the pairs leave sorted by
// (query face, tree face) whatever the tree's builder and leaf order.  Integers and a fixed fp64 order throughout: the
// same inputs give the same bytes.
#include "cross_walk.h"
#include "mesh_topology.h"

namespace {

struct CrossFrame {
  float f[6];
};

struct CrossArgs {
  const uint4* qnodes;
  const float4* tris;
  int root;
  CrossFrame frame;
  CrossMesh tree, query;
  const int32_t* order;       // lane i takes query face order[i]; null: face i
  // count pass
  int32_t* count_query;
  int32_t* count_tree;
  int32_t* count_emit;        // self mode: the partners above the face; else null (= count_query)
  unsigned long long* total;
  // emit pass
  const int32_t* offsets;
  long long nr_pairs;
  unsigned long long* keys;
  uint32_t* vals;
  double* segs;
};

// The lane's query face: its index (-1: none), its triangle and its box in the tree's grid.  A face with an index out
// of range or a NaN coordinate crosses nothing: the lane does not walk.
__device__ __forceinline__ int cross_query(const CrossArgs& a, long long i, CrossTri& Q, CrossBox& qb) {
  if (i >= a.query.F) return -1;
  const long long f = a.order ? a.order[i] : i;
  int i0, i1, i2;
  if (!cross_face_ok(a.query, f, i0, i1, i2)) return -1;
  float x[3], y[3], z[3];
  cross_vertex(a.query, i0, 0, Q, x, y, z);
  cross_vertex(a.query, i1, 1, Q, x, y, z);
  cross_vertex(a.query, i2, 2, Q, x, y, z);
  bool numbers = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) numbers = numbers && x[k] == x[k] && y[k] == y[k] && z[k] == z[k];
  if (!numbers) return -1;
  qb = cross_qbox(a.frame.f, x, y, z);
  return (int)f;
}

template <int STACK, bool SELF>
__global__ __launch_bounds__(TRACE_BLOCK) void cross_count_kernel(CrossArgs a) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  const int lane = threadIdx.x;
  CrossTri Q;
  CrossBox qb;
  const int face = cross_query(a, (long long)blockIdx.x * TRACE_BLOCK + lane, Q, qb);
  int n = 0, up = 0;
  cross_walk<STACK, SELF, false, false>(a.qnodes, a.tris, a.tree, Q, qb, face, face >= 0 ? a.root : TRACE_EMPTY, s_node,
                                        lane, [&](int other, const double*) {
                                          ++n;
                                          if (SELF) up += other > face;
                                          else atomicAdd(a.count_tree + other, 1);
                                        });
  if (face >= 0) {
    a.count_query[face] = n;
    if (SELF) a.count_emit[face] = up;
  }
  int t = SELF ? up : n;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m);
  if (lane == 0 && t) atomicAdd(a.total, (unsigned long long)t);
}

template <int STACK, bool SELF, bool SEG>
__global__ __launch_bounds__(TRACE_BLOCK) void cross_emit_kernel(CrossArgs a) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  const int lane = threadIdx.x;
  CrossTri Q;
  CrossBox qb;
  const int face = cross_query(a, (long long)blockIdx.x * TRACE_BLOCK + lane, Q, qb);
  long long pos = face >= 0 ? a.offsets[face] : 0;
  cross_walk<STACK, SELF, true, SEG>(a.qnodes, a.tris, a.tree, Q, qb, face, face >= 0 ? a.root : TRACE_EMPTY, s_node,
                                     lane, [&](int other, const double* seg) {
                                       if (pos < 0 || pos >= a.nr_pairs) return;      // (offsets of another call)
                                       a.keys[pos] = (unsigned long long)(unsigned)face << 32 | (unsigned)other;
                                       a.vals[pos] = (uint32_t)pos;
                                       if constexpr (SEG) {
#pragma unroll
                                         for (int c = 0; c < 6; ++c) a.segs[6 * pos + c] = seg[c];
                                       }
                                       ++pos;
                                     });
}

__global__ __launch_bounds__(MT_BLOCK) void cross_gather_kernel(const unsigned long long* __restrict__ keys,
                                                                const uint32_t* __restrict__ vals,
                                                                const double* __restrict__ segs_in, long long n,
                                                                long long* __restrict__ pairs,
                                                                double* __restrict__ segs_out) {
  const long long i = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  pairs[2 * i] = (long long)(k >> 32);
  pairs[2 * i + 1] = (long long)(k & 0xffffffffull);
  if (segs_out) {
    const long long s = vals[i];
#pragma unroll
    for (int c = 0; c < 6; ++c) segs_out[6 * i + c] = segs_in[6 * s + c];
  }
}

struct CountLayout {
  size_t emit, tmp, tmp_bytes, total;
};

int count_layout(long long Fq, CountLayout* L) {
  mt::TmpCounts c = {};
  c.xscan32 = (size_t)Fq;
  MT_TRY(mt::tmp_bytes(c, &L->tmp_bytes));
  mt::Bump b;
  L->emit = b.take(4 * (size_t)Fq);
  L->tmp = b.take(L->tmp_bytes);
  L->total = b.o;
  return VSA_OK;
}

struct EmitLayout {
  size_t keys, sorted, vals, vals_sorted, segs, tmp, tmp_bytes, total;
};

int emit_layout(long long P, bool segments, EmitLayout* L) {
  mt::TmpCounts c = {};
  c.pairs64 = (size_t)P;
  MT_TRY(mt::tmp_bytes(c, &L->tmp_bytes));
  mt::Bump b;
  L->keys = b.take(8 * (size_t)P);
  L->sorted = b.take(8 * (size_t)P);
  L->vals = b.take(4 * (size_t)P);
  L->vals_sorted = b.take(4 * (size_t)P);
  L->segs = b.take(segments ? 48 * (size_t)P : 0);
  L->tmp = b.take(L->tmp_bytes);
  L->total = b.o;
  return VSA_OK;
}

constexpr long long MAX_I32 = 0x7fffffffll;

// The status of the arguments the two passes share, before any HIP call.
int check_cross_args(const uint32_t* qnodes, const float* tris, int root, const float* frame, int max_depth,
                     const float* tree_vertices, long long nr_tree_verts, const int32_t* tree_faces,
                     long long nr_tree_faces, const float* query_vertices, long long nr_query_verts,
                     const int32_t* query_faces, long long nr_query_faces, int self_mode) {
  if (const int rc = check_qtree(qnodes, tris, &root, frame, 1, max_depth, VSA_ERR_ARG)) return rc;
  if (root < 0 || !tree_vertices || !tree_faces || !query_vertices || !query_faces) return VSA_ERR_ARG;
  if (nr_tree_verts < 1 || nr_tree_faces < 1 || nr_query_verts < 1 || nr_query_faces < 1) return VSA_ERR_ARG;
  if (self_mode != 0 && self_mode != 1) return VSA_ERR_ARG;
  if (self_mode && (nr_query_faces != nr_tree_faces || nr_query_verts != nr_tree_verts)) return VSA_ERR_ARG;
  if (nr_tree_verts > MAX_I32 || nr_query_verts > MAX_I32 || nr_tree_faces > MAX_I32 / 3 - 1 ||
      nr_query_faces > MAX_I32 / 3 - 1)
    return VSA_ERR_UNSUPPORTED;
  return VSA_OK;
}

CrossArgs make_args(const uint32_t* qnodes, const float* tris, int root, const float* frame,
                    const float* tree_vertices, long long nr_tree_verts, const int32_t* tree_faces,
                    long long nr_tree_faces, const float* query_vertices, long long nr_query_verts,
                    const int32_t* query_faces, long long nr_query_faces, const int32_t* query_order) {
  CrossArgs a = {};
  a.qnodes = reinterpret_cast<const uint4*>(qnodes);
  a.tris = reinterpret_cast<const float4*>(tris);
  a.root = root;
  for (int j = 0; j < 6; ++j) a.frame.f[j] = frame[j];
  a.tree = CrossMesh{tree_vertices, tree_faces, nr_tree_verts, nr_tree_faces};
  a.query = CrossMesh{query_vertices, query_faces, nr_query_verts, nr_query_faces};
  a.order = query_order;
  return a;
}

}  // namespace

extern "C" long long vsa_mesh_cross_workspace_bytes(long long nr_query_faces, long long nr_pairs, int segments) {
  if (nr_query_faces < 1 || nr_pairs < 0) return VSA_ERR_ARG;
  if (nr_query_faces > MAX_I32 / 3 - 1 || nr_pairs > MAX_I32) return VSA_ERR_UNSUPPORTED;
  CountLayout C;
  int rc = count_layout(nr_query_faces, &C);
  if (rc != VSA_OK) return mt::abi_status(rc);
  size_t total = C.total;
  if (nr_pairs > 0) {
    EmitLayout E;
    rc = emit_layout(nr_pairs, segments != 0, &E);
    if (rc != VSA_OK) return mt::abi_status(rc);
    total = total > E.total ? total : E.total;
  }
  return (long long)total;
}

extern "C" int vsa_mesh_cross_count(const uint32_t* qnodes, const float* tris, int root, const float* frame,
                                    int max_depth, const float* tree_vertices, long long nr_tree_verts,
                                    const int32_t* tree_faces, long long nr_tree_faces, const float* query_vertices,
                                    long long nr_query_verts, const int32_t* query_faces, long long nr_query_faces,
                                    const int32_t* query_order, int self_mode, int32_t* count_query,
                                    int32_t* count_tree, int32_t* offsets, long long* total, void* workspace,
                                    long long workspace_bytes, void* stream) {
  MT_TRY(check_cross_args(qnodes, tris, root, frame, max_depth, tree_vertices, nr_tree_verts, tree_faces, nr_tree_faces,
                          query_vertices, nr_query_verts, query_faces, nr_query_faces, self_mode));
  if (!count_query || (!self_mode && !count_tree) || !offsets || !total || !workspace) return VSA_ERR_ARG;
  CountLayout L;
  MT_TRY(mt::abi_status(count_layout(nr_query_faces, &L)));
  if (workspace_bytes < (long long)L.total) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  CrossArgs a = make_args(qnodes, tris, root, frame, tree_vertices, nr_tree_verts, tree_faces, nr_tree_faces,
                          query_vertices, nr_query_verts, query_faces, nr_query_faces, query_order);
  a.count_query = count_query;
  a.count_tree = count_tree;
  a.count_emit = self_mode ? mt::at<int32_t>(ws, L.emit) : nullptr;
  a.total = reinterpret_cast<unsigned long long*>(total);
  VSA_HIP_TRY(hipMemsetAsync(count_query, 0, 4 * (size_t)nr_query_faces, st));
  if (self_mode) VSA_HIP_TRY(hipMemsetAsync(a.count_emit, 0, 4 * (size_t)nr_query_faces, st));
  else VSA_HIP_TRY(hipMemsetAsync(count_tree, 0, 4 * (size_t)nr_tree_faces, st));
  VSA_HIP_TRY(hipMemsetAsync(total, 0, 8, st));
  const dim3 grid((unsigned)((nr_query_faces + TRACE_BLOCK - 1) / TRACE_BLOCK)), block(TRACE_BLOCK);
  with_stack(max_depth, [&](auto sk) {
    with_flag(self_mode != 0, [&](auto sf) {
      hipLaunchKernelGGL((cross_count_kernel<decltype(sk)::value, decltype(sf)::value>), grid, block, 0, st, a);
    });
  });
  MT_LAUNCHED();
  return mt::exclusive_scan({ws + L.tmp, L.tmp_bytes}, self_mode ? a.count_emit : count_query, offsets,
                            (size_t)nr_query_faces, st);
}

extern "C" int vsa_mesh_cross_emit(const uint32_t* qnodes, const float* tris, int root, const float* frame,
                                   int max_depth, const float* tree_vertices, long long nr_tree_verts,
                                   const int32_t* tree_faces, long long nr_tree_faces, const float* query_vertices,
                                   long long nr_query_verts, const int32_t* query_faces, long long nr_query_faces,
                                   const int32_t* query_order, int self_mode, const int32_t* offsets,
                                   long long nr_pairs, long long* pairs, double* segments, void* workspace,
                                   long long workspace_bytes, void* stream) {
  MT_TRY(check_cross_args(qnodes, tris, root, frame, max_depth, tree_vertices, nr_tree_verts, tree_faces, nr_tree_faces,
                          query_vertices, nr_query_verts, query_faces, nr_query_faces, self_mode));
  if (!offsets || !pairs || !workspace || nr_pairs < 1) return VSA_ERR_ARG;
  if (nr_pairs > MAX_I32) return VSA_ERR_UNSUPPORTED;
  EmitLayout L;
  MT_TRY(mt::abi_status(emit_layout(nr_pairs, segments != nullptr, &L)));
  if (workspace_bytes < (long long)L.total) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  CrossArgs a = make_args(qnodes, tris, root, frame, tree_vertices, nr_tree_verts, tree_faces, nr_tree_faces,
                          query_vertices, nr_query_verts, query_faces, nr_query_faces, query_order);
  a.offsets = offsets;
  a.nr_pairs = nr_pairs;
  a.keys = mt::at<unsigned long long>(ws, L.keys);
  a.vals = mt::at<uint32_t>(ws, L.vals);
  a.segs = segments ? mt::at<double>(ws, L.segs) : nullptr;
  // (a slot the walk does not reach -- offsets that are not this call's count pass's -- sorts last as (-1, -1))
  VSA_HIP_TRY(hipMemsetAsync(a.keys, 0xff, 8 * (size_t)nr_pairs, st));
  VSA_HIP_TRY(hipMemsetAsync(a.vals, 0, 4 * (size_t)nr_pairs, st));
  const dim3 grid((unsigned)((nr_query_faces + TRACE_BLOCK - 1) / TRACE_BLOCK)), block(TRACE_BLOCK);
  with_stack(max_depth, [&](auto sk) {
    with_flag(self_mode != 0, [&](auto sf) {
      with_flag(segments != nullptr, [&](auto sg) {
        hipLaunchKernelGGL((cross_emit_kernel<decltype(sk)::value, decltype(sf)::value, decltype(sg)::value>), grid,
                           block, 0, st, a);
      });
    });
  });
  MT_LAUNCHED();
  mt::u64* sorted = mt::at<mt::u64>(ws, L.sorted);
  uint32_t* vals_sorted = mt::at<uint32_t>(ws, L.vals_sorted);
  MT_TRY(mt::sort_pairs({ws + L.tmp, L.tmp_bytes}, a.keys, sorted, a.vals, vals_sorted, (size_t)nr_pairs, 0,
                        32 + mt::bits_of(nr_query_faces), st));
  hipLaunchKernelGGL(cross_gather_kernel, mt::grid(nr_pairs), dim3(MT_BLOCK), 0, st, sorted, vals_sorted, a.segs,
                     nr_pairs, pairs, segments);
  VSA_RETURN_LAUNCH_STATUS();
}
