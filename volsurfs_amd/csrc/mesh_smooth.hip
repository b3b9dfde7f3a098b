// Smooth one shell: Taubin's lambda | mu fairing, with a guard that keeps it from crossing its neighbours.  (The
// reference has no such stage: the rule is this library's own -- include/volsurfs_hip.h "Mesh smoothing", DESIGN §37:
// restated in tests/mesh_smooth_restated.py, unpinned.)
//
// vsa_mesh_smooth_prepare, once per call: the vertex rings and the sorted edge keys of mesh_topology.hip, then
//   msm_boundary: one lane per sorted key; a key with no equal neighbour flags its two endpoints (plain stores of 1).
// vsa_mesh_smooth_step: msm_step, one lane per vertex.  The lane walks its ring in vff (contiguous, ascending corner
//   slot) and sums the two other corners of every slot in exactly that order -- no reduction across lanes and no float
//   atomics: the order is the contract.  Every vertex reads src and writes dst (Jacobi).  stuck leaves as one integer
//   atomic per wave.  The unguarded path is 2 x iterations of these launches and nothing else.
// vsa_mesh_smooth_guard: msm_guard, one lane per face of the moving mesh, one wave per workgroup.  A face with a vertex
//   whose bits differ from P walks each guard's q16 tree (cross_guards_hit of cross_walk.h, vsa_simplify_guarded's
//   guard block and loop: LDS stack, the wave kept together by ballots, no scratch); after its first crossing it walks
//   no further guard -- a verdict, not a count -- and stamps its three vertices with the round number (racing stores
//   of one value).  After an iteration's first round only a face with a vertex stamped in the round before can have a
//   new verdict: the others are as they were when they were found clear.
// vsa_mesh_smooth_revert: msm_revert, one lane per vertex.  A vertex stamped this round and still different from P is
//   restored; the newly reverted count leaves as one integer atomic per wave.
// Integers and a fixed fp32 order throughout: the same inputs give the same bytes.
#include "cross_walk.h"
#include "mesh_topology.h"

namespace {

struct MsmLayout {
  size_t boundary, stamp, vstart, vend, vff, kin, kout, vin, keys, sorted, tmp, tmp_bytes, total;
};

// The buffers, then rocPRIM's temporary storage: `query` = false leaves the size query out and counts its 16-byte
// minimum, a lower bound of the total that needs no device.
int msm_layout(long long V, long long F, bool query, MsmLayout* l) {
  const size_t n3 = 3 * (size_t)F;
  mt::Bump b;
  l->boundary = b.take(4 * (size_t)V);
  l->stamp = b.take(4 * (size_t)V);
  l->vstart = b.take(4 * (size_t)V);
  l->vend = b.take(4 * (size_t)V);
  l->vff = b.take(4 * n3);
  l->kin = b.take(4 * n3);
  l->kout = b.take(4 * n3);
  l->vin = b.take(4 * n3);
  l->keys = b.take(8 * n3);
  l->sorted = b.take(8 * n3);
  mt::TmpCounts n = {};
  n.pairs32 = n3;
  n.keys64 = n3;
  l->tmp_bytes = 16;
  if (query) MT_TRY(mt::tmp_bytes(n, &l->tmp_bytes));
  l->tmp = b.take(l->tmp_bytes);
  l->total = b.o;
  return VSA_OK;
}

// The checks every entry point makes of (V, F, workspace) before it touches the device.
int msm_bind(long long V, long long F, void* workspace, long long workspace_bytes, MsmLayout* l) {
  if (!workspace) return VSA_ERR_ARG;
  MT_TRY(mt::check_vf(V, F));
  MT_TRY(msm_layout(V, F, false, l));
  if (workspace_bytes < (long long)l->total) return VSA_ERR_ARG;
  MT_TRY(mt::abi_status(msm_layout(V, F, true, l)));
  if (workspace_bytes < (long long)l->total) return VSA_ERR_ARG;
  return VSA_OK;
}

__device__ __forceinline__ bool msm_same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

__global__ __launch_bounds__(MT_BLOCK) void msm_boundary(const mt::u64* __restrict__ sorted, long long n3, int s,
                                                        int32_t* __restrict__ boundary) {
  const long long i = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= n3) return;
  const mt::u64 k = sorted[i];
  if ((i > 0 && sorted[i - 1] == k) || (i + 1 < n3 && sorted[i + 1] == k)) return;
  boundary[k >> s] = 1;
  boundary[k & ((1ull << s) - 1)] = 1;
}

__global__ __launch_bounds__(MT_BLOCK) void msm_step(const float* __restrict__ P, float* __restrict__ Q,
                                                    const int32_t* __restrict__ faces,
                                                    const uint32_t* __restrict__ vff,
                                                    const int32_t* __restrict__ vstart,
                                                    const int32_t* __restrict__ vend,
                                                    const int32_t* __restrict__ boundary, long long V, float w,
                                                    int fix_boundary, unsigned long long* __restrict__ state) {
  const long long v = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  bool stuck = false;
  if (v < V) {
    const float px = P[3 * v], py = P[3 * v + 1], pz = P[3 * v + 2];
    float qx = px, qy = py, qz = pz;
    const int s = vstart[v], e = vend[v];
    if (e > s && !(fix_boundary && boundary[v])) {
      float ax = 0.f, ay = 0.f, az = 0.f;
      long long f1 = -1, f2 = -1;                   // the faces of the two slots before this one
      for (int j = s; j < e; ++j) {
        const long long f = vff[j];
        // a face that names v more than once sits in the ring once per corner, side by side: the slot's corner is the
        // match after those the earlier slots took
        int skip = (f == f1) + (f == f1 && f == f2);
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        int c = 2;
        if (i0 == v && skip-- == 0) c = 0;
        else if (i1 == v && skip-- == 0) c = 1;
        const long long a = c == 0 ? i1 : c == 1 ? i2 : i0, b = c == 0 ? i2 : c == 1 ? i0 : i1;
        ax = (ax + P[3 * a]) + P[3 * b];
        ay = (ay + P[3 * a + 1]) + P[3 * b + 1];
        az = (az + P[3 * a + 2]) + P[3 * b + 2];
        f2 = f1;
        f1 = f;
      }
      const float n = (float)(2ll * (e - s));
      const float cx = ax / n, cy = ay / n, cz = az / n;
      const float tx = w * (cx - px), ty = w * (cy - py), tz = w * (cz - pz);   // (a multiply, then an add)
      const float nx = px + tx, ny = py + ty, nz = pz + tz;
      if (fabsf(nx) < INFINITY && fabsf(ny) < INFINITY && fabsf(nz) < INFINITY) qx = nx, qy = ny, qz = nz;
      else stuck = true;
    }
    Q[3 * v] = qx, Q[3 * v + 1] = qy, Q[3 * v + 2] = qz;
  }
  const unsigned long long held = __builtin_amdgcn_ballot_w64(stuck);
  if ((threadIdx.x & 63) == 0 && held) atomicAdd(state, (unsigned long long)__popcll(held));
}

template <int STACK>
__global__ __launch_bounds__(TRACE_BLOCK) void msm_guard(const float* __restrict__ P, CrossMesh m, int first, int round,
                                                        int32_t* stamp, CrossGuards G) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const long long f = (long long)blockIdx.x * TRACE_BLOCK + lane;
  int id[3];
  const bool face = cross_face_ok(m, f, id[0], id[1], id[2]);
  CrossTri T;
  float x[3], y[3], z[3];
  // (a stamp of this round, stored by a lane that got here first, counts as one of the round before: the face is
  // then judged where it need not be, and its verdict is the same either way)
  bool moved = false, touched = round == first;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    cross_vertex(m, id[c], c, T, x, y, z);
    const long long v = id[c];
    touched = touched || stamp[v] >= round - 1;
    moved = moved || !msm_same_bits(x[c], P[3 * v]) || !msm_same_bits(y[c], P[3 * v + 1]) ||
            !msm_same_bits(z[c], P[3 * v + 2]);
  }
  bool bad = false;
  cross_guards_hit<STACK>(G, T, x, y, z, face && moved && touched, bad, s_node, lane);
  if (bad) stamp[id[0]] = round, stamp[id[1]] = round, stamp[id[2]] = round;
}

__global__ __launch_bounds__(MT_BLOCK) void msm_revert(const float* __restrict__ P, float* __restrict__ Q, long long V,
                                                      int round, const int32_t* __restrict__ stamp,
                                                      unsigned long long* __restrict__ state) {
  const long long v = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  bool back = false;
  if (v < V && stamp[v] == round) {
    const float px = P[3 * v], py = P[3 * v + 1], pz = P[3 * v + 2];
    back = !msm_same_bits(Q[3 * v], px) || !msm_same_bits(Q[3 * v + 1], py) || !msm_same_bits(Q[3 * v + 2], pz);
    if (back) Q[3 * v] = px, Q[3 * v + 1] = py, Q[3 * v + 2] = pz;
  }
  const unsigned long long went = __builtin_amdgcn_ballot_w64(back);
  if ((threadIdx.x & 63) == 0 && went) atomicAdd(state, (unsigned long long)__popcll(went));
}

}  // namespace

extern "C" long long vsa_mesh_smooth_workspace_bytes(long long nr_verts, long long nr_faces) {
  MT_TRY(mt::check_vf(nr_verts, nr_faces));
  MsmLayout l;
  MT_TRY(mt::abi_status(msm_layout(nr_verts, nr_faces, true, &l)));
  return (long long)l.total;
}

extern "C" int vsa_mesh_smooth_prepare(const int32_t* faces, long long nr_verts, long long nr_faces, void* workspace,
                                       long long workspace_bytes, void* stream) {
  if (!faces) return VSA_ERR_ARG;
  MsmLayout l;
  MT_TRY(msm_bind(nr_verts, nr_faces, workspace, workspace_bytes, &l));
  const hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  const int s = mt::bits_of(nr_verts);
  const mt::Tmp tmp = {ws + l.tmp, l.tmp_bytes};
  MT_TRY(mt::vertex_rings(faces, nr_faces, nr_verts, s, mt::at<uint32_t>(ws, l.kin), mt::at<uint32_t>(ws, l.kout),
                          mt::at<uint32_t>(ws, l.vin), mt::at<uint32_t>(ws, l.vff), mt::at<int32_t>(ws, l.vstart),
                          mt::at<int32_t>(ws, l.vend), tmp, st));
  MT_TRY(mt::sorted_edges(faces, nr_faces, s, mt::at<mt::u64>(ws, l.keys), mt::at<mt::u64>(ws, l.sorted), nullptr,
                          nullptr, tmp, st));
  VSA_HIP_TRY(hipMemsetAsync(ws + l.boundary, 0, 4 * (size_t)nr_verts, st));
  VSA_HIP_TRY(hipMemsetAsync(ws + l.stamp, 0xff, 4 * (size_t)nr_verts, st));   // -1: below every round
  hipLaunchKernelGGL(msm_boundary, mt::grid(3 * nr_faces), dim3(MT_BLOCK), 0, st, mt::at<mt::u64>(ws, l.sorted),
                     3 * nr_faces, s, mt::at<int32_t>(ws, l.boundary));
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_mesh_smooth_step(const float* src, float* dst, const int32_t* faces, long long nr_verts,
                                    long long nr_faces, int half, float weight, int fix_boundary,
                                    const void* workspace, long long workspace_bytes, long long* state, void* stream) {
  if (!src || !dst || !faces || !state || src == dst) return VSA_ERR_ARG;
  if (!(fabsf(weight) < INFINITY)) return VSA_ERR_ARG;                        // inf or NaN
  if (half == 0 ? !(weight > 0.0f && weight <= 1.0f) : half == 1 ? weight > 0.0f : true) return VSA_ERR_ARG;
  MsmLayout l;
  MT_TRY(msm_bind(nr_verts, nr_faces, const_cast<void*>(workspace), workspace_bytes, &l));
  char* ws = static_cast<char*>(const_cast<void*>(workspace));
  hipLaunchKernelGGL(msm_step, mt::grid(nr_verts), dim3(MT_BLOCK), 0, (hipStream_t)stream, src, dst, faces,
                     mt::at<uint32_t>(ws, l.vff), mt::at<int32_t>(ws, l.vstart), mt::at<int32_t>(ws, l.vend),
                     mt::at<int32_t>(ws, l.boundary), nr_verts, weight, fix_boundary != 0,
                     reinterpret_cast<unsigned long long*>(state));
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_mesh_smooth_guard(const float* before, const float* after, const int32_t* faces, long long nr_verts,
                                     long long nr_faces, int nr_guards, const uint32_t* const* guard_qnodes,
                                     const float* const* guard_tris, const int32_t* guard_roots,
                                     const float* guard_frames, const int32_t* guard_max_depths,
                                     const float* const* guard_vertices, const long long* guard_nr_verts,
                                     const int32_t* const* guard_faces, const long long* guard_nr_faces, int first_round,
                                     int round, void* workspace, long long workspace_bytes, void* stream) {
  if (!before || !after || !faces || first_round < 0 || round < first_round) return VSA_ERR_ARG;
  CrossGuards G;
  MT_TRY(cross_guards_bind(nr_guards, guard_qnodes, guard_tris, guard_roots, guard_frames, guard_max_depths,
                           guard_vertices, guard_nr_verts, guard_faces, guard_nr_faces, &G));
  MsmLayout l;
  MT_TRY(msm_bind(nr_verts, nr_faces, workspace, workspace_bytes, &l));
  char* ws = static_cast<char*>(workspace);
  const CrossMesh m = {after, faces, nr_verts, nr_faces};
  const dim3 grid((unsigned)((nr_faces + TRACE_BLOCK - 1) / TRACE_BLOCK)), block(TRACE_BLOCK);
  with_stack(G.max_depth, [&](auto sk) {
    hipLaunchKernelGGL((msm_guard<decltype(sk)::value>), grid, block, 0, (hipStream_t)stream, before, m, first_round,
                       round, mt::at<int32_t>(ws, l.stamp), G);
  });
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_mesh_smooth_revert(const float* before, float* after, long long nr_verts, long long nr_faces,
                                      int round, const void* workspace, long long workspace_bytes, long long* state,
                                      void* stream) {
  if (!before || !after || !state || round < 0) return VSA_ERR_ARG;
  MsmLayout l;
  MT_TRY(msm_bind(nr_verts, nr_faces, const_cast<void*>(workspace), workspace_bytes, &l));
  char* ws = static_cast<char*>(const_cast<void*>(workspace));
  hipLaunchKernelGGL(msm_revert, mt::grid(nr_verts), dim3(MT_BLOCK), 0, (hipStream_t)stream, before, after, nr_verts,
                     round, mt::at<int32_t>(ws, l.stamp), reinterpret_cast<unsigned long long*>(state));
  VSA_RETURN_LAUNCH_STATUS();
}
