// Move the vertices of one shell until it clears its neighbour.  (The reference has no such stage: the rule is this
// library's own -- include/volsurfs_hip.h "Shell untangling", DESIGN §34: restated in tests/shell_untangle_restated.py,
// unpinned.)
//
// One round of the loop of volsurfs_amd/shell_untangle.py is three launches and one read: the project kernel below, the
// crossing count pass of csrc/mesh_cross.hip (the moving shell's faces against the fixed shell's tree), the escalate
// kernel below; the four words of `state` are what the host reads.
// vsa_shell_untangle_project: one lane per vertex of the moving shell M.  The lane walks the fixed shell X's q16 tree
//   with the closest-point walk (closest_walk.h: LDS stack, no scratch), takes the sign as vsa_signed_distance_q does
//   (the pseudonormal of the closest feature) or as vsa_signed_distance_w_q does (the winding walk, winding_walk.h),
//   and -- all in registers -- tests the vertex against its margin and moves it along the residual (or the pseudonormal
//   where it lies on X).  The vertex is written in place; dist, slot and the weights never go to memory.  moved, stuck
//   and max |t| are reduced in the wave, then one integer atomic per wave and word.
// vsa_shell_untangle_escalate: one lane per face of M.  A face the count pass found crossing stamps its three vertices
//   with the round number (atomicMax); the lane that raises a stamp raises the vertex's level, so a vertex is raised
//   once per round however many of its faces cross, and the stamps need no clearing.
// Integers and a fixed fp32 order throughout, no float atomics: the same inputs give the same bytes.
#include "cross_walk.h"
#include "mesh_topology.h"
#include "winding_walk.h"

namespace {

constexpr long long MAX_GRID = 0x7fffffffll;
constexpr int MAX_LEVEL_CAP = 30;             // margin * 2^level is formed as margin * (float)(1 << level)
constexpr float OVERSHOOT = 1.25f;            // a step that lands exactly on the margin would flicker on the last ulp

struct UntangleFrame {
  float f[6];
};

struct ProjectArgs {
  const uint4* qnodes;
  const float4* tris;
  int root;
  UntangleFrame frame;
  const float* table;         // X's pseudonormals
  long long table_base;
  const float4* moments;      // X's winding moments (WINDING only)
  long long moment_root;
  float beta;
  float* vertices;            // M's, moved in place
  long long V;
  const int32_t* level;
  float side, margin;
  int max_level;
  unsigned long long* state;  // moved, stuck, bits of max |t|
};

template <int STACK, bool BOUNDS, bool WINDING>
__global__ __launch_bounds__(TRACE_BLOCK) void untangle_project_kernel(ProjectArgs a) {
  __shared__ int s_node[STACK][TRACE_BLOCK];
  __shared__ float s_bound[BOUNDS ? STACK : 1][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const long long i = (long long)blockIdx.x * TRACE_BLOCK + lane;
  const bool alive = i < a.V;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (alive) px = a.vertices[3 * i], py = a.vertices[3 * i + 1], pz = a.vertices[3 * i + 2];
  const int root = alive ? a.root : TRACE_EMPTY;
  const QPoint q = closest_qpoint(a.frame.f, px, py, pz);
  Closest best = no_closest();
  closest_walk<STACK, BOUNDS>(a.qnodes, a.tris, q, px, py, pz, root, best, s_node, s_bound, lane);
  float wn = 0.0f;
  if constexpr (WINDING)
    wn = winding_walk<STACK>(a.qnodes, a.tris, a.moments, root, a.moment_root, px, py, pz, a.beta, s_node, lane);
  bool moved = false, stuck = false;
  float abs_t = 0.0f;
  if (alive && best.slot >= 0) {                                  // (no closest record: a NaN vertex stays)
    const float dist = WINDING ? signed_by_winding(best, wn)
                               : signed_distance(a.tris, a.table, a.table_base, best, px, py, pz);
    const float m = a.margin * (float)(1 << min(a.level[i], a.max_level));
    if (a.side * dist < m) {
      const float t = a.side * (OVERSHOOT * m) - dist;
      const float ad = fabsf(dist);
      float gx, gy, gz;
      if (ad > 0.0f) {
        closest_residual(a.tris, best, px, py, pz, gx, gy, gz);
        gx /= ad, gy /= ad, gz /= ad;
        if (dist < 0.0f) gx = -gx, gy = -gy, gz = -gz;
      } else {
        const float* n = closest_pseudonormal(a.table, a.table_base, best);
        const float len = sqrtf(dot3(n[0], n[1], n[2], n[0], n[1], n[2]));
        gx = n[0] / len, gy = n[1] / len, gz = n[2] / len;
      }
      if (fabsf(gx) < INFINITY && fabsf(gy) < INFINITY && fabsf(gz) < INFINITY) {
        const float tx = t * gx, ty = t * gy, tz = t * gz;        // (a multiply, then an add: no contraction)
        float* out = a.vertices + 3 * i;
        out[0] = px + tx, out[1] = py + ty, out[2] = pz + tz;
        moved = true;
        abs_t = fabsf(t);
      } else {
        stuck = true;
      }
    }
  }
  const int nr_moved = __popcll(__builtin_amdgcn_ballot_w64(moved));
  const int nr_stuck = __popcll(__builtin_amdgcn_ballot_w64(stuck));
  unsigned top = __float_as_uint(abs_t);                          // (|t| >= 0, never NaN: its bits order as integers)
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) top = max(top, (unsigned)__shfl_xor((int)top, w));
  if (lane == 0) {
    if (nr_moved) atomicAdd(a.state, (unsigned long long)nr_moved);
    if (nr_stuck) atomicAdd(a.state + 1, (unsigned long long)nr_stuck);
    if (top) atomicMax(a.state + 2, (unsigned long long)top);
  }
}

__global__ __launch_bounds__(MT_BLOCK) void untangle_escalate_kernel(const int32_t* __restrict__ count, CrossMesh m,
                                                                     int round, int32_t* __restrict__ stamp,
                                                                     int32_t* __restrict__ level) {
  const long long f = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (f >= m.F || count[f] == 0) return;
  int v[3];
  if (!cross_face_ok(m, f, v[0], v[1], v[2])) return;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (atomicMax(stamp + v[k], round) < round) level[v[k]] += 1;   // (the one lane that raised the stamp)
}

struct Layout {
  size_t level, stamp, total;
};

Layout untangle_layout(long long V) {
  Layout l;
  mt::Bump b;
  l.level = b.take(4 * (size_t)V);
  l.stamp = b.take(4 * (size_t)V);
  l.total = b.o;
  return l;
}

}  // namespace

extern "C" long long vsa_shell_untangle_workspace_bytes(long long nr_verts) {
  if (nr_verts < 1) return VSA_ERR_ARG;
  if (nr_verts > MAX_GRID) return VSA_ERR_UNSUPPORTED;
  return (long long)untangle_layout(nr_verts).total;
}

extern "C" int vsa_shell_untangle_project(const uint32_t* qnodes, const float* tris, int root, const float* frame,
                                          int max_depth, const float* table, long long table_face_base,
                                          const float* moments, long long moment_root, float beta, float* vertices,
                                          long long nr_verts, int side, float margin, int max_level, int round,
                                          void* workspace, long long workspace_bytes, long long* state, void* stream) {
  if (const int rc = check_qtree(qnodes, tris, &root, frame, 1, max_depth, VSA_ERR_ARG)) return rc;
  if (!table || !vertices || !workspace || !state || root < 0 || table_face_base < 0 || nr_verts < 1) return VSA_ERR_ARG;
  if (side != 1 && side != -1) return VSA_ERR_ARG;
  if (!(margin > 0.0f) || !(margin < INFINITY)) return VSA_ERR_ARG;          // zero, negative, inf or NaN
  if (max_level < 0 || max_level > MAX_LEVEL_CAP || round < 0) return VSA_ERR_ARG;
  if (moments && (moment_root < 0 || !(beta > 1.0f))) return VSA_ERR_ARG;
  if (nr_verts > MAX_GRID) return VSA_ERR_UNSUPPORTED;
  const Layout l = untangle_layout(nr_verts);
  if (workspace_bytes < (long long)l.total) return VSA_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  if (round == 0) {                                                          // levels 0, stamps -1: below every round
    VSA_HIP_TRY(hipMemsetAsync(ws + l.level, 0, 4 * (size_t)nr_verts, st));
    VSA_HIP_TRY(hipMemsetAsync(ws + l.stamp, 0xff, 4 * (size_t)nr_verts, st));
  }
  VSA_HIP_TRY(hipMemsetAsync(state, 0, 24, st));
  ProjectArgs a = {};
  a.qnodes = reinterpret_cast<const uint4*>(qnodes);
  a.tris = reinterpret_cast<const float4*>(tris);
  a.root = root;
  for (int j = 0; j < 6; ++j) a.frame.f[j] = frame[j];
  a.table = table;
  a.table_base = table_face_base;
  a.moments = reinterpret_cast<const float4*>(moments);
  a.moment_root = moment_root;
  a.beta = beta;
  a.vertices = vertices;
  a.V = nr_verts;
  a.level = mt::at<int32_t>(ws, l.level);
  a.side = (float)side;
  a.margin = margin;
  a.max_level = max_level;
  a.state = reinterpret_cast<unsigned long long*>(state);
  const dim3 grid((unsigned)((nr_verts + TRACE_BLOCK - 1) / TRACE_BLOCK)), block(TRACE_BLOCK);
  with_stack(max_depth, [&](auto sk) {
    with_flag(closest_walk_bounds(max_depth), [&](auto bd) {
      with_flag(moments != nullptr, [&](auto wd) {
        hipLaunchKernelGGL((untangle_project_kernel<decltype(sk)::value, decltype(bd)::value, decltype(wd)::value>),
                           grid, block, 0, st, a);
      });
    });
  });
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_shell_untangle_escalate(const int32_t* count_query, const int32_t* faces, long long nr_faces,
                                           long long nr_verts, int round, void* workspace, long long workspace_bytes,
                                           void* stream) {
  if (!count_query || !faces || !workspace || nr_faces < 1 || nr_verts < 1 || round < 0) return VSA_ERR_ARG;
  if (nr_verts > MAX_GRID || nr_faces > MAX_GRID / 3 - 1) return VSA_ERR_UNSUPPORTED;
  const Layout l = untangle_layout(nr_verts);
  if (workspace_bytes < (long long)l.total) return VSA_ERR_ARG;
  char* ws = static_cast<char*>(workspace);
  const CrossMesh m = {nullptr, faces, nr_verts, nr_faces};
  hipLaunchKernelGGL(untangle_escalate_kernel, mt::grid(nr_faces), dim3(MT_BLOCK), 0, (hipStream_t)stream, count_query,
                     m, round, mt::at<int32_t>(ws, l.stamp), mt::at<int32_t>(ws, l.level));
  VSA_RETURN_LAUNCH_STATUS();
}
