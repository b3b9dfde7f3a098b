// Device-side BVH builder for the K shell meshes (build half, on the GPU).
//
// A Karras-style linear BVH (Karras 2012, "Maximizing parallelism in the construction of BVHs, octrees and
// k-d trees") built from the meshes' device arrays, emitted in exactly the node / triangle layouts of
// vsa_bvh_export and vsa_bvh_export_q (csrc/bvh_build.cpp), so the trace kernels run on it unchanged.
//
//   1. per triangle: box, centre (the host builder's centroid), block-partial triangle / centroid bounds;
//   2. one block reduces the partials: mesh bounds, the host's box padding;
//   3. 30-bit Morton code of the centroid on the centroid bounds' grid;
//   4. stable radix sort of (code, face id) — equal codes stay in face-id order: the build is deterministic;
//   5. the n - 1 internal nodes from the common-prefix lengths of neighbouring keys (duplicates split by
//      index), with the sorted range each covers and parent links;
//      vsa_bvh_dev_build_ploc puts PLOC clustering (csrc/bvh_ploc.hip) in its place: the same form (root 0, ranges,
//      parent links), leaf order = the PLOC tree's left-to-right order instead of the sorted order;
//   6. bottom-up: one thread per leaf climbs with one arrival counter per node, the second arrival
//      continues; it writes its un-padded box and its subtree's kept-internal-node count into the parent's
//      child slot.  Min / max do not depend on arrival order: the boxes are the same bits every build;
//   7. pre-order numbering of the kept internal nodes (a subtree of > leaf_size triangles; smaller ones
//      collapse into one leaf, the host rule `n <= leaf_size`), and the tree depth;
//   8. export: fp32 64-B nodes, q16 32-B nodes on the union of the root's child boxes, and the triangle
//      records in leaf order.
// Refit re-runs 1, 2 and 6 on moved vertices; slots and topology stay.
// Every closest hit is a minimum over (t, face id) and the boxes only prune, so hits through this tree are
// bit-identical to the host tree's and to brute force (tests/test_bvh_device.py).
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <cstdint>
#include <utility>

#include "bvh_ploc.h"
#include "common.h"

namespace {

constexpr int BVHD_BLOCK = 256;
constexpr int BVHD_MAX_PARTIALS = 1024;      // blocks of the set-up kernel (grid-stride beyond)
constexpr int BVHD_TRACE_STACK = 48;         // trace.hip: TRACE_STACK
constexpr int BVHD_MAX_CLIMB = 4096;         // bound of every upward walk (a tree is < 64 deep)

// info words (device, int32)
enum { INFO_ERR = 0, INFO_ROOT_NINT = 1, INFO_MAX_DEPTH = 2, INFO_WORDS = 4 };
enum { ERR_FACE_INDEX = 1, ERR_WALK = 2 };

// bnd (device, float): tri lo xyz, tri hi xyz, centroid lo xyz, centroid hi xyz, pad, frame[6]
enum { BND_TRI_LO = 0, BND_TRI_HI = 3, BND_CEN_LO = 6, BND_CEN_HI = 9, BND_PAD = 12, BND_FRAME = 16, BND_WORDS = 24 };

__device__ __forceinline__ int clamp_vertex(int32_t i, int nv, int32_t* info) {
  if (i < 0 || i >= nv) {
    atomicOr(&info[INFO_ERR], ERR_FACE_INDEX);
    return 0;
  }
  return i;
}

__device__ __forceinline__ void fetch_tri(const float* __restrict__ verts, const int32_t* __restrict__ faces, int nv,
                                          int f, int32_t* info, float a[3], float b[3], float c[3]) {
  const int ia = clamp_vertex(faces[3 * (size_t)f + 0], nv, info);
  const int ib = clamp_vertex(faces[3 * (size_t)f + 1], nv, info);
  const int ic = clamp_vertex(faces[3 * (size_t)f + 2], nv, info);
  for (int k = 0; k < 3; ++k) {
    a[k] = verts[3 * (size_t)ia + k];
    b[k] = verts[3 * (size_t)ib + k];
    c[k] = verts[3 * (size_t)ic + k];
  }
}

// host rule (bvh_build.cpp, Builder::padded): pad + 1e-6 * max|coord| per axis
__device__ __forceinline__ void pad_box(float lo[3], float hi[3], float pad) {
  for (int a = 0; a < 3; ++a) {
    const float e = pad + 1e-6f * fmaxf(fabsf(lo[a]), fabsf(hi[a]));
    lo[a] = lo[a] - e;
    hi[a] = hi[a] + e;
  }
}

__device__ __forceinline__ int delta(const uint32_t* __restrict__ keys, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const uint32_t a = keys[i], b = keys[j];
  if (a == b) return 32 + __clz((uint32_t)(i ^ j));
  return __clz(a ^ b);
}

__device__ __forceinline__ uint32_t expand_bits10(uint32_t v) {
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

__device__ __forceinline__ uint32_t quant10(float x, float lo, float hi) {
  if (!(hi > lo)) return 0u;
  const float u = (x - lo) / (hi - lo) * 1024.0f;
  return (uint32_t)fminf(fmaxf(u, 0.0f), 1023.0f);
}

// q16 grid coordinates (bvh_build.cpp: vsa_bvh_export_q), in fp64
__device__ __forceinline__ uint32_t qlo(float x, double lo, double step) {
  const double q = floor(((double)x - lo) / step) - 1.0 + 1.0;
  return (uint32_t)fmin(fmax(q, 0.0), 65535.0);
}
__device__ __forceinline__ uint32_t qhi(float x, double lo, double step) {
  const double q = ceil(((double)x - lo) / step) + 1.0 + 1.0;
  return (uint32_t)fmin(fmax(q, 0.0), 65535.0);
}

}  // namespace

// 1. triangle boxes + block partials of the triangle and centroid bounds
__global__ __launch_bounds__(BVHD_BLOCK) void bvh_dev_tri_setup(const float* __restrict__ verts,
                                                                const int32_t* __restrict__ faces, int nv, int nf,
                                                                float4* __restrict__ tbox, float* __restrict__ partials,
                                                                int32_t* info) {
  float r[12];
  for (int a = 0; a < 3; ++a) {
    r[a] = r[6 + a] = INFINITY;
    r[3 + a] = r[9 + a] = -INFINITY;
  }
  for (int f = blockIdx.x * BVHD_BLOCK + threadIdx.x; f < nf; f += gridDim.x * BVHD_BLOCK) {
    float a[3], b[3], c[3];
    fetch_tri(verts, faces, nv, f, info, a, b, c);
    float lo[3], hi[3], cen[3];
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(fminf(a[k], b[k]), c[k]);
      hi[k] = fmaxf(fmaxf(a[k], b[k]), c[k]);
      cen[k] = 0.5f * (lo[k] + hi[k]);        // bvh_build.cpp: tcen
      r[k] = fminf(r[k], lo[k]);
      r[3 + k] = fmaxf(r[3 + k], hi[k]);
      r[6 + k] = fminf(r[6 + k], cen[k]);
      r[9 + k] = fmaxf(r[9 + k], cen[k]);
    }
    tbox[2 * (size_t)f] = make_float4(lo[0], lo[1], lo[2], 0.f);
    tbox[2 * (size_t)f + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 12; ++k) {
      const float o = __shfl_xor(r[k], off);
      r[k] = (k % 6) < 3 ? fminf(r[k], o) : fmaxf(r[k], o);
    }
  __shared__ float red[BVHD_BLOCK / VSA_WAVE][12];
  const int wave = threadIdx.x / VSA_WAVE;
  if ((threadIdx.x & (VSA_WAVE - 1)) == 0)
    for (int k = 0; k < 12; ++k) red[wave][k] = r[k];
  __syncthreads();
  if (threadIdx.x < 12) {
    const int k = threadIdx.x;
    float v = red[0][k];
    for (int w = 1; w < BVHD_BLOCK / VSA_WAVE; ++w) v = (k % 6) < 3 ? fminf(v, red[w][k]) : fmaxf(v, red[w][k]);
    partials[12 * blockIdx.x + k] = v;
  }
}

// 2. mesh bounds and the padding of bvh_build.cpp (pad = 1e-6 |diag| of the triangle bounds)
__global__ __launch_bounds__(BVHD_BLOCK) void bvh_dev_bounds(const float* __restrict__ partials, int nparts,
                                                             float* __restrict__ bnd) {
  __shared__ float red[BVHD_BLOCK][12];
  float r[12];
  for (int a = 0; a < 3; ++a) {
    r[a] = r[6 + a] = INFINITY;
    r[3 + a] = r[9 + a] = -INFINITY;
  }
  for (int i = threadIdx.x; i < nparts; i += BVHD_BLOCK)
    for (int k = 0; k < 12; ++k) r[k] = (k % 6) < 3 ? fminf(r[k], partials[12 * i + k]) : fmaxf(r[k], partials[12 * i + k]);
  for (int k = 0; k < 12; ++k) red[threadIdx.x][k] = r[k];
  __syncthreads();
  if (threadIdx.x < 12) {
    const int k = threadIdx.x;
    float v = red[0][k];
    for (int t = 1; t < BVHD_BLOCK; ++t) v = (k % 6) < 3 ? fminf(v, red[t][k]) : fmaxf(v, red[t][k]);
    bnd[k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float dx = bnd[BND_TRI_HI + 0] - bnd[BND_TRI_LO + 0];
    const float dy = bnd[BND_TRI_HI + 1] - bnd[BND_TRI_LO + 1];
    const float dz = bnd[BND_TRI_HI + 2] - bnd[BND_TRI_LO + 2];
    bnd[BND_PAD] = 1e-6f * sqrtf(dx * dx + dy * dy + dz * dz);
  }
}

// 3. 30-bit Morton code of every centroid; values = face ids in ascending order
__global__ __launch_bounds__(BVHD_BLOCK) void bvh_dev_morton(const float4* __restrict__ tbox, int nf,
                                                             const float* __restrict__ bnd, uint32_t* __restrict__ keys,
                                                             int32_t* __restrict__ vals) {
  const int f = blockIdx.x * BVHD_BLOCK + threadIdx.x;
  if (f >= nf) return;
  const float4 lo = tbox[2 * (size_t)f], hi = tbox[2 * (size_t)f + 1];
  const float cx = 0.5f * (lo.x + hi.x), cy = 0.5f * (lo.y + hi.y), cz = 0.5f * (lo.z + hi.z);
  const uint32_t x = quant10(cx, bnd[BND_CEN_LO + 0], bnd[BND_CEN_HI + 0]);
  const uint32_t y = quant10(cy, bnd[BND_CEN_LO + 1], bnd[BND_CEN_HI + 1]);
  const uint32_t z = quant10(cz, bnd[BND_CEN_LO + 2], bnd[BND_CEN_HI + 2]);
  keys[f] = (expand_bits10(x) << 2) | (expand_bits10(y) << 1) | expand_bits10(z);
  vals[f] = f;
}

// 5. internal node i of the n - 1 (Karras 2012, Fig. 4): children (>= 0 internal, ~p leaf at sorted position
// p), covered range [first, last] of the sorted order, parent links ((parent << 1) | side; the root's is -1)
__global__ __launch_bounds__(BVHD_BLOCK) void bvh_dev_hierarchy(const uint32_t* __restrict__ keys, int n,
                                                                int2* __restrict__ child, int2* __restrict__ range,
                                                                int32_t* __restrict__ parent_int,
                                                                int32_t* __restrict__ parent_leaf) {
  const int i = blockIdx.x * BVHD_BLOCK + threadIdx.x;
  if (i >= n - 1) return;
  const int d = delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1) >= 0 ? 1 : -1;
  const int dmin = delta(keys, n, i, i - d);
  int lmax = 2;
  while (delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = delta(keys, n, i, j);
  int s = 0, t = l;
  do {
    t = (t + 1) >> 1;
    if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  const int gamma = i + s * d + min(d, 0);
  const int first = min(i, j), last = max(i, j);
  const int left = first == gamma ? ~gamma : gamma;
  const int right = last == gamma + 1 ? ~(gamma + 1) : gamma + 1;
  child[i] = make_int2(left, right);
  range[i] = make_int2(first, last);
  if (left < 0) parent_leaf[gamma] = i << 1;
  else parent_int[gamma] = i << 1;
  if (right < 0) parent_leaf[gamma + 1] = (i << 1) | 1;
  else parent_int[gamma + 1] = (i << 1) | 1;
  if (i == 0) parent_int[0] = -1;
}

// 6. bottom-up boxes.  Child slot (node, side) = 8 dwords: un-padded box lo xyz, kept-internal-node count of the
// child's subtree (int bits), hi xyz, 0.  The slots one thread writes are read by the sibling's thread, in any
// workgroup on any XCD: the writer's agent-scope release drains its stores before the arrival counter, and the
// second arrival's agent-scope acquire drops stale L1 lines before it reads the sibling's slot
// (cdna_hip_programming.md §6 Guideline 16).  cnt: zeroed before every launch.
__global__ __launch_bounds__(BVHD_BLOCK) void bvh_dev_bottom_up(const float4* __restrict__ tbox,
                                                                const int32_t* __restrict__ order, int n, int leaf_size,
                                                                const int2* __restrict__ range,
                                                                const int32_t* __restrict__ parent_int,
                                                                const int32_t* __restrict__ parent_leaf,
                                                                uint32_t* cnt, float4* slots, int32_t* info) {
  const int p = blockIdx.x * BVHD_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int f = order[p];
  float4 lo = tbox[2 * (size_t)f], hi = tbox[2 * (size_t)f + 1];
  int nint = 0;
  int pr = parent_leaf[p];
  for (int step = 0;; ++step) {
    const int node = pr >> 1, side = pr & 1;
    if (step >= BVHD_MAX_CLIMB || pr < 0 || node >= n - 1) {
      atomicOr(&info[INFO_ERR], ERR_WALK);
      return;
    }
    float4* mine = slots + 2 * (2 * (size_t)node + side);
    mine[0] = make_float4(lo.x, lo.y, lo.z, __int_as_float(nint));
    mine[1] = make_float4(hi.x, hi.y, hi.z, 0.f);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t old = __hip_atomic_fetch_add(&cnt[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == 0) return;                      // first arrival: the sibling's thread continues
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const float4* sib = slots + 2 * (2 * (size_t)node + (side ^ 1));
    const float4 slo = sib[0], shi = sib[1];
    lo = make_float4(fminf(lo.x, slo.x), fminf(lo.y, slo.y), fminf(lo.z, slo.z), 0.f);
    hi = make_float4(fmaxf(hi.x, shi.x), fmaxf(hi.y, shi.y), fmaxf(hi.z, shi.z), 0.f);
    const int2 r = range[node];
    nint = r.y - r.x + 1 > leaf_size ? 1 + nint + __float_as_int(slo.w) : 0;
    if (node == 0) {
      info[INFO_ROOT_NINT] = nint;
      return;
    }
    pr = parent_int[node];
  }
}

// 7. pre-order index of every kept internal node (root 0, parent before children: a node's index is its parent's
// + 1, + the left sibling's kept-internal count if it is a right child) by walking up; -1 for a collapsed node.
// The depth of a leaf = its kept ancestors (bvh_build.cpp's max_depth).
__global__ __launch_bounds__(BVHD_BLOCK) void bvh_dev_preorder(int n, int leaf_size, const int2* __restrict__ range,
                                                               const int32_t* __restrict__ parent_int,
                                                               const float4* __restrict__ slots,
                                                               int32_t* __restrict__ pre, int32_t* info) {
  const int i = blockIdx.x * BVHD_BLOCK + threadIdx.x;
  if (i >= n - 1) return;
  const int2 r = range[i];
  if (r.y - r.x + 1 <= leaf_size) {
    pre[i] = -1;
    return;
  }
  int idx = 0, depth = 0, cur = i;
  while (cur != 0) {
    const int pr = parent_int[cur];
    if (pr < 0 || (pr >> 1) >= n - 1 || depth >= BVHD_MAX_CLIMB) {
      atomicOr(&info[INFO_ERR], ERR_WALK);
      pre[i] = -1;
      return;
    }
    const int par = pr >> 1;
    idx += 1 + ((pr & 1) ? __float_as_int(slots[2 * (2 * (size_t)par)].w) : 0);
    ++depth;
    cur = par;
  }
  pre[i] = idx;
  atomicMax(&info[INFO_MAX_DEPTH], depth + 1);
}

// q16 frame: the union of the root's padded child boxes (every deeper padded box lies inside it), step =
// extent / 65533 rounded to the float the traversal uses (bvh_build.cpp: vsa_bvh_export_q).  One thread.
__global__ void bvh_dev_frame(int n, int leaf_size, const float4* __restrict__ slots, float* bnd) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float pad = bnd[BND_PAD];
  float lo[3], hi[3];
  if (n <= leaf_size) {
    for (int a = 0; a < 3; ++a) {
      lo[a] = bnd[BND_TRI_LO + a];
      hi[a] = bnd[BND_TRI_HI + a];
    }
    pad_box(lo, hi, pad);
  } else {
    for (int a = 0; a < 3; ++a) {
      lo[a] = INFINITY;
      hi[a] = -INFINITY;
    }
    for (int c = 0; c < 2; ++c) {
      const float4 sl = slots[2 * c], sh = slots[2 * c + 1];
      float l[3] = {sl.x, sl.y, sl.z}, h[3] = {sh.x, sh.y, sh.z};
      pad_box(l, h, pad);
      for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(lo[a], l[a]);
        hi[a] = fmaxf(hi[a], h[a]);
      }
    }
  }
  for (int a = 0; a < 3; ++a) {
    const double step = fmax((double)hi[a] - (double)lo[a], 1e-30) / 65533.0;
    bnd[BND_FRAME + a] = lo[a];
    bnd[BND_FRAME + 3 + a] = (float)step;
  }
}

namespace {

struct QFrame {
  double lo[3], step[3];
};

__device__ __forceinline__ void emit_child(float* __restrict__ o, uint32_t* __restrict__ q, int c, const float lo[3],
                                           const float hi[3], int32_t ref, int32_t cnt, int32_t qref, bool empty,
                                           const QFrame& fr) {
  for (int a = 0; a < 3; ++a) {
    o[6 * c + a] = lo[a];
    o[6 * c + 3 + a] = hi[a];
  }
  o[12 + c] = __int_as_float(ref);
  o[14 + c] = __int_as_float(cnt);
  uint32_t v[6];
  if (empty) {
    v[0] = v[1] = v[2] = 65535u;
    v[3] = v[4] = v[5] = 0u;
  } else {
    for (int a = 0; a < 3; ++a) {
      v[a] = qlo(lo[a], fr.lo[a], fr.step[a]);
      v[3 + a] = qhi(hi[a], fr.lo[a], fr.step[a]);
    }
  }
  q[3 * c + 0] = v[0] | (v[1] << 16);
  q[3 * c + 1] = v[2] | (v[3] << 16);
  q[3 * c + 2] = v[4] | (v[5] << 16);
  q[6 + c] = (uint32_t)qref;
}

}  // namespace

// 8a. both node formats of every kept internal node (or the wrapped root of a one-leaf mesh)
__global__ __launch_bounds__(BVHD_BLOCK) void bvh_dev_emit_nodes(int n, int leaf_size, const int2* __restrict__ child,
                                                                 const int2* __restrict__ range,
                                                                 const int32_t* __restrict__ pre,
                                                                 const float4* __restrict__ slots,
                                                                 const float* __restrict__ bnd, float* __restrict__ nodes_out,
                                                                 uint32_t* __restrict__ qnodes_out, int nr_nodes,
                                                                 int node_base, int tri_base) {
  const int i = blockIdx.x * BVHD_BLOCK + threadIdx.x;
  QFrame fr;
  for (int a = 0; a < 3; ++a) {
    fr.lo[a] = (double)bnd[BND_FRAME + a];
    fr.step[a] = (double)bnd[BND_FRAME + 3 + a];
  }
  const float pad = bnd[BND_PAD];
  float o[16];
  uint32_t q[8];
  int k;
  if (n <= leaf_size) {                        // one leaf: a root whose second child is empty (bvh_build.cpp)
    if (i != 0) return;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = bnd[BND_TRI_LO + a];
      hi[a] = bnd[BND_TRI_HI + a];
    }
    pad_box(lo, hi, pad);
    emit_child(o, q, 0, lo, hi, ~tri_base, n, ~((tri_base << 4) | n), false, fr);
    const float elo[3] = {1.f, 1.f, 1.f}, ehi[3] = {-1.f, -1.f, -1.f};
    emit_child(o, q, 1, elo, ehi, ~tri_base, 0, 0x7fffffff, true, fr);
    k = 0;
  } else {
    if (i >= n - 1) return;
    k = pre[i];
    if (k < 0 || k >= nr_nodes) return;        // (a kept node numbers below nr_nodes: vsa_bvh_dev_sizes)
    const int2 ch = child[i];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int e = c ? ch.y : ch.x;
      const int2 r = e < 0 ? make_int2(~e, ~e) : range[e];
      const int size = r.y - r.x + 1;
      const float4 sl = slots[2 * (2 * (size_t)i + c)], sh = slots[2 * (2 * (size_t)i + c) + 1];
      float lo[3] = {sl.x, sl.y, sl.z}, hi[3] = {sh.x, sh.y, sh.z};
      pad_box(lo, hi, pad);
      if (e >= 0 && size > leaf_size) {
        const int ref = pre[e] + node_base;
        emit_child(o, q, c, lo, hi, ref, 0, ref, false, fr);
      } else {
        emit_child(o, q, c, lo, hi, ~(r.x + tri_base), size, ~(((r.x + tri_base) << 4) | size), false, fr);
      }
    }
  }
  float4* on = reinterpret_cast<float4*>(nodes_out + 16 * (size_t)k);
  for (int v = 0; v < 4; ++v) on[v] = make_float4(o[4 * v], o[4 * v + 1], o[4 * v + 2], o[4 * v + 3]);
  uint4* oq = reinterpret_cast<uint4*>(qnodes_out + 8 * (size_t)k);
  oq[0] = make_uint4(q[0], q[1], q[2], q[3]);
  oq[1] = make_uint4(q[4], q[5], q[6], q[7]);
}

// 8b. triangle records in leaf (sorted) order: v0.xyz, face id bits, e1 = b - a, 0, e2 = c - a, 0
__global__ __launch_bounds__(BVHD_BLOCK) void bvh_dev_emit_tris(const float* __restrict__ verts,
                                                                const int32_t* __restrict__ faces, int nv, int n,
                                                                const int32_t* __restrict__ order,
                                                                float* __restrict__ tris_out, int32_t* info) {
  const int p = blockIdx.x * BVHD_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int f = order[p];
  float a[3], b[3], c[3];
  fetch_tri(verts, faces, nv, f, info, a, b, c);
  float4* o = reinterpret_cast<float4*>(tris_out + 12 * (size_t)p);
  o[0] = make_float4(a[0], a[1], a[2], __int_as_float(f));
  o[1] = make_float4(b[0] - a[0], b[1] - a[1], b[2] - a[2], 0.f);
  o[2] = make_float4(c[0] - a[0], c[1] - a[1], c[2] - a[2], 0.f);
}

struct vsa_bvh_dev {
  int nv = 0, nf = 0, leaf_size = 4, nparts = 1;
  hipStream_t stream = nullptr;
  float* verts = nullptr;          // [nv,3] copy (export / refit read it)
  int32_t* faces = nullptr;        // [nf,3] copy
  float4* tbox = nullptr;          // [nf,2]
  float* partials = nullptr;       // [nparts,12]
  float* bnd = nullptr;            // [BND_WORDS]
  int32_t* info = nullptr;         // [INFO_WORDS]
  uint32_t* keys_in = nullptr;     // [nf]
  uint32_t* keys = nullptr;        // [nf] sorted
  int32_t* vals_in = nullptr;      // [nf]
  int32_t* order = nullptr;        // [nf] face id at every sorted position
  void* sort_tmp = nullptr;
  size_t sort_bytes = 0;
  int2* child = nullptr;           // [nf-1]
  int2* range = nullptr;           // [nf-1]
  int32_t* parent_int = nullptr;   // [nf-1]
  int32_t* parent_leaf = nullptr;  // [nf]
  uint32_t* cnt = nullptr;         // [nf-1] arrival counters
  float4* slots = nullptr;         // [nf-1,2,2] child slots
  int32_t* pre = nullptr;          // [nf-1]
  int nr_nodes = 0, max_depth = 0;
  bool sized = false;
};

namespace {

void free_all(vsa_bvh_dev* h) {
  void* ptrs[] = {h->verts, h->faces, h->tbox, h->partials, h->bnd, h->info, h->keys_in, h->keys, h->vals_in,
                  h->order, h->sort_tmp, h->child, h->range, h->parent_int, h->parent_leaf, h->cnt, h->slots, h->pre};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
}

template <typename T>
hipError_t alloc(T** p, size_t count) {
  return hipMalloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T));
}

// 1, 2 and 6 (shared by build and refit), then the q16 frame
int fit_boxes(vsa_bvh_dev* h) {
  const int n = h->nf;
  hipLaunchKernelGGL(bvh_dev_tri_setup, dim3(h->nparts), dim3(BVHD_BLOCK), 0, h->stream, h->verts, h->faces, h->nv, n,
                     h->tbox, h->partials, h->info);
  hipLaunchKernelGGL(bvh_dev_bounds, dim3(1), dim3(BVHD_BLOCK), 0, h->stream, h->partials, h->nparts, h->bnd);
  VSA_HIP_TRY(hipGetLastError());
  return VSA_OK;
}

int bottom_up_and_frame(vsa_bvh_dev* h) {
  const int n = h->nf;
  if (n > 1) {
    VSA_HIP_TRY(hipMemsetAsync(h->cnt, 0, sizeof(uint32_t) * (size_t)(n - 1), h->stream));
    hipLaunchKernelGGL(bvh_dev_bottom_up, dim3(vsa_div_up(n, BVHD_BLOCK)), dim3(BVHD_BLOCK), 0, h->stream, h->tbox,
                       h->order, n, h->leaf_size, h->range, h->parent_int, h->parent_leaf, h->cnt, h->slots, h->info);
  }
  hipLaunchKernelGGL(bvh_dev_frame, dim3(1), dim3(64), 0, h->stream, n, h->leaf_size, h->slots, h->bnd);
  VSA_HIP_TRY(hipGetLastError());
  return VSA_OK;
}

}  // namespace

namespace {

// The whole build; radius 0: the Karras hierarchy (step 5), radius >= 1: PLOC clustering at that radius
// (csrc/bvh_ploc.hip) in its place.  Arguments checked by the callers.
int build_handle(const float* verts, const int32_t* faces, int nr_verts, int nr_faces, int leaf_size, int radius,
                 void* stream, vsa_bvh_dev** out_bvh) {
  if (nr_faces >= (1 << 27)) return VSA_ERR_UNSUPPORTED;     // q16 leaf code: first triangle << 4
  if (leaf_size < 1) leaf_size = 4;
  if (leaf_size > 8) leaf_size = 8;
  *out_bvh = nullptr;
  vsa_bvh_dev* h = new vsa_bvh_dev();
  h->nv = nr_verts;
  h->nf = nr_faces;
  h->leaf_size = leaf_size;
  h->stream = (hipStream_t)stream;
  h->nparts = std::min(BVHD_MAX_PARTIALS, vsa_div_up(nr_faces, BVHD_BLOCK));
  const int n = nr_faces, ni = nr_faces - 1;
  hipError_t e = hipSuccess;
#define BVHD_ALLOC(p, count) \
  if (e == hipSuccess) e = alloc(&h->p, (size_t)(count))
  BVHD_ALLOC(verts, 3 * (size_t)nr_verts);
  BVHD_ALLOC(faces, 3 * (size_t)n);
  BVHD_ALLOC(tbox, 2 * (size_t)n);
  BVHD_ALLOC(partials, 12 * (size_t)h->nparts);
  BVHD_ALLOC(bnd, BND_WORDS);
  BVHD_ALLOC(info, INFO_WORDS);
  BVHD_ALLOC(keys_in, n);
  BVHD_ALLOC(keys, n);
  BVHD_ALLOC(vals_in, n);
  BVHD_ALLOC(order, n);
  BVHD_ALLOC(child, ni);
  BVHD_ALLOC(range, ni);
  BVHD_ALLOC(parent_int, ni);
  BVHD_ALLOC(parent_leaf, n);
  BVHD_ALLOC(cnt, ni);
  BVHD_ALLOC(slots, 4 * (size_t)ni);
  BVHD_ALLOC(pre, ni);
#undef BVHD_ALLOC
  if (e == hipSuccess)
    e = rocprim::radix_sort_pairs(nullptr, h->sort_bytes, h->keys_in, h->keys, h->vals_in, h->order, (unsigned)n, 0, 30,
                                  h->stream);
  if (e == hipSuccess) e = hipMalloc(&h->sort_tmp, h->sort_bytes ? h->sort_bytes : 16);
  if (e == hipSuccess) e = hipMemcpyAsync(h->verts, verts, sizeof(float) * 3 * (size_t)nr_verts, hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->faces, faces, sizeof(int32_t) * 3 * (size_t)n, hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->info, 0, sizeof(int32_t) * INFO_WORDS, h->stream);
  int rc = e == hipSuccess ? VSA_OK : (int)e;
  if (rc == VSA_OK) rc = fit_boxes(h);
  if (rc == VSA_OK) {
    hipLaunchKernelGGL(bvh_dev_morton, dim3(vsa_div_up(n, BVHD_BLOCK)), dim3(BVHD_BLOCK), 0, h->stream, h->tbox, n, h->bnd,
                       h->keys_in, h->vals_in);
    e = hipGetLastError();
    if (e == hipSuccess)
      e = rocprim::radix_sort_pairs(h->sort_tmp, h->sort_bytes, h->keys_in, h->keys, h->vals_in, h->order, (unsigned)n, 0,
                                    30, h->stream);
    if (e == hipSuccess && n > 1) e = hipMemsetAsync(h->parent_leaf, 0xff, sizeof(int32_t) * (size_t)n, h->stream);
    if (e == hipSuccess && n > 1) e = hipMemsetAsync(h->parent_int, 0xff, sizeof(int32_t) * (size_t)ni, h->stream);
    if (e == hipSuccess && n > 1 && radius == 0) {
      hipLaunchKernelGGL(bvh_dev_hierarchy, dim3(vsa_div_up(ni, BVHD_BLOCK)), dim3(BVHD_BLOCK), 0, h->stream, h->keys, n,
                         h->child, h->range, h->parent_int, h->parent_leaf);
      e = hipGetLastError();
    }
    rc = e == hipSuccess ? VSA_OK : (int)e;
    if (rc == VSA_OK && n > 1 && radius > 0) {
      // the PLOC tree's leaf order replaces the sorted order: written to vals_in (consumed by the sort), then swapped
      rc = bvh_ploc_topology(h->tbox, h->order, n, radius, h->stream, h->vals_in, h->child, h->range, h->parent_int,
                             h->parent_leaf, h->info + INFO_ERR, ERR_WALK);
      std::swap(h->order, h->vals_in);
    }
  }
  if (rc == VSA_OK) rc = bottom_up_and_frame(h);
  if (rc == VSA_OK && n > leaf_size) {
    hipLaunchKernelGGL(bvh_dev_preorder, dim3(vsa_div_up(ni, BVHD_BLOCK)), dim3(BVHD_BLOCK), 0, h->stream, n, leaf_size,
                       h->range, h->parent_int, h->slots, h->pre, h->info);
    e = hipGetLastError();
    rc = e == hipSuccess ? VSA_OK : (int)e;
  }
  if (rc != VSA_OK) {
    (void)hipStreamSynchronize(h->stream);
    free_all(h);
    delete h;
    return rc;
  }
  *out_bvh = h;
  return VSA_OK;
}

}  // namespace

extern "C" int vsa_bvh_dev_build(const float* verts, const int32_t* faces, int nr_verts, int nr_faces, int leaf_size,
                                 void* stream, vsa_bvh_dev** out_bvh) {
  if (!verts || !faces || !out_bvh || nr_verts <= 0 || nr_faces <= 0) return VSA_ERR_ARG;
  return build_handle(verts, faces, nr_verts, nr_faces, leaf_size, 0, stream, out_bvh);
}

extern "C" int vsa_bvh_dev_build_ploc(const float* verts, const int32_t* faces, int nr_verts, int nr_faces,
                                      int leaf_size, int radius, void* stream, vsa_bvh_dev** out_bvh) {
  if (!verts || !faces || !out_bvh || nr_verts <= 0 || nr_faces <= 0) return VSA_ERR_ARG;
  if (radius < 1 || radius > BVH_PLOC_MAX_RADIUS) return VSA_ERR_ARG;
  return build_handle(verts, faces, nr_verts, nr_faces, leaf_size, radius, stream, out_bvh);
}

extern "C" int vsa_bvh_dev_sizes(const vsa_bvh_dev* bvh, int* nr_nodes, int* nr_tris, int* max_depth) {
  if (!bvh) return VSA_ERR_ARG;
  vsa_bvh_dev* h = const_cast<vsa_bvh_dev*>(bvh);
  int32_t info[INFO_WORDS];
  VSA_HIP_TRY(hipMemcpyAsync(info, h->info, sizeof(info), hipMemcpyDeviceToHost, h->stream));
  VSA_HIP_TRY(hipStreamSynchronize(h->stream));
  if (info[INFO_ERR] & ERR_FACE_INDEX) return VSA_ERR_ARG;
  if (info[INFO_ERR]) return VSA_ERR_UNSUPPORTED;
  h->nr_nodes = h->nf <= h->leaf_size ? 1 : info[INFO_ROOT_NINT];
  h->max_depth = info[INFO_MAX_DEPTH];
  if (nr_nodes) *nr_nodes = h->nr_nodes;
  if (nr_tris) *nr_tris = h->nf;
  if (max_depth) *max_depth = h->max_depth;
  if (h->max_depth >= BVHD_TRACE_STACK) return VSA_ERR_UNSUPPORTED;
  h->sized = true;
  return VSA_OK;
}

extern "C" int vsa_bvh_dev_export(const vsa_bvh_dev* bvh, float* nodes_out, uint32_t* qnodes_out, float* tris_out,
                                  int node_base, int tri_base, float* frame_out, void* stream) {
  if (!bvh || !nodes_out || !qnodes_out || !tris_out || !frame_out || node_base < 0 || tri_base < 0) return VSA_ERR_ARG;
  if (!bvh->sized) return VSA_ERR_ARG;                 // vsa_bvh_dev_sizes first (it also checks the build)
  const int n = bvh->nf;
  hipStream_t st = (hipStream_t)stream;
  // the handle's buffers were written on the build's stream
  if (st != bvh->stream) VSA_HIP_TRY(hipStreamSynchronize(bvh->stream));
  const int nthreads = n <= bvh->leaf_size ? 1 : n - 1;
  hipLaunchKernelGGL(bvh_dev_emit_nodes, dim3(vsa_div_up(nthreads, BVHD_BLOCK)), dim3(BVHD_BLOCK), 0, st, n,
                     bvh->leaf_size, bvh->child, bvh->range, bvh->pre, bvh->slots, bvh->bnd, nodes_out, qnodes_out,
                     bvh->nr_nodes, node_base, tri_base);
  hipLaunchKernelGGL(bvh_dev_emit_tris, dim3(vsa_div_up(n, BVHD_BLOCK)), dim3(BVHD_BLOCK), 0, st, bvh->verts, bvh->faces,
                     bvh->nv, n, bvh->order, tris_out, bvh->info);
  VSA_HIP_TRY(hipGetLastError());
  VSA_HIP_TRY(hipMemcpyAsync(frame_out, bvh->bnd + BND_FRAME, 6 * sizeof(float), hipMemcpyDeviceToHost, st));
  VSA_HIP_TRY(hipStreamSynchronize(st));
  return VSA_OK;
}

extern "C" int vsa_bvh_dev_refit(vsa_bvh_dev* bvh, const float* verts, int nr_verts, void* stream) {
  if (!bvh || !verts || nr_verts != bvh->nv) return VSA_ERR_ARG;
  if (!bvh->sized) return VSA_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (st != bvh->stream) VSA_HIP_TRY(hipStreamSynchronize(bvh->stream));
  bvh->stream = st;
  VSA_HIP_TRY(hipMemcpyAsync(bvh->verts, verts, sizeof(float) * 3 * (size_t)nr_verts, hipMemcpyDeviceToDevice, st));
  int rc = fit_boxes(bvh);
  if (rc == VSA_OK) rc = bottom_up_and_frame(bvh);
  return rc;
}

extern "C" int vsa_bvh_dev_destroy(vsa_bvh_dev* bvh) {
  if (!bvh) return VSA_OK;
  (void)hipStreamSynchronize(bvh->stream);
  free_all(bvh);
  delete bvh;
  return VSA_OK;
}
