// UV atlas of one consistently wound triangle mesh by box projection (vsa_atlas*; rules in include/volsurfs_hip.h,
// DESIGN §16), and with the box charts merged into plane-projected groups first (vsa_atlas_merged).
//
// One stream.  Once per call:
//   label:   fp32 face normals; the (vertex, face) list radix-sorted by vertex (ascending face within a vertex) gives
//            the per-vertex normal sums in a fixed order; one lane per face picks the face's direction label.  The 3F
//            (min, max) edge keys are radix-sorted with their slots: an edge with exactly two slots, traversed in
//            opposite directions by two faces of one label, is a join pair; pairs are compacted by a scan.
// vsa_atlas_merged only, once per call:
//   merge:   the join pairs are the eligible edges without the label test.  The box charts (a union-find over the pairs
//            of one label) are the first groups; the faces radix-sorted by group give every group's run, and one wave
//            per group sums its area vector in ascending face order.  Then merge rounds: the pairs' (lo group, hi group)
//            keys radix-sorted and run-lengthed into adjacent pairs with weights; a scan of the pairs' face counts lays
//            out (face, pair) items, one lane per item tests its face against the pair's summed area vector and clears
//            the pair's flag when it fails; every valid pair offers itself to both groups by a 64-bit atomic max of
//            (weight, ~neighbour); pairs that picked each other merge (parent, area vector, merged mark), every face
//            is relabelled through the parent, and the faces are sorted by group again.  The host reads the valid-pair
//            count once per round.  Last, one lane per merged group builds its frame and one lane per face writes its
//            corners' plane coordinates, which the boxes, the UVs and the split read instead of the label's pick.
// Then rounds, until no chart overlaps itself:
//   charts:  union-find over the join pairs whose faces carry the same split code (CAS hooks of the larger root under
//            the smaller, so a root is its component's minimum face index whatever the order); roots flagged and
//            scanned into chart indices; chart boxes by 32-bit atomic min / max of ordered float bits.
//   pack:    a bisection over the fp32 bit pattern of the texel density s.  A step: rectangle keys per chart, a radix
//            sort, a scan of the sorted widths, and one lane walking the next-fit shelves (a binary search over the
//            width prefix per shelf: about sqrt(charts) shelves); the host reads the fit flag.  The last walk writes
//            the shelves, and one lane per sorted rectangle finds its shelf and offset.
//   emit:    one lane per face writes its three corners' UVs.
//   raster:  the coverage rule is uv_raster.h's (faces snapped to 1/256 texel, int64 edge functions, top-left rule); a
//            scan of every face's 8x8-tile count gives (face, tile) work items, one lane per item tests its 64 texel
//            centres and counts them; a second
//            pass over the same items flags the charts with a texel counted twice.  Flagged charts are split by a bit
//            of their faces' split codes and the round repeats.
// No float is summed by atomics: the normal sums have a fixed order, and integer atomics form minima, maxima, unions,
// flags and counts.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "mesh_topology.h"
#include "uv_raster.h"

#define ATL_BLOCK MT_BLOCK
#define ATL_TILE 8
#define ATL_DEPTH_CAP 24
#define ATL_MIN_RES 8
#define ATL_MAX_RES 16384
#define ATL_MAX_ROUNDS 100   // rounds of chart building and packing; measured at most 20

// device counters
#define ACT_J 0
#define ACT_C 1
#define ACT_FIT 2
#define ACT_NSH 3
#define ACT_OVL 4
#define ACT_COV 5
#define ACT_PROG 6
#define ACT_BOX 8      // vsa_atlas_merged: box charts, adjacent group pairs, valid pairs, merges
#define ACT_NP 9
#define ACT_NV 10
#define ACT_MERGES 11
#define ACT_N 16

using mt::at;
using mt::u64;

// Projection axes per label (+x, -x, +y, -y, +z, -z): +x -> (y, z), -x -> (z, y), +y -> (z, x), -y -> (x, z),
// +z -> (x, y), -z -> (y, x).
__constant__ int atl_ax_u[6] = {1, 2, 2, 0, 0, 1};
__constant__ int atl_ax_v[6] = {2, 1, 0, 2, 1, 0};

__device__ __forceinline__ unsigned atl_ord(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float atl_unord(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// ------------------------------------------------------------------------------------------------ label

__global__ __launch_bounds__(ATL_BLOCK) void atl_normals(const float* __restrict__ P, const int32_t* __restrict__ faces,
                                                        long long F, float* __restrict__ fn) {
  const long long f = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (f >= F) return;
  const long long a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  const float e1x = P[3 * b] - P[3 * a], e1y = P[3 * b + 1] - P[3 * a + 1], e1z = P[3 * b + 2] - P[3 * a + 2];
  const float e2x = P[3 * c] - P[3 * a], e2y = P[3 * c + 1] - P[3 * a + 1], e2z = P[3 * c + 2] - P[3 * a + 2];
  fn[3 * f] = e1y * e2z - e1z * e2y;
  fn[3 * f + 1] = e1z * e2x - e1x * e2z;
  fn[3 * f + 2] = e1x * e2y - e1y * e2x;
}

// N_v: the fp32 sum of n_f over the faces at v, in ascending face index, from 0.
__global__ __launch_bounds__(ATL_BLOCK) void atl_vertex_sums(const float* __restrict__ fn,
                                                            const uint32_t* __restrict__ vff,
                                                            const int32_t* __restrict__ vstart,
                                                            const int32_t* __restrict__ vend, long long V,
                                                            float* __restrict__ nv) {
  const long long v = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (v >= V) return;
  float x = 0.f, y = 0.f, z = 0.f;
  for (int j = vstart[v]; j < vend[v]; ++j) {
    const long long f = vff[j];
    x = x + fn[3 * f];
    y = y + fn[3 * f + 1];
    z = z + fn[3 * f + 2];
  }
  nv[3 * v] = x;
  nv[3 * v + 1] = y;
  nv[3 * v + 2] = z;
}

// argmax of (x, -x, y, -y, z, -z), ties to the earlier direction.
__device__ __forceinline__ int atl_argmax6(float x, float y, float z) {
  const float d[6] = {x, -x, y, -y, z, -z};
  int best = 0;
#pragma unroll
  for (int k = 1; k < 6; ++k)
    if (d[k] > d[best]) best = k;
  return best;
}

__global__ __launch_bounds__(ATL_BLOCK) void atl_labels(const int32_t* __restrict__ faces, long long F,
                                                       const float* __restrict__ fn, const float* __restrict__ nv,
                                                       int32_t* __restrict__ label, uint32_t* __restrict__ code) {
  const long long f = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (f >= F) return;
  const float nx = fn[3 * f], ny = fn[3 * f + 1], nz = fn[3 * f + 2];
  code[f] = 1u;
  if (nx == 0.f && ny == 0.f && nz == 0.f) {
    label[f] = 0;
    return;
  }
  const long long a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  const float sx = (nv[3 * a] + nv[3 * b]) + nv[3 * c];
  const float sy = (nv[3 * a + 1] + nv[3 * b + 1]) + nv[3 * c + 1];
  const float sz = (nv[3 * a + 2] + nv[3 * b + 2]) + nv[3 * c + 2];
  const int cand = atl_argmax6(sx, sy, sz);
  const float comp[3] = {nx, ny, nz};
  const double dn = (double)(cand & 1 ? -comp[cand >> 1] : comp[cand >> 1]);
  const double nn = ((double)nx * (double)nx + (double)ny * (double)ny) + (double)nz * (double)nz;
  label[f] = (dn >= 0.0 && 4.0 * (dn * dn) >= nn) ? cand : atl_argmax6(nx, ny, nz);
}

// Join flag at the first sorted slot of an edge with exactly two slots, opposite directions and one label (label
// null: the edge test alone, vsa_atlas_merged's).
__global__ __launch_bounds__(ATL_BLOCK) void atl_join_flags(const u64* __restrict__ sorted,
                                                           const uint32_t* __restrict__ slot,
                                                           const int32_t* __restrict__ faces,
                                                           const int32_t* __restrict__ label, long long n3,
                                                           int32_t* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (i >= n3) return;
  int ok = 0;
  if ((i == 0 || sorted[i - 1] != sorted[i]) && i + 1 < n3 && sorted[i + 1] == sorted[i] &&
      (i + 2 == n3 || sorted[i + 2] != sorted[i])) {
    const long long s0 = slot[i], s1 = slot[i + 1];
    const long long f0 = s0 / 3, f1 = s1 / 3;
    const int c0 = (int)(s0 - 3 * f0), c1 = (int)(s1 - 3 * f1);
    ok = faces[3 * f0 + c0] == faces[3 * f1 + (c1 == 2 ? 0 : c1 + 1)] && (!label || label[f0] == label[f1]);
  }
  flags[i] = ok;
}

__global__ __launch_bounds__(ATL_BLOCK) void atl_join_compact(const uint32_t* __restrict__ slot,
                                                             const int32_t* __restrict__ flags,
                                                             const int32_t* __restrict__ rank, long long n3,
                                                             int2* __restrict__ pairs, long long* __restrict__ ctr) {
  const long long i = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (i >= n3) return;
  if (flags[i]) pairs[rank[i]] = make_int2((int)(slot[i] / 3), (int)(slot[i + 1] / 3));
  if (i == n3 - 1) ctr[ACT_J] = rank[i] + flags[i];
}

// ------------------------------------------------------------------------------------------------ charts

// Every parent is <= its child, so the root of a component is its minimum face index (mesh_topology.h).
// key (vsa_atlas_merged: the label, then the group): the pair's faces must also agree on it.
__global__ __launch_bounds__(ATL_BLOCK) void atl_hook(const int2* __restrict__ pairs, const long long* __restrict__ ctr,
                                                     const uint32_t* __restrict__ code,
                                                     const int32_t* __restrict__ key, int32_t* par) {
  const long long i = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (i >= ctr[ACT_J]) return;
  const int2 pr = pairs[i];
  const uint32_t k = code[pr.x];
  if (k == 0u || k != code[pr.y]) return;
  if (key && key[pr.x] != key[pr.y]) return;
  fu_union(par, pr.x, pr.y);
}

// cidx[f] = the chart number of f's root, in place over root[f] (each lane reads and writes its own entry only).
__global__ __launch_bounds__(ATL_BLOCK) void atl_chart_index(const int32_t* __restrict__ flags,
                                                            const int32_t* __restrict__ rank, long long F,
                                                            int32_t* __restrict__ cidx, long long* __restrict__ ctr) {
  const long long f = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (f >= F) return;
  cidx[f] = rank[cidx[f]];
  if (f == F - 1) ctr[ACT_C] = rank[f] + flags[f];
}

// Chart box: [umin, umax, vmin, vmax] as ordered bits; minima start at 0xFFFFFFFF, maxima at 0.
__global__ __launch_bounds__(ATL_BLOCK) void atl_box_init(unsigned* __restrict__ box, long long n) {
  const long long i = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (i < n) box[i] = (i & 1) ? 0u : 0xFFFFFFFFu;
}

// Corner c of face f in its chart's plane.  PC (vsa_atlas_merged): the plane coordinates atl_plane_coords wrote; else
// the two coordinates the face's label picks.
template <bool PC>
__device__ __forceinline__ float2 atl_corner(const float* __restrict__ P, const int32_t* __restrict__ faces,
                                             const int32_t* __restrict__ label, const float* __restrict__ pc,
                                             long long f, int c) {
  if (PC) return make_float2(pc[6 * f + 2 * c], pc[6 * f + 2 * c + 1]);
  const int l = label[f];
  const long long v = faces[3 * f + c];
  return make_float2(P[3 * v + atl_ax_u[l]], P[3 * v + atl_ax_v[l]]);
}

template <bool PC>
__global__ __launch_bounds__(ATL_BLOCK) void atl_boxes(const float* __restrict__ P, const int32_t* __restrict__ faces,
                                                      long long F, const int32_t* __restrict__ label,
                                                      const float* __restrict__ pc,
                                                      const int32_t* __restrict__ cidx, unsigned* __restrict__ box) {
  const long long f = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (f >= F) return;
  unsigned umin = 0xFFFFFFFFu, umax = 0u, vmin = 0xFFFFFFFFu, vmax = 0u;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float2 q = atl_corner<PC>(P, faces, label, pc, f, c);
    const unsigned ku = atl_ord(q.x), kv = atl_ord(q.y);
    umin = ku < umin ? ku : umin;
    umax = ku > umax ? ku : umax;
    vmin = kv < vmin ? kv : vmin;
    vmax = kv > vmax ? kv : vmax;
  }
  unsigned* b = box + 4 * (long long)cidx[f];
  atomicMin(b, umin);
  atomicMax(b + 1, umax);
  atomicMin(b + 2, vmin);
  atomicMax(b + 3, vmax);
}

// ------------------------------------------------------------------------------------------------ pack

// (width, height) extents of chart c after its rotation; rot = height > width before it.
__device__ __forceinline__ void atl_extent(const unsigned* __restrict__ box, long long c, float* ew, float* eh,
                                           bool* rot) {
  const float w = atl_unord(box[4 * c + 1]) - atl_unord(box[4 * c]);
  const float h = atl_unord(box[4 * c + 3]) - atl_unord(box[4 * c + 2]);
  *rot = h > w;
  *ew = *rot ? h : w;
  *eh = *rot ? w : h;
}

// ceil(fl(e * s)) + 2p texels, or R + 1 when ceil(fl(e * s)) > R (inf included).
__device__ __forceinline__ int atl_side(float e, float s, int R, int p) {
  const float t = ceilf(e * s);
  return t <= (float)R ? (int)t + 2 * p : R + 1;
}

__global__ __launch_bounds__(ATL_BLOCK) void atl_rect_keys(const unsigned* __restrict__ box, long long C, float s,
                                                          int R, int p, u64* __restrict__ keys) {
  const long long c = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (c >= C) return;
  float ew, eh;
  bool rot;
  atl_extent(box, c, &ew, &eh, &rot);
  const int W = atl_side(ew, s, R, p), H = atl_side(eh, s, R, p);
  keys[c] = (u64)(0xFFFFu - (unsigned)H) << 48 | (u64)(0xFFFFu - (unsigned)W) << 32 | (u64)c;
}

__global__ __launch_bounds__(ATL_BLOCK) void atl_rect_widths(const u64* __restrict__ sorted, long long C,
                                                            long long* __restrict__ wid) {
  const long long k = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (k >= C) return;
  wid[k] = (long long)(0xFFFFu - (unsigned)((sorted[k] >> 32) & 0xFFFFu));
}

// One lane: next-fit shelves over the sorted rectangles.  pre[k] = sum of the first k widths (pre[0] = 0).  A shelf
// starting at i takes rectangles i .. j - 1, j the largest index with pre[j] - pre[i] <= R; its height is rectangle
// i's.  emit: shelf starts and y offsets written.
__global__ void atl_shelf_walk(const u64* __restrict__ sorted, const long long* __restrict__ pre, long long C, int R,
                               int emit, int32_t* __restrict__ sh_start, int32_t* __restrict__ sh_y,
                               long long* __restrict__ ctr) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  long long i = 0, y = 0, nsh = 0;
  int fit = 1;
  while (i < C) {
    const long long lim = pre[i] + R;
    long long lo = i, hi = C;   // largest j in [i, C] with pre[j] <= lim
    while (lo < hi) {
      const long long mid = lo + (hi - lo + 1) / 2;
      if (pre[mid] <= lim) lo = mid;
      else hi = mid - 1;
    }
    if (lo == i) {
      fit = 0;
      break;
    }
    if (emit) {
      sh_start[nsh] = (int32_t)i;
      sh_y[nsh] = (int32_t)y;
    }
    ++nsh;
    y += (long long)(0xFFFFu - (unsigned)(sorted[i] >> 48));
    if (y > R) {
      fit = 0;
      break;
    }
    i = lo;
  }
  ctr[ACT_FIT] = fit;
  ctr[ACT_NSH] = nsh;
}

__global__ __launch_bounds__(ATL_BLOCK) void atl_offsets(const u64* __restrict__ sorted,
                                                        const long long* __restrict__ pre, long long C,
                                                        const int32_t* __restrict__ sh_start,
                                                        const int32_t* __restrict__ sh_y,
                                                        const long long* __restrict__ ctr, int2* __restrict__ off) {
  const long long k = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (k >= C) return;
  long long lo = 0, hi = ctr[ACT_NSH] - 1;   // the last shelf starting at or before k
  while (lo < hi) {
    const long long mid = lo + (hi - lo + 1) / 2;
    if (sh_start[mid] <= k) lo = mid;
    else hi = mid - 1;
  }
  off[sorted[k] & 0xFFFFFFFFull] = make_int2((int)(pre[k] - pre[sh_start[lo]]), sh_y[lo]);
}

// ------------------------------------------------------------------------------------------------ emit

// uv = (local * s + (offset + p)) / R in fp32; local = (u - umin, v - vmin), or (vmax - v, u - umin) when rotated.
template <bool PC>
__global__ __launch_bounds__(ATL_BLOCK) void atl_emit(const float* __restrict__ P, const int32_t* __restrict__ faces,
                                                     long long F, const int32_t* __restrict__ label,
                                                     const float* __restrict__ pc, const int32_t* __restrict__ cidx,
                                                     const unsigned* __restrict__ box, const int2* __restrict__ off,
                                                     float s, int R, int p, float* __restrict__ uv) {
  const long long f = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (f >= F) return;
  const long long c = cidx[f];
  const float umin = atl_unord(box[4 * c]), umax = atl_unord(box[4 * c + 1]);
  const float vmin = atl_unord(box[4 * c + 2]), vmax = atl_unord(box[4 * c + 3]);
  const bool rot = (vmax - vmin) > (umax - umin);
  const int2 o = off[c];
  const float ox = (float)(o.x + p), oy = (float)(o.y + p), r = (float)R;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float2 q = atl_corner<PC>(P, faces, label, pc, f, k);
    const float u = q.x, w = q.y;
    const float lx = rot ? vmax - w : u - umin;
    const float ly = rot ? u - umin : w - vmin;
    uv[6 * f + 2 * k] = (lx * s + ox) / r;
    uv[6 * f + 2 * k + 1] = (ly * s + oy) / r;
  }
}

// ------------------------------------------------------------------------------------------------ raster

// Coverage is uv_raster.h's rule: the snapped corners, the texel box and the edge tests are its own.
__global__ __launch_bounds__(ATL_BLOCK) void atl_tile_counts(const float* __restrict__ uv, long long F, int R,
                                                            long long* __restrict__ ntile) {
  const long long f = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (f >= F) return;
  const UvBox b = uv_box(uv_snap(uv + 6 * f, R), R);
  ntile[f] = (b.i0 > b.i1 || b.j0 > b.j1)
                 ? 0
                 : (long long)(b.i1 / ATL_TILE - b.i0 / ATL_TILE + 1) * (b.j1 / ATL_TILE - b.j0 / ATL_TILE + 1);
}

// mode 0: count[j R + i] += 1 and face_id[j R + i] = min(face) (unsigned: empty stays -1) for every covered texel;
// mode 1: flag[cidx[f]] = 1 where a covered texel's count is >= 2.  toff[f] = tiles before face f (toff[F] = total).
__global__ __launch_bounds__(ATL_BLOCK) void atl_raster(const float* __restrict__ uv, long long F, int R,
                                                       const long long* __restrict__ toff, long long total, int mode,
                                                       int32_t* __restrict__ count, uint32_t* __restrict__ face_id,
                                                       const int32_t* __restrict__ cidx, int32_t* __restrict__ flag) {
  for (long long it = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x; it < total;
       it += (long long)gridDim.x * ATL_BLOCK) {
    long long lo = 0, hi = F - 1;   // the last face with toff[f] <= it
    while (lo < hi) {
      const long long mid = lo + (hi - lo + 1) / 2;
      if (toff[mid] <= it) lo = mid;
      else hi = mid - 1;
    }
    const long long f = lo;
    const UvTri t = uv_snap(uv + 6 * f, R);
    const UvBox b = uv_box(t, R);
    const long long k = it - toff[f];
    const int ntx = b.i1 / ATL_TILE - b.i0 / ATL_TILE + 1;
    const int tx = b.i0 / ATL_TILE + (int)(k % ntx), ty = b.j0 / ATL_TILE + (int)(k / ntx);
    const int ia = max(tx * ATL_TILE, b.i0), ib = min(tx * ATL_TILE + ATL_TILE - 1, b.i1);
    const int ja = max(ty * ATL_TILE, b.j0), jb = min(ty * ATL_TILE + ATL_TILE - 1, b.j1);
    bool hit2 = false;
    for (int j = ja; j <= jb; ++j) {
      const long long py = uv_centre(j);
      for (int i = ia; i <= ib; ++i) {
        if (!uv_edges_in(t, uv_centre(i), py)) continue;      // (the box is empty unless the face is front)
        const long long o = (long long)j * R + i;
        if (mode == 0) {
          atomicAdd(count + o, 1);
          if (face_id) atomicMin(face_id + o, (uint32_t)f);
        } else {
          hit2 |= count[o] >= 2;
        }
      }
    }
    if (hit2) flag[cidx[f]] = 1;
  }
}

__global__ __launch_bounds__(ATL_BLOCK) void atl_covered(const int32_t* __restrict__ count, long long n,
                                                        long long* __restrict__ ctr) {
  __shared__ int part[ATL_BLOCK / VSA_WAVE];
  const long long i = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  int c = i < n && count[i] > 0;
#pragma unroll
  for (int d = VSA_WAVE / 2; d > 0; d >>= 1) c += __shfl_down(c, d, VSA_WAVE);
  if ((threadIdx.x & (VSA_WAVE - 1)) == 0) part[threadIdx.x / VSA_WAVE] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < ATL_BLOCK / VSA_WAVE; ++w) s += part[w];
    if (s) atomicAdd((unsigned long long*)(ctr + ACT_COV), (unsigned long long)s);
  }
}

__global__ __launch_bounds__(ATL_BLOCK) void atl_count_flags(const int32_t* __restrict__ flag, long long C,
                                                            long long* __restrict__ ctr) {
  const long long c = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (c < C && flag[c]) atomicAdd((unsigned long long*)(ctr + ACT_OVL), 1ull);
}

// A face of a flagged chart: code 0 (one chart per face) at the depth cap, else code = 2 code + side, side = 1 when
// the sum of its corners' coordinates along the box's longer side (u on a tie) exceeds 3 x the side's midpoint (fp64).
template <bool PC>
__global__ __launch_bounds__(ATL_BLOCK) void atl_split(const float* __restrict__ P, const int32_t* __restrict__ faces,
                                                      long long F, const int32_t* __restrict__ label,
                                                      const float* __restrict__ pc, const int32_t* __restrict__ cidx,
                                                      const unsigned* __restrict__ box,
                                                      const int32_t* __restrict__ flag, uint32_t* __restrict__ code,
                                                      long long* __restrict__ ctr) {
  const long long f = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  bool changed = false;
  if (f < F) {
    const long long c = cidx[f];
    const uint32_t k = code[f];
    if (flag[c] && k != 0u) {
      changed = true;
      if (k >= (1u << ATL_DEPTH_CAP)) {
        code[f] = 0u;
      } else {
        const float umin = atl_unord(box[4 * c]), umax = atl_unord(box[4 * c + 1]);
        const float vmin = atl_unord(box[4 * c + 2]), vmax = atl_unord(box[4 * c + 3]);
        const bool along_u = (umax - umin) >= (vmax - vmin);
        const double lo = along_u ? umin : vmin, hi = along_u ? umax : vmax;
        double sum;
        if (PC) {
          const float* q = pc + 6 * f + (along_u ? 0 : 1);
          sum = ((double)q[0] + (double)q[2]) + (double)q[4];
        } else {
          const int ax = along_u ? atl_ax_u[label[f]] : atl_ax_v[label[f]];
          sum = ((double)P[3 * (long long)faces[3 * f] + ax] + (double)P[3 * (long long)faces[3 * f + 1] + ax]) +
                (double)P[3 * (long long)faces[3 * f + 2] + ax];
        }
        code[f] = 2u * k + (sum > 1.5 * (lo + hi) ? 1u : 0u);
      }
    }
  }
  // faces whose code changed (one atomic per wave): 0 means the next round would repeat this one
  const u64 m = __ballot(changed);
  if ((threadIdx.x & (VSA_WAVE - 1)) == 0 && m)
    atomicAdd((unsigned long long*)(ctr + ACT_PROG), (unsigned long long)__popcll(m));
}

// ------------------------------------------------------------------------------------------------ merge

// vsa_atlas_merged (rules in include/volsurfs_hip.h).  A group is named by its minimum face; grp[f] is the
// group of face f, and gA, merged, best, gstart, gend and fr are indexed by group id.  Integer atomics only: the area
// vectors are summed in a fixed order.

__global__ __launch_bounds__(ATL_BLOCK) void atl_group_list(const int32_t* __restrict__ flags,
                                                           const int32_t* __restrict__ rank, long long F,
                                                           int32_t* __restrict__ glist, long long* __restrict__ ctr) {
  const long long f = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (f >= F) return;
  if (flags[f]) glist[rank[f]] = (int32_t)f;
  if (f == F - 1) ctr[ACT_BOX] = rank[f] + flags[f];
}

// The run of group g in the faces sorted by group: gf[gstart[g] .. gend[g]).
__global__ __launch_bounds__(ATL_BLOCK) void atl_group_runs(const uint32_t* __restrict__ sg, long long F,
                                                           int32_t* __restrict__ gstart, int32_t* __restrict__ gend) {
  const long long i = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (i >= F) return;
  if (i == 0 || sg[i] != sg[i - 1]) gstart[sg[i]] = (int32_t)i;
  if (i == F - 1 || sg[i] != sg[i + 1]) gend[sg[i]] = (int32_t)(i + 1);
}

// A_g = 0 + the fp64 n_f of the group's faces in ascending face index.  One wave per group: the lanes load 64 faces'
// normals at once, and every lane adds them one after the other in lane order, so the order is the rule's while the
// loads run side by side (one lane walking a sphere's 25 000-face chart alone is a chain of as many dependent loads).
__global__ __launch_bounds__(VSA_WAVE) void atl_group_area(const float* __restrict__ fn, const uint32_t* __restrict__ gf,
                                                          const int32_t* __restrict__ gstart,
                                                          const int32_t* __restrict__ gend,
                                                          const int32_t* __restrict__ glist, double* __restrict__ gA) {
  const long long g = glist[blockIdx.x];
  const int lane = threadIdx.x, end = gend[g];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int i = gstart[g]; i < end; i += VSA_WAVE) {
    double x = 0.0, y = 0.0, z = 0.0;
    if (i + lane < end) {
      const long long f = gf[i + lane];
      x = (double)fn[3 * f];
      y = (double)fn[3 * f + 1];
      z = (double)fn[3 * f + 2];
    }
    const int m = end - i < VSA_WAVE ? end - i : VSA_WAVE;
    for (int k = 0; k < m; ++k) {
      sx += __shfl(x, k, VSA_WAVE);
      sy += __shfl(y, k, VSA_WAVE);
      sz += __shfl(z, k, VSA_WAVE);
    }
  }
  if (lane == 0) {
    gA[3 * g] = sx;
    gA[3 * g + 1] = sy;
    gA[3 * g + 2] = sz;
  }
}

// Key of an eligible edge between two groups: lo << s | hi at s = the bits of F - 1; all ones inside one group (no
// key of two groups is: lo < hi < 2^s).
__global__ __launch_bounds__(ATL_BLOCK) void atl_pair_keys(const int2* __restrict__ pairs, long long E,
                                                          const int32_t* __restrict__ grp, int s,
                                                          u64* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (i >= E) return;
  const int2 pr = pairs[i];
  const unsigned a = (unsigned)grp[pr.x], b = (unsigned)grp[pr.y];
  keys[i] = a == b ? (1ull << (2 * s)) - 1ull : (u64)(a < b ? a : b) << s | (u64)(a < b ? b : a);
}

__global__ __launch_bounds__(ATL_BLOCK) void atl_pair_heads(const u64* __restrict__ sk, long long E, int s,
                                                           int32_t* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (i >= E) return;
  flags[i] = sk[i] != (1ull << (2 * s)) - 1ull && (i == 0 || sk[i - 1] != sk[i]);
}

// Pair j = the j-th run of equal keys: its groups, and its run [pstart, pend) (the weight is the run's length).
__global__ __launch_bounds__(ATL_BLOCK) void atl_pair_runs(const u64* __restrict__ sk, const int32_t* __restrict__ flags,
                                                          const int32_t* __restrict__ rank, long long E, int s,
                                                          int2* __restrict__ gp, int32_t* __restrict__ pstart,
                                                          int32_t* __restrict__ pend, long long* __restrict__ ctr) {
  const long long i = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (i >= E) return;
  const u64 k = sk[i];
  if (k != (1ull << (2 * s)) - 1ull) {
    const long long j = rank[i] + flags[i] - 1;
    if (flags[i]) {
      gp[j] = make_int2((int)(k >> s), (int)(k & ((1ull << s) - 1ull)));
      pstart[j] = (int32_t)i;
    }
    if (i == E - 1 || sk[i + 1] != k) pend[j] = (int32_t)(i + 1);
  }
  if (i == E - 1) ctr[ACT_NP] = rank[i] + flags[i];
}

// cnt[j] = the (face, pair) items of pair j: the faces of both groups (0 past the last pair).  Pairs start valid, and
// the picks of their groups empty.
__global__ __launch_bounds__(ATL_BLOCK) void atl_pair_items(const int2* __restrict__ gp, long long E,
                                                           const long long* __restrict__ ctr,
                                                           const int32_t* __restrict__ gstart,
                                                           const int32_t* __restrict__ gend,
                                                           long long* __restrict__ cnt, int32_t* __restrict__ valid,
                                                           u64* __restrict__ best) {
  const long long j = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (j >= E) return;
  if (j >= ctr[ACT_NP]) {
    cnt[j] = 0;
    return;
  }
  const int2 ab = gp[j];
  cnt[j] = (long long)(gend[ab.x] - gstart[ab.x]) + (long long)(gend[ab.y] - gstart[ab.y]);
  valid[j] = 1;
  best[ab.x] = 0ull;   // (every lane that writes one writes 0)
  best[ab.y] = 0ull;
}

// One lane per (face, pair) item, ioff[j] = the items before pair j: the face against D = A_a + A_b in fp64; a face
// that fails clears its pair's flag.
__global__ __launch_bounds__(ATL_BLOCK) void atl_validity(const long long* __restrict__ ioff,
                                                         const long long* __restrict__ ctr,
                                                         const int2* __restrict__ gp,
                                                         const int32_t* __restrict__ gstart,
                                                         const int32_t* __restrict__ gend,
                                                         const uint32_t* __restrict__ gf, const float* __restrict__ fn,
                                                         const double* __restrict__ gA, double tt,
                                                         int32_t* __restrict__ valid) {
  const long long np = ctr[ACT_NP];
  if (np <= 0) return;
  const long long total = ioff[np];
  for (long long it = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x; it < total;
       it += (long long)gridDim.x * ATL_BLOCK) {
    long long lo = 0, hi = np - 1;   // the last pair with ioff[j] <= it
    while (lo < hi) {
      const long long mid = lo + (hi - lo + 1) / 2;
      if (ioff[mid] <= it) lo = mid;
      else hi = mid - 1;
    }
    const int2 ab = gp[lo];
    const long long k = it - ioff[lo], na = gend[ab.x] - gstart[ab.x];
    const long long f = k < na ? gf[gstart[ab.x] + k] : gf[gstart[ab.y] + (k - na)];
    const float fx = fn[3 * f], fy = fn[3 * f + 1], fz = fn[3 * f + 2];
    if (fx == 0.f && fy == 0.f && fz == 0.f) continue;
    const double nx = fx, ny = fy, nz = fz;
    const double dx = gA[3 * (long long)ab.x] + gA[3 * (long long)ab.y];
    const double dy = gA[3 * (long long)ab.x + 1] + gA[3 * (long long)ab.y + 1];
    const double dz = gA[3 * (long long)ab.x + 2] + gA[3 * (long long)ab.y + 2];
    const double c = (nx * dx + ny * dy) + nz * dz;
    const double nn = (nx * nx + ny * ny) + nz * nz;
    const double dd = (dx * dx + dy * dy) + dz * dz;
    if (!(c > 0.0 && c * c >= (tt * nn) * dd)) atomicAnd(valid + lo, 0);
  }
}

// A pick is (weight << 32 | ~neighbour): the maximum is the largest weight, ties to the smaller group id.
__device__ __forceinline__ u64 atl_pick_key(int w, int g) { return (u64)(unsigned)w << 32 | (u64)(~(unsigned)g); }

__global__ __launch_bounds__(ATL_BLOCK) void atl_pick(const int2* __restrict__ gp, long long E,
                                                     const long long* __restrict__ ctr,
                                                     const int32_t* __restrict__ pstart,
                                                     const int32_t* __restrict__ pend,
                                                     const int32_t* __restrict__ valid, u64* __restrict__ best,
                                                     long long* __restrict__ nv) {
  const long long j = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  const bool ok = j < E && j < ctr[ACT_NP] && valid[j];
  if (ok) {
    const int2 ab = gp[j];
    const int w = pend[j] - pstart[j];
    atomicMax((unsigned long long*)(best + ab.x), (unsigned long long)atl_pick_key(w, ab.y));
    atomicMax((unsigned long long*)(best + ab.y), (unsigned long long)atl_pick_key(w, ab.x));
  }
  const u64 m = __ballot(ok);
  if ((threadIdx.x & (VSA_WAVE - 1)) == 0 && m) atomicAdd((unsigned long long*)nv, (unsigned long long)__popcll(m));
}

// Two groups that picked each other merge under the smaller id a: par[b] = a, A_a = A_a + A_b, a is marked merged.  A
// group is in at most one such pair, so no lane reads what another writes.
__global__ __launch_bounds__(ATL_BLOCK) void atl_merge(const int2* __restrict__ gp, long long E,
                                                      const long long* __restrict__ ctr,
                                                      const int32_t* __restrict__ pstart,
                                                      const int32_t* __restrict__ pend,
                                                      const int32_t* __restrict__ valid, const u64* __restrict__ best,
                                                      int32_t* __restrict__ par, double* __restrict__ gA,
                                                      int32_t* __restrict__ merged, long long* __restrict__ nm) {
  const long long j = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (j >= E || j >= ctr[ACT_NP] || !valid[j]) return;
  const int2 ab = gp[j];
  const int w = pend[j] - pstart[j];
  if (best[ab.x] != atl_pick_key(w, ab.y) || best[ab.y] != atl_pick_key(w, ab.x)) return;
  const long long a = ab.x, b = ab.y;
  par[b] = ab.x;
#pragma unroll
  for (int k = 0; k < 3; ++k) gA[3 * a + k] = gA[3 * a + k] + gA[3 * b + k];
  merged[a] = 1;
  atomicAdd((unsigned long long*)nm, 1ull);
}

__global__ __launch_bounds__(ATL_BLOCK) void atl_relabel(const int32_t* __restrict__ par, long long F,
                                                        int32_t* __restrict__ grp) {
  const long long f = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (f < F) grp[f] = par[grp[f]];
}

// Frame of a merged group (par[g] = g: it is one still), D = A_g: k the smallest |D_k| (ties to the earlier), t = e_k x
// D, b = D x t, each over the square root of its own squared length, in fp64.  fr[6 g ..] = (t, b).
__global__ __launch_bounds__(ATL_BLOCK) void atl_frames(const int32_t* __restrict__ par,
                                                       const int32_t* __restrict__ merged,
                                                       const double* __restrict__ gA, long long F,
                                                       double* __restrict__ fr) {
  const long long g = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (g >= F || par[g] != g || !merged[g]) return;
  const double dx = gA[3 * g], dy = gA[3 * g + 1], dz = gA[3 * g + 2];
  const double ax = fabs(dx), ay = fabs(dy), az = fabs(dz);
  const int k = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
  const double tx = k == 0 ? 0.0 : (k == 1 ? dz : -dy);
  const double ty = k == 0 ? -dz : (k == 1 ? 0.0 : dx);
  const double tz = k == 0 ? dy : (k == 1 ? -dx : 0.0);
  const double bx = dy * tz - dz * ty, by = dz * tx - dx * tz, bz = dx * ty - dy * tx;
  const double tl = sqrt((tx * tx + ty * ty) + tz * tz), bl = sqrt((bx * bx + by * by) + bz * bz);
  fr[6 * g] = tx / tl;
  fr[6 * g + 1] = ty / tl;
  fr[6 * g + 2] = tz / tl;
  fr[6 * g + 3] = bx / bl;
  fr[6 * g + 4] = by / bl;
  fr[6 * g + 5] = bz / bl;
}

// pc[f, c] = corner c's plane coordinates: the label's pick for a face of an unmerged group, (P . t, P . b) in fp64
// rounded once to fp32 for one of a merged group.
__global__ __launch_bounds__(ATL_BLOCK) void atl_plane_coords(const float* __restrict__ P,
                                                             const int32_t* __restrict__ faces, long long F,
                                                             const int32_t* __restrict__ label,
                                                             const int32_t* __restrict__ grp,
                                                             const int32_t* __restrict__ merged,
                                                             const double* __restrict__ fr, float* __restrict__ pc) {
  const long long f = (long long)blockIdx.x * ATL_BLOCK + threadIdx.x;
  if (f >= F) return;
  const long long g = grp[f];
  if (!merged[g]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float2 q = atl_corner<false>(P, faces, label, nullptr, f, c);
      pc[6 * f + 2 * c] = q.x;
      pc[6 * f + 2 * c + 1] = q.y;
    }
    return;
  }
  const double tx = fr[6 * g], ty = fr[6 * g + 1], tz = fr[6 * g + 2];
  const double bx = fr[6 * g + 3], by = fr[6 * g + 4], bz = fr[6 * g + 5];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long v = faces[3 * f + c];
    const double x = P[3 * v], y = P[3 * v + 1], z = P[3 * v + 2];
    pc[6 * f + 2 * c] = (float)((x * tx + y * ty) + z * tz);
    pc[6 * f + 2 * c + 1] = (float)((x * bx + y * by) + z * bz);
  }
}

// ------------------------------------------------------------------------------------------------ host

struct AtlLayout {
  size_t fn, nv, vstart, vend, label, code, par, cidx, flags, rank, A, B, va, vb, pairs, box, off, flag, pre, wid,
      sh_start, sh_y, toff, ntile, count, ctr, tmp, tmp_bytes, total;
  // vsa_atlas_merged
  size_t grp, sg, gf, fiota, gstart, gend, glist, merged, gA, fr, best, pc, gp, pstart, pend, valid, cnt, ioff;
};

static int atl_check(long long V, long long F, int R) {
  if (R < ATL_MIN_RES || R > ATL_MAX_RES) return VSA_ERR_ARG;
  return mt::check_vf(V, F);
}

// V = 0: the rasterize-only layout (toff, ntile, count unused, ctr, tmp).  merged: vsa_atlas_merged's buffers after
// vsa_atlas's, e = the most eligible edges (3F / 2) + 1.
static int atl_layout(long long V, long long F, int R, AtlLayout* l, bool merged = false) {
  const size_t v = (size_t)V, f = (size_t)F, n3 = 3 * f, rr = (size_t)R * (size_t)R, e = n3 / 2 + 1;
  const bool full = V > 0;
  mt::TmpCounts cnt = {};
  cnt.iscan64 = merged ? e : f;
  if (full) {
    cnt.pairs64 = n3;
    cnt.pairs32 = n3;
    cnt.keys64 = merged ? e : f;
    cnt.xscan32 = n3;
  }
  MT_TRY(mt::tmp_bytes(cnt, &l->tmp_bytes));
  mt::Bump b;
  l->toff = b.take(8 * (f + 1));
  l->ntile = b.take(8 * f);
  l->ctr = b.take(8 * ACT_N);
  l->fn = b.take(full ? 12 * f : 0);
  l->nv = b.take(12 * v);
  l->vstart = b.take(4 * v);
  l->vend = b.take(4 * v);
  l->label = b.take(full ? 4 * f : 0);
  l->code = b.take(full ? 4 * f : 0);
  l->par = b.take(full ? 4 * f : 0);
  l->cidx = b.take(full ? 4 * f : 0);
  l->flags = b.take(full ? 4 * n3 : 0);
  l->rank = b.take(full ? 4 * n3 : 0);
  l->A = b.take(full ? 8 * n3 : 0);
  l->B = b.take(full ? 8 * n3 : 0);
  l->va = b.take(full ? 4 * n3 : 0);
  l->vb = b.take(full ? 4 * n3 : 0);
  l->pairs = b.take(full ? 8 * n3 : 0);
  l->box = b.take(full ? 16 * f : 0);
  l->off = b.take(full ? 8 * f : 0);
  l->flag = b.take(full ? 4 * f : 0);
  l->pre = b.take(full ? 8 * (f + 1) : 0);
  l->wid = b.take(full ? 8 * f : 0);
  l->sh_start = b.take(full ? 4 * f : 0);
  l->sh_y = b.take(full ? 4 * f : 0);
  l->count = b.take(full ? 4 * rr : 0);
  l->tmp = b.take(l->tmp_bytes);
  if (merged) {
    l->grp = b.take(4 * f);
    l->sg = b.take(4 * f);
    l->gf = b.take(4 * f);
    l->fiota = b.take(4 * f);
    l->gstart = b.take(4 * f);
    l->gend = b.take(4 * f);
    l->glist = b.take(4 * f);
    l->merged = b.take(4 * f);
    l->gA = b.take(24 * f);
    l->fr = b.take(48 * f);
    l->best = b.take(8 * f);
    l->pc = b.take(24 * f);
    l->gp = b.take(8 * e);
    l->pstart = b.take(4 * e);
    l->pend = b.take(4 * e);
    l->valid = b.take(4 * e);
    l->cnt = b.take(8 * e);
    l->ioff = b.take(8 * (e + 1));
  }
  l->total = b.o;
  return VSA_OK;
}

extern "C" long long vsa_atlas_workspace_bytes(long long nr_verts, long long nr_faces, int resolution) {
  AtlLayout l;
  int rc = atl_check(nr_verts, nr_faces, resolution);
  if (rc == VSA_OK) rc = mt::abi_status(atl_layout(nr_verts, nr_faces, resolution, &l));
  return rc != VSA_OK ? rc : (long long)l.total;
}

extern "C" long long vsa_atlas_merged_workspace_bytes(long long nr_verts, long long nr_faces, int resolution) {
  AtlLayout l;
  int rc = atl_check(nr_verts, nr_faces, resolution);
  if (rc == VSA_OK) rc = mt::abi_status(atl_layout(nr_verts, nr_faces, resolution, &l, true));
  return rc != VSA_OK ? rc : (long long)l.total;
}

extern "C" long long vsa_atlas_rasterize_workspace_bytes(long long nr_faces) {
  if (nr_faces < 1) return VSA_ERR_ARG;
  if (nr_faces > 0x7FFFFFFFll) return VSA_ERR_UNSUPPORTED;
  AtlLayout l;
  const int rc = mt::abi_status(atl_layout(0, nr_faces, ATL_MIN_RES, &l));
  return rc != VSA_OK ? rc : (long long)l.total;
}

namespace {

struct Atl {
  hipStream_t st;
  char* ws;
  AtlLayout l;
  mt::Tmp tmp;
  long long V, F, C;
  int R, p, s_bits;
  const float* P;
  const int32_t* faces;
  long long* ctr;
  mt::StageTimer timer;
  // vsa_atlas_merged: charts are built inside groups and laid out from plane coordinates
  bool merged;
  double min_cos;
  int merge_rounds;
  long long mstats[4];   // box charts, groups, merge rounds run, valid pairs left
};

// Rasterization of F faces' UVs: tile counts, their scan and the item passes (mode 0 counts, then mode 1 flags when
// `flag` is given).  count / face_id must be zeroed / 0xFF-filled by the caller.
int raster(hipStream_t st, char* ws, const AtlLayout& l, const float* uv, long long F, int R, int32_t* count,
           uint32_t* face_id, const int32_t* cidx, int32_t* flag) {
  long long* toff = at<long long>(ws, l.toff);
  long long* ntile = at<long long>(ws, l.ntile);
  hipLaunchKernelGGL(atl_tile_counts, mt::grid(F), dim3(ATL_BLOCK), 0, st, uv, F, R, ntile);
  MT_LAUNCHED();
  VSA_HIP_TRY(hipMemsetAsync(toff, 0, 8, st));
  MT_TRY(mt::inclusive_scan({ws + l.tmp, l.tmp_bytes}, ntile, toff + 1, (size_t)F, st));
  long long total = 0;
  MT_TRY(mt::read_counters(st, toff + F, &total));
  if (total < 0) return VSA_ERR_UNSUPPORTED;
  if (total == 0) return VSA_OK;
  const long long blocks = (total + ATL_BLOCK - 1) / ATL_BLOCK;
  const dim3 g((unsigned)(blocks < 65536 ? blocks : 65536));
  hipLaunchKernelGGL(atl_raster, g, dim3(ATL_BLOCK), 0, st, uv, F, R, toff, total, 0, count, face_id, cidx, flag);
  MT_LAUNCHED();
  if (flag) {
    hipLaunchKernelGGL(atl_raster, g, dim3(ATL_BLOCK), 0, st, uv, F, R, toff, total, 1, count, face_id, cidx, flag);
    MT_LAUNCHED();
  }
  return VSA_OK;
}

int label_stage(Atl& m) {
  const long long F = m.F, V = m.V, n3 = 3 * F;
  char* ws = m.ws;
  const AtlLayout& l = m.l;
  float* fn = at<float>(ws, l.fn);
  hipLaunchKernelGGL(atl_normals, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, m.P, m.faces, F, fn);
  MT_LAUNCHED();
  uint32_t* kin = at<uint32_t>(ws, l.A);
  uint32_t* kout = at<uint32_t>(ws, l.B);
  uint32_t* vin = at<uint32_t>(ws, l.va);
  uint32_t* vff = at<uint32_t>(ws, l.vb);
  int32_t* vstart = at<int32_t>(ws, l.vstart);
  int32_t* vend = at<int32_t>(ws, l.vend);
  MT_TRY(mt::vertex_rings(m.faces, F, V, m.s_bits, kin, kout, vin, vff, vstart, vend, m.tmp, m.st));
  float* nv = at<float>(ws, l.nv);
  hipLaunchKernelGGL(atl_vertex_sums, mt::grid(V), dim3(ATL_BLOCK), 0, m.st, fn, vff, vstart, vend, V, nv);
  MT_LAUNCHED();
  int32_t* label = at<int32_t>(ws, l.label);
  hipLaunchKernelGGL(atl_labels, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, m.faces, F, fn, nv, label,
                     at<uint32_t>(ws, l.code));
  MT_LAUNCHED();
  // edges -> join pairs
  u64* ek = at<u64>(ws, l.A);
  u64* es = at<u64>(ws, l.B);
  uint32_t* slot = at<uint32_t>(ws, l.vb);
  MT_TRY(mt::sorted_edges(m.faces, F, m.s_bits, ek, es, vin, slot, m.tmp, m.st));
  int32_t* flags = at<int32_t>(ws, l.flags);
  int32_t* rank = at<int32_t>(ws, l.rank);
  hipLaunchKernelGGL(atl_join_flags, mt::grid(n3), dim3(ATL_BLOCK), 0, m.st, es, slot, m.faces,
                     m.merged ? nullptr : label, n3, flags);
  MT_LAUNCHED();
  MT_TRY(mt::exclusive_scan(m.tmp, flags, rank, (size_t)n3, m.st));
  hipLaunchKernelGGL(atl_join_compact, mt::grid(n3), dim3(ATL_BLOCK), 0, m.st, slot, flags, rank, n3,
                     at<int2>(ws, l.pairs), m.ctr);
  MT_LAUNCHED();
  return VSA_OK;
}

int chart_stage(Atl& m) {
  const long long F = m.F;
  char* ws = m.ws;
  const AtlLayout& l = m.l;
  int32_t* par = at<int32_t>(ws, l.par);
  int32_t* flags = at<int32_t>(ws, l.flags);
  int32_t* rank = at<int32_t>(ws, l.rank);
  MT_TRY(mt::iota(par, F, m.st));
  // J <= 3F / 2: the grid covers every pair, the kernel reads J on the device
  hipLaunchKernelGGL(atl_hook, mt::grid(3 * F / 2 + 1), dim3(ATL_BLOCK), 0, m.st, at<int2>(ws, l.pairs), m.ctr,
                     at<uint32_t>(ws, l.code), m.merged ? at<int32_t>(ws, l.grp) : nullptr, par);
  MT_LAUNCHED();
  int32_t* cidx = at<int32_t>(ws, l.cidx);
  MT_TRY(mt::roots(par, F, cidx, flags, m.st));
  MT_TRY(mt::exclusive_scan(m.tmp, flags, rank, (size_t)F, m.st));
  hipLaunchKernelGGL(atl_chart_index, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, flags, rank, F, cidx, m.ctr);
  MT_LAUNCHED();
  MT_TRY(mt::read_counters(m.st, m.ctr + ACT_C, &m.C));
  if (m.C < 1 || m.C > F) return VSA_ERR_UNSUPPORTED;
  unsigned* box = at<unsigned>(ws, l.box);
  hipLaunchKernelGGL(atl_box_init, mt::grid(4 * m.C), dim3(ATL_BLOCK), 0, m.st, box, 4 * m.C);
  MT_LAUNCHED();
  if (m.merged)
    hipLaunchKernelGGL(atl_boxes<true>, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, m.P, m.faces, F,
                       at<int32_t>(ws, l.label), at<float>(ws, l.pc), cidx, box);
  else
    hipLaunchKernelGGL(atl_boxes<false>, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, m.P, m.faces, F,
                       at<int32_t>(ws, l.label), nullptr, cidx, box);
  MT_LAUNCHED();
  return VSA_OK;
}

// One shelf walk at density bits `sb`; returns the fit flag in *fit.
int pack_step(Atl& m, uint32_t sb, int emit, long long* fit) {
  char* ws = m.ws;
  const AtlLayout& l = m.l;
  const long long C = m.C;
  float s;
  memcpy(&s, &sb, 4);
  u64* keys = at<u64>(ws, l.A);
  u64* sorted = at<u64>(ws, l.B);
  long long* wid = at<long long>(ws, l.wid);
  long long* pre = at<long long>(ws, l.pre);
  hipLaunchKernelGGL(atl_rect_keys, mt::grid(C), dim3(ATL_BLOCK), 0, m.st, at<unsigned>(ws, l.box), C, s, m.R, m.p, keys);
  MT_LAUNCHED();
  MT_TRY(mt::sort_keys(m.tmp, keys, sorted, (size_t)C, 0, 64, m.st));
  hipLaunchKernelGGL(atl_rect_widths, mt::grid(C), dim3(ATL_BLOCK), 0, m.st, sorted, C, wid);
  MT_LAUNCHED();
  VSA_HIP_TRY(hipMemsetAsync(pre, 0, 8, m.st));
  MT_TRY(mt::inclusive_scan(m.tmp, wid, pre + 1, (size_t)C, m.st));
  hipLaunchKernelGGL(atl_shelf_walk, dim3(1), dim3(1), 0, m.st, sorted, pre, C, m.R, emit,
                     at<int32_t>(ws, l.sh_start), at<int32_t>(ws, l.sh_y), m.ctr);
  MT_LAUNCHED();
  return mt::read_counters(m.st, m.ctr + ACT_FIT, fit);
}

// Smallest resolution at which C charts of (2p)^2 texels fit by next-fit shelves.
long long min_resolution(long long C, int p) {
  const long long side = 2ll * p;
  for (long long r = side;; ++r) {
    const long long per = r / side;
    if (per > 0 && ((C + per - 1) / per) * side <= r) return r;
  }
}

int pack_stage(Atl& m, uint32_t* s_out, long long* minres) {
  const long long C = m.C;
  if (m.p > 0) {
    const long long side = 2ll * m.p, per = m.R / side;
    if (per == 0 || ((C + per - 1) / per) * side > m.R) {
      *minres = min_resolution(C, m.p);
      return VSA_ERR_ATLAS_FULL;
    }
  }
  uint32_t lo = 0u, hi = 0x7F800000u;   // fits(lo); hi (+inf) is never tried
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    long long fit = 0;
    MT_TRY(pack_step(m, mid, 0, &fit));
    if (fit) lo = mid;
    else hi = mid;
  }
  long long fit = 0;
  MT_TRY(pack_step(m, lo, 1, &fit));
  if (!fit) return VSA_ERR_UNSUPPORTED;
  char* ws = m.ws;
  const AtlLayout& l = m.l;
  hipLaunchKernelGGL(atl_offsets, mt::grid(C), dim3(ATL_BLOCK), 0, m.st, at<u64>(ws, l.B), at<long long>(ws, l.pre), C,
                     at<int32_t>(ws, l.sh_start), at<int32_t>(ws, l.sh_y), m.ctr, at<int2>(ws, l.off));
  MT_LAUNCHED();
  *s_out = lo;
  return VSA_OK;
}

// The faces sorted by group (ascending face within a group) and every group's run in them.
int group_faces(Atl& m) {
  char* ws = m.ws;
  const AtlLayout& l = m.l;
  uint32_t* sg = at<uint32_t>(ws, l.sg);
  MT_TRY(mt::sort_pairs(m.tmp, at<uint32_t>(ws, l.grp), sg, at<uint32_t>(ws, l.fiota), at<uint32_t>(ws, l.gf),
                        (size_t)m.F, 0, mt::bits_of(m.F), m.st));
  hipLaunchKernelGGL(atl_group_runs, mt::grid(m.F), dim3(ATL_BLOCK), 0, m.st, sg, m.F, at<int32_t>(ws, l.gstart),
                     at<int32_t>(ws, l.gend));
  MT_LAUNCHED();
  return VSA_OK;
}

// The box charts as groups, then merge rounds (header rules 1 - 5) and the plane coordinates of every corner.  The
// host reads the edge and box-chart counts once, the valid-pair count once per round, and the merge count at the end.
int merge_stage(Atl& m) {
  const long long F = m.F;
  char* ws = m.ws;
  const AtlLayout& l = m.l;
  int32_t* par = at<int32_t>(ws, l.par);
  int32_t* grp = at<int32_t>(ws, l.grp);
  int32_t* flags = at<int32_t>(ws, l.flags);
  int32_t* rank = at<int32_t>(ws, l.rank);
  int32_t* label = at<int32_t>(ws, l.label);
  int32_t* merged = at<int32_t>(ws, l.merged);
  int32_t* gstart = at<int32_t>(ws, l.gstart);
  int32_t* gend = at<int32_t>(ws, l.gend);
  uint32_t* gf = at<uint32_t>(ws, l.gf);
  float* fn = at<float>(ws, l.fn);
  double* gA = at<double>(ws, l.gA);
  int2* pairs = at<int2>(ws, l.pairs);
  // groups = the box charts: the eligible edges between faces of one label
  MT_TRY(mt::iota(par, F, m.st));
  hipLaunchKernelGGL(atl_hook, mt::grid(3 * F / 2 + 1), dim3(ATL_BLOCK), 0, m.st, pairs, m.ctr, at<uint32_t>(ws, l.code),
                     label, par);
  MT_LAUNCHED();
  MT_TRY(mt::roots(par, F, grp, flags, m.st));
  MT_TRY(mt::exclusive_scan(m.tmp, flags, rank, (size_t)F, m.st));
  hipLaunchKernelGGL(atl_group_list, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, flags, rank, F, at<int32_t>(ws, l.glist),
                     m.ctr);
  MT_LAUNCHED();
  MT_TRY(mt::iota(at<int32_t>(ws, l.fiota), F, m.st));
  VSA_HIP_TRY(hipMemsetAsync(merged, 0, 4 * (size_t)F, m.st));
  MT_TRY(group_faces(m));
  long long ctr[ACT_N];
  MT_TRY(mt::read_counters(m.st, m.ctr, ctr, ACT_N));
  const long long E = ctr[ACT_J], box = ctr[ACT_BOX];
  if (E < 0 || E > 3 * F / 2 || box < 1 || box > F) return VSA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(atl_group_area, dim3((unsigned)box), dim3(VSA_WAVE), 0, m.st, fn, gf, gstart, gend,
                     at<int32_t>(ws, l.glist), gA);
  MT_LAUNCHED();
  const int s = mt::bits_of(F);
  const double tt = m.min_cos * m.min_cos;
  u64* keys = at<u64>(ws, l.A);
  u64* sk = at<u64>(ws, l.B);
  int2* gp = at<int2>(ws, l.gp);
  int32_t* pstart = at<int32_t>(ws, l.pstart);
  int32_t* pend = at<int32_t>(ws, l.pend);
  int32_t* valid = at<int32_t>(ws, l.valid);
  long long* cnt = at<long long>(ws, l.cnt);
  long long* ioff = at<long long>(ws, l.ioff);
  u64* best = at<u64>(ws, l.best);
  long long rounds = 0, nv = 0;
  // item lanes: enough to fill the device, each walking its share of the (face, pair) items
  const long long vb = (8 * F + ATL_BLOCK - 1) / ATL_BLOCK;
  const dim3 vgrid((unsigned)(vb < 64 ? 64 : (vb > 65536 ? 65536 : vb)));
  while (E > 0) {
    hipLaunchKernelGGL(atl_pair_keys, mt::grid(E), dim3(ATL_BLOCK), 0, m.st, pairs, E, grp, s, keys);
    MT_LAUNCHED();
    MT_TRY(mt::sort_keys(m.tmp, keys, sk, (size_t)E, 0, 2 * s, m.st));
    hipLaunchKernelGGL(atl_pair_heads, mt::grid(E), dim3(ATL_BLOCK), 0, m.st, sk, E, s, flags);
    MT_LAUNCHED();
    MT_TRY(mt::exclusive_scan(m.tmp, flags, rank, (size_t)E, m.st));
    hipLaunchKernelGGL(atl_pair_runs, mt::grid(E), dim3(ATL_BLOCK), 0, m.st, sk, flags, rank, E, s, gp, pstart, pend,
                       m.ctr);
    MT_LAUNCHED();
    hipLaunchKernelGGL(atl_pair_items, mt::grid(E), dim3(ATL_BLOCK), 0, m.st, gp, E, m.ctr, gstart, gend, cnt, valid,
                       best);
    MT_LAUNCHED();
    VSA_HIP_TRY(hipMemsetAsync(ioff, 0, 8, m.st));
    MT_TRY(mt::inclusive_scan(m.tmp, cnt, ioff + 1, (size_t)E, m.st));
    hipLaunchKernelGGL(atl_validity, vgrid, dim3(ATL_BLOCK), 0, m.st, ioff, m.ctr, gp, gstart, gend, gf, fn, gA, tt,
                       valid);
    MT_LAUNCHED();
    VSA_HIP_TRY(hipMemsetAsync(m.ctr + ACT_NV, 0, 8, m.st));
    hipLaunchKernelGGL(atl_pick, mt::grid(E), dim3(ATL_BLOCK), 0, m.st, gp, E, m.ctr, pstart, pend, valid, best,
                       m.ctr + ACT_NV);
    MT_LAUNCHED();
    MT_TRY(mt::read_counters(m.st, m.ctr + ACT_NV, &nv));
    if (rounds == m.merge_rounds) break;
    ++rounds;   // (the round that finds no valid pair counts)
    if (nv == 0) break;
    hipLaunchKernelGGL(atl_merge, mt::grid(E), dim3(ATL_BLOCK), 0, m.st, gp, E, m.ctr, pstart, pend, valid, best, par,
                       gA, merged, m.ctr + ACT_MERGES);
    MT_LAUNCHED();
    hipLaunchKernelGGL(atl_relabel, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, par, F, grp);
    MT_LAUNCHED();
    MT_TRY(group_faces(m));
  }
  if (E == 0 && m.merge_rounds > 0) rounds = 1;   // no pair at all: the one round that finds none
  long long merges = 0;
  MT_TRY(mt::read_counters(m.st, m.ctr + ACT_MERGES, &merges));
  if (merges < 0 || merges >= box) return VSA_ERR_UNSUPPORTED;
  m.mstats[0] = box;
  m.mstats[1] = box - merges;
  m.mstats[2] = rounds;
  m.mstats[3] = nv;
  hipLaunchKernelGGL(atl_frames, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, par, merged, gA, F, at<double>(ws, l.fr));
  MT_LAUNCHED();
  hipLaunchKernelGGL(atl_plane_coords, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, m.P, m.faces, F, label, grp, merged,
                     at<double>(ws, l.fr), at<float>(ws, l.pc));
  MT_LAUNCHED();
  return VSA_OK;
}

int run(Atl& m, float* uv, int32_t* out_chart, long long* stats, float* scale) {
  char* ws = m.ws;
  const AtlLayout& l = m.l;
  const long long F = m.F;
  VSA_HIP_TRY(hipMemsetAsync(m.ctr, 0, 8 * ACT_N, m.st));
  MT_TRY(m.timer.open());
  MT_TRY(label_stage(m));
  MT_TRY(m.timer.close(0));
  if (m.merged) {
    MT_TRY(m.timer.open());
    MT_TRY(merge_stage(m));
    MT_TRY(m.timer.close(5));
  }
  int32_t* count = at<int32_t>(ws, l.count);
  int32_t* flag = at<int32_t>(ws, l.flag);
  int32_t* cidx = at<int32_t>(ws, l.cidx);
  long long splits = 0;
  uint32_t sb = 0;
  while (true) {
    MT_TRY(m.timer.open());
    MT_TRY(chart_stage(m));
    MT_TRY(m.timer.close(1));
    MT_TRY(m.timer.open());
    long long minres = 0;
    const int rc = pack_stage(m, &sb, &minres);
    if (rc == VSA_ERR_ATLAS_FULL) {
      stats[0] = m.C;
      stats[1] = splits;
      stats[2] = 0;
      stats[3] = minres;
      if (m.merged) memcpy(stats + 4, m.mstats, sizeof(m.mstats));
    }
    if (rc != VSA_OK) return rc;
    MT_TRY(m.timer.close(2));
    MT_TRY(m.timer.open());
    float s;
    memcpy(&s, &sb, 4);
    if (m.merged)
      hipLaunchKernelGGL(atl_emit<true>, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, m.P, m.faces, F,
                         at<int32_t>(ws, l.label), at<float>(ws, l.pc), cidx, at<unsigned>(ws, l.box),
                         at<int2>(ws, l.off), s, m.R, m.p, uv);
    else
      hipLaunchKernelGGL(atl_emit<false>, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, m.P, m.faces, F,
                         at<int32_t>(ws, l.label), nullptr, cidx, at<unsigned>(ws, l.box), at<int2>(ws, l.off), s, m.R,
                         m.p, uv);
    MT_LAUNCHED();
    MT_TRY(m.timer.close(3));
    MT_TRY(m.timer.open());
    VSA_HIP_TRY(hipMemsetAsync(count, 0, 4 * (size_t)m.R * (size_t)m.R, m.st));
    VSA_HIP_TRY(hipMemsetAsync(flag, 0, 4 * (size_t)m.C, m.st));
    VSA_HIP_TRY(hipMemsetAsync(m.ctr + ACT_OVL, 0, 16, m.st));
    MT_TRY(raster(m.st, ws, l, uv, F, m.R, count, nullptr, cidx, flag));
    hipLaunchKernelGGL(atl_count_flags, mt::grid(m.C), dim3(ATL_BLOCK), 0, m.st, flag, m.C, m.ctr);
    MT_LAUNCHED();
    long long ovl = 0;
    MT_TRY(mt::read_counters(m.st, m.ctr + ACT_OVL, &ovl));
    if (ovl == 0) {
      const long long rr = (long long)m.R * m.R;
      hipLaunchKernelGGL(atl_covered, mt::grid(rr), dim3(ATL_BLOCK), 0, m.st, count, rr, m.ctr);
      MT_LAUNCHED();
      VSA_HIP_TRY(hipMemcpyAsync(out_chart, cidx, 4 * (size_t)F, hipMemcpyDeviceToDevice, m.st));
      long long cov = 0;
      MT_TRY(mt::read_counters(m.st, m.ctr + ACT_COV, &cov));
      MT_TRY(m.timer.close(4));
      stats[0] = m.C;
      stats[1] = splits;
      stats[2] = cov;
      stats[3] = 0;
      if (m.merged) memcpy(stats + 4, m.mstats, sizeof(m.mstats));
      memcpy(scale, &sb, 4);
      return VSA_OK;
    }
    // a texel counted twice across two charts, or one-face charts flagged, would repeat the round unchanged
    if (splits + 1 >= ATL_MAX_ROUNDS) return VSA_ERR_UNSUPPORTED;
    VSA_HIP_TRY(hipMemsetAsync(m.ctr + ACT_PROG, 0, 8, m.st));
    if (m.merged)
      hipLaunchKernelGGL(atl_split<true>, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, m.P, m.faces, F,
                         at<int32_t>(ws, l.label), at<float>(ws, l.pc), cidx, at<unsigned>(ws, l.box), flag,
                         at<uint32_t>(ws, l.code), m.ctr);
    else
      hipLaunchKernelGGL(atl_split<false>, mt::grid(F), dim3(ATL_BLOCK), 0, m.st, m.P, m.faces, F,
                         at<int32_t>(ws, l.label), nullptr, cidx, at<unsigned>(ws, l.box), flag,
                         at<uint32_t>(ws, l.code), m.ctr);
    MT_LAUNCHED();
    long long changed = 0;
    MT_TRY(mt::read_counters(m.st, m.ctr + ACT_PROG, &changed));
    if (changed == 0) return VSA_ERR_UNSUPPORTED;
    MT_TRY(m.timer.close(4));
    ++splits;
  }
}

// The body of both entries: merged = vsa_atlas_merged's groups and plane coordinates.
int atlas(bool merged, double min_cos, int merge_rounds, const float* verts, long long nr_verts, const int32_t* faces,
          long long nr_faces, int resolution, int padding, void* workspace, long long workspace_bytes,
          float* out_faces_uvs, int32_t* out_chart, long long* stats, float* scale, float* stage_ms, void* stream) {
  if (!verts || !faces || !workspace || !out_faces_uvs || !out_chart || !stats || !scale) return VSA_ERR_ARG;
  MT_TRY(atl_check(nr_verts, nr_faces, resolution));
  if (padding < 0 || 2 * padding >= resolution) return VSA_ERR_ARG;
  Atl m;
  MT_TRY(mt::abi_status(atl_layout(nr_verts, nr_faces, resolution, &m.l, merged)));
  m.merged = merged;
  m.min_cos = min_cos;
  m.merge_rounds = merge_rounds;
  if (workspace_bytes < (long long)m.l.total) return VSA_ERR_ARG;
  m.st = (hipStream_t)stream;
  m.ws = static_cast<char*>(workspace);
  m.tmp = {m.ws + m.l.tmp, m.l.tmp_bytes};
  m.V = nr_verts;
  m.F = nr_faces;
  m.C = 0;
  m.R = resolution;
  m.p = padding;
  m.P = verts;
  m.faces = faces;
  m.s_bits = mt::bits_of(nr_verts);
  m.ctr = at<long long>(m.ws, m.l.ctr);
  MT_TRY(m.timer.create(stage_ms, merged ? 6 : 5, m.st));
  const int rc = run(m, out_faces_uvs, out_chart, stats, scale);
  m.timer.destroy();
  return rc;
}

}  // namespace

extern "C" int vsa_atlas(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                         int resolution, int padding, void* workspace, long long workspace_bytes, float* out_faces_uvs,
                         int32_t* out_chart, long long* stats, float* scale, float* stage_ms, void* stream) {
  return atlas(false, 0.0, 0, verts, nr_verts, faces, nr_faces, resolution, padding, workspace, workspace_bytes,
               out_faces_uvs, out_chart, stats, scale, stage_ms, stream);
}

extern "C" int vsa_atlas_merged(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                                int resolution, int padding, double min_cos, int merge_rounds, void* workspace,
                                long long workspace_bytes, float* out_faces_uvs, int32_t* out_chart, long long* stats,
                                float* scale, float* stage_ms, void* stream) {
  if (!(min_cos > 0.0 && min_cos <= 1.0) || merge_rounds < 0) return VSA_ERR_ARG;   // (a NaN fails the first test)
  return atlas(true, min_cos, merge_rounds, verts, nr_verts, faces, nr_faces, resolution, padding, workspace,
               workspace_bytes, out_faces_uvs, out_chart, stats, scale, stage_ms, stream);
}

extern "C" int vsa_atlas_rasterize(const float* faces_uvs, long long nr_faces, int resolution, void* workspace,
                                   long long workspace_bytes, int32_t* out_face_id, int32_t* out_count, void* stream) {
  if (!faces_uvs || !workspace || !out_face_id || !out_count) return VSA_ERR_ARG;
  if (nr_faces < 1 || resolution < ATL_MIN_RES || resolution > ATL_MAX_RES) return VSA_ERR_ARG;
  if (nr_faces > 0x7FFFFFFFll) return VSA_ERR_UNSUPPORTED;
  AtlLayout l;
  MT_TRY(mt::abi_status(atl_layout(0, nr_faces, resolution, &l)));
  if (workspace_bytes < (long long)l.total) return VSA_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t rr = (size_t)resolution * (size_t)resolution;
  VSA_HIP_TRY(hipMemsetAsync(out_count, 0, 4 * rr, st));
  VSA_HIP_TRY(hipMemsetAsync(out_face_id, 0xFF, 4 * rr, st));
  MT_TRY(raster(st, static_cast<char*>(workspace), l, faces_uvs, nr_faces, resolution, out_count,
                reinterpret_cast<uint32_t*>(out_face_id), nullptr, nullptr));
  VSA_HIP_TRY(hipStreamSynchronize(st));
  return VSA_OK;
}
