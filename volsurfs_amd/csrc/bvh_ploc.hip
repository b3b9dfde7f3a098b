// PLOC topology for the device BVH builder (RayTracer(builder="ploc"), vsa_bvh_dev_build_ploc).
//
// Parallel Locally-Ordered Clustering (Meister & Bittner 2018, "Parallel Locally-Ordered Clustering for BVH
// construction") over the Morton-sorted triangles of csrc/bvh_device.hip (steps 1-4 there, unchanged).  It starts
// from one cluster per sorted triangle, holding its un-padded box, and repeats until one cluster is left:
//   a. nearest neighbour: cluster i picks the j != i with |i - j| <= radius whose union with it has the smallest
//      surface area; one LDS window per block holds the block's clusters and `radius` of halo on each side;
//   b. survivors: a rocPRIM exclusive scan of "i survives" (i is not the higher end of a mutual pair);
//   c. merge: a mutual pair (nn[nn[i]] == i) becomes one internal node at the lower position, left child = the lower
//      cluster, box = the min / max union, with its subtree's triangle count; every survivor moves to its scanned
//      position, so the array stays in Morton order.
// Ties break on the pair key (area, |i - j|, parity of min(i, j), min(i, j)): one total order on unordered pairs,
// computed alike from both ends, so the globally smallest pair is always mutual and every iteration with two or
// more clusters merges at least one pair.  (The parity term pairs (2k, 2k + 1) when every area is equal: equal
// boxes still halve per iteration.)  Each merge removes one cluster, and the node it makes is numbered by the
// removals before it: the n - 1 nodes are 0 .. n - 2 in merge order, the same every build, the root n - 2.
// Iterations hand over at kernel boundaries only.  The live count stays on the device (ping-pong between two
// words); the host enqueues a batch of iterations without a sync and reads the count once per batch; kernels past
// convergence exit at once.  The host bounds the loop at n - 1 iterations.
// Finally one thread per node walks up over the subtree counts to its first leaf position and writes the tree in the
// form bvh_device.hip's steps 6-8 consume (nodes renumbered n - 2 - k: the root is 0).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstdint>

#include "bvh_ploc.h"
#include "common.h"

namespace {

constexpr int PLOC_BLOCK = 256;
constexpr int PLOC_WINDOW = PLOC_BLOCK + 2 * BVH_PLOC_MAX_RADIUS;
constexpr int PLOC_BATCH = 4;                // iterations enqueued per read of the live count
constexpr int PLOC_MAX_CLIMB = 4096;         // bound of every upward walk (bvh_device.hip: BVHD_MAX_CLIMB)

// the pair key (area bits, |i - j|, parity of min(i, j), min(i, j)), compared lexicographically
__device__ __forceinline__ bool pair_less(uint32_t a, int d, int lo, uint32_t best_a, int best_d, int best_lo) {
  if (a != best_a) return a < best_a;
  if (d != best_d) return d < best_d;
  if ((lo & 1) != (best_lo & 1)) return (lo & 1) < (best_lo & 1);
  return lo < best_lo;
}

// "cluster i survives this iteration" (the scan's input): it is not the higher end of a mutual pair
struct PlocSurvivor {
  const int32_t* nn;
  const int32_t* live;
  __device__ uint32_t operator()(int i) const {
    const int m = *live;
    if (m <= 1 || i >= m) return 0u;
    const int j = nn[i];
    return (j < i && nn[j] == i) ? 0u : 1u;
  }
};

}  // namespace

// Clusters: lo = (box lo xyz, reference bits: internal node >= 0, leaf ~sorted position), hi = (box hi xyz, triangle
// count bits).  live[0] = n.
__global__ __launch_bounds__(PLOC_BLOCK) void bvh_ploc_init(const float4* __restrict__ tbox,
                                                            const int32_t* __restrict__ sorted, int n,
                                                            float4* __restrict__ clo, float4* __restrict__ chi,
                                                            int32_t* __restrict__ live) {
  const int i = blockIdx.x * PLOC_BLOCK + threadIdx.x;
  if (i == 0) live[0] = n;
  if (i >= n) return;
  const int f = sorted[i];
  const float4 lo = tbox[2 * (size_t)f], hi = tbox[2 * (size_t)f + 1];
  clo[i] = make_float4(lo.x, lo.y, lo.z, __int_as_float(~i));
  chi[i] = make_float4(hi.x, hi.y, hi.z, __int_as_float(1));
}

// a. nn[i] for every live cluster i < *live
__global__ __launch_bounds__(PLOC_BLOCK) void bvh_ploc_nearest(const float4* __restrict__ clo,
                                                               const float4* __restrict__ chi,
                                                               const int32_t* __restrict__ live, int radius,
                                                               int32_t* __restrict__ nn) {
  const int m = *live;
  const int b0 = blockIdx.x * PLOC_BLOCK;
  if (m <= 1 || b0 >= m) return;
  __shared__ float box[6][PLOC_WINDOW];        // SoA: lo x y z, hi x y z of clusters b0 - radius ..
  const int w0 = b0 - radius;
  for (int t = threadIdx.x; t < PLOC_BLOCK + 2 * radius; t += PLOC_BLOCK) {
    const int g = w0 + t;
    if (g >= 0 && g < m) {
      const float4 lo = clo[g], hi = chi[g];
      box[0][t] = lo.x;
      box[1][t] = lo.y;
      box[2][t] = lo.z;
      box[3][t] = hi.x;
      box[4][t] = hi.y;
      box[5][t] = hi.z;
    }
  }
  __syncthreads();
  const int i = b0 + threadIdx.x;
  if (i >= m) return;
  const int li = threadIdx.x + radius;
  const float lx = box[0][li], ly = box[1][li], lz = box[2][li];
  const float hx = box[3][li], hy = box[4][li], hz = box[5][li];
  uint32_t best_a = 0xffffffffu;
  int best_d = 0x7fffffff, best_lo = 0x7fffffff, best_j = i == 0 ? 1 : i - 1;
  for (int d = 1; d <= radius; ++d) {
    for (int side = 0; side < 2; ++side) {
      const int j = side ? i + d : i - d;
      if (j < 0 || j >= m) continue;
      const int lj = li + (j - i);               // in [threadIdx.x, threadIdx.x + 2 radius]: inside the window
      const float ex = fmaxf(hx, box[3][lj]) - fminf(lx, box[0][lj]);
      const float ey = fmaxf(hy, box[4][lj]) - fminf(ly, box[1][lj]);
      const float ez = fmaxf(hz, box[5][lj]) - fminf(lz, box[2][lj]);
      const uint32_t a = __float_as_uint(ex * ey + ey * ez + ez * ex);   // >= 0: the bits order as the values
      const int lo = min(i, j);
      if (pair_less(a, d, lo, best_a, best_d, best_lo)) {
        best_a = a;
        best_d = d;
        best_lo = lo;
        best_j = j;
      }
    }
  }
  nn[i] = best_j;
}

// c. merge the mutual pairs and move every survivor to its scanned position surv[i]; live_next = the survivors
__global__ __launch_bounds__(PLOC_BLOCK) void bvh_ploc_merge(const float4* __restrict__ clo,
                                                             const float4* __restrict__ chi,
                                                             const int32_t* __restrict__ nn,
                                                             const uint32_t* __restrict__ surv,
                                                             const int32_t* __restrict__ live, int n,
                                                             float4* __restrict__ olo, float4* __restrict__ ohi,
                                                             int32_t* __restrict__ live_next, int2* __restrict__ pchild,
                                                             int32_t* __restrict__ pcount,
                                                             int32_t* __restrict__ pparent) {
  const int m = *live;
  const int i = blockIdx.x * PLOC_BLOCK + threadIdx.x;
  if (m <= 1) {
    if (i == 0) *live_next = m;
    return;
  }
  if (i >= m) return;
  const int j = nn[i];
  const bool mutual = nn[j] == i;
  if (i == m - 1) *live_next = (int)surv[i] + ((mutual && j < i) ? 0 : 1);
  if (mutual && j < i) return;                  // merged into cluster j's node
  float4 lo = clo[i], hi = chi[i];
  if (mutual) {
    const float4 lo2 = clo[j], hi2 = chi[j];
    const int node = (n - m) + (j - (int)surv[j]);   // removals so far + removals before j: in [0, n - 2]
    if (node < 0 || node >= n - 1) return;           // (cannot happen: a bound, not a path)
    const int a = __float_as_int(lo.w), b = __float_as_int(lo2.w);
    const int count = __float_as_int(hi.w) + __float_as_int(hi2.w);
    pchild[node] = make_int2(a, b);
    pcount[node] = count;
    if (a >= 0) pparent[a] = node << 1;
    if (b >= 0) pparent[b] = (node << 1) | 1;
    lo = make_float4(fminf(lo.x, lo2.x), fminf(lo.y, lo2.y), fminf(lo.z, lo2.z), __int_as_float(node));
    hi = make_float4(fmaxf(hi.x, hi2.x), fmaxf(hi.y, hi2.y), fmaxf(hi.z, hi2.z), __int_as_float(count));
  }
  olo[surv[i]] = lo;
  ohi[surv[i]] = hi;
}

// The tree in bvh_device.hip's form.  Node k (merge order) becomes n - 2 - k; its first leaf position is the sum of
// the left siblings' triangle counts on its way up; its left child starts there, its right child after the left's
// count; a leaf child at position p takes the face of its sorted position.
__global__ __launch_bounds__(PLOC_BLOCK) void bvh_ploc_layout(int n, const int2* __restrict__ pchild,
                                                              const int32_t* __restrict__ pcount,
                                                              const int32_t* __restrict__ pparent,
                                                              const int32_t* __restrict__ sorted,
                                                              int32_t* __restrict__ order, int2* __restrict__ child,
                                                              int2* __restrict__ range, int32_t* __restrict__ parent_int,
                                                              int32_t* __restrict__ parent_leaf, int32_t* err,
                                                              int err_walk) {
  const int k = blockIdx.x * PLOC_BLOCK + threadIdx.x;
  const int ni = n - 1;
  if (k >= ni) return;
  int first = 0;
  for (int cur = k, step = 0; cur != ni - 1; ++step) {
    const int pr = pparent[cur];
    if (step >= PLOC_MAX_CLIMB || pr < 0 || (pr >> 1) >= ni) {
      atomicOr(err, err_walk);
      return;
    }
    const int par = pr >> 1;
    if (pr & 1) {
      const int l = pchild[par].x;
      if (l >= ni) {
        atomicOr(err, err_walk);
        return;
      }
      first += l < 0 ? 1 : pcount[l];
    }
    cur = par;
  }
  const int self = ni - 1 - k;
  const int2 ch = pchild[k];
  const int count = pcount[k];
  const bool ok = ch.x >= -n && ch.x < ni && ch.y >= -n && ch.y < ni;
  const int left_count = !ok ? 0 : ch.x < 0 ? 1 : pcount[ch.x];
  if (!ok || first < 0 || left_count < 1 || left_count >= count || first + count > n) {
    atomicOr(err, err_walk);
    return;
  }
  range[self] = make_int2(first, first + count - 1);
  if (self == 0) parent_int[0] = -1;
  int out[2];
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int c = side ? ch.y : ch.x;
    const int link = (self << 1) | side;
    if (c < 0) {
      const int p = side ? first + left_count : first;
      order[p] = sorted[~c];
      parent_leaf[p] = link;
      out[side] = ~p;
    } else {
      parent_int[ni - 1 - c] = link;
      out[side] = ni - 1 - c;
    }
  }
  child[self] = make_int2(out[0], out[1]);
}

namespace {

size_t aligned(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

int bvh_ploc_topology(const float4* tbox, const int32_t* sorted, int n, int radius, hipStream_t stream, int32_t* order,
                      int2* child, int2* range, int32_t* parent_int, int32_t* parent_leaf, int32_t* err,
                      int err_walk) {
  if (n < 2 || radius < 1 || radius > BVH_PLOC_MAX_RADIUS) return VSA_ERR_ARG;
  const int ni = n - 1;
  auto survivors = [](const int32_t* nn, const int32_t* live) {
    return rocprim::make_transform_iterator(rocprim::make_counting_iterator<int>(0), PlocSurvivor{nn, live});
  };
  size_t scan_bytes = 0;
  VSA_HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, survivors(nullptr, nullptr), (uint32_t*)nullptr, 0u,
                                      (size_t)n, rocprim::plus<uint32_t>(), stream));
  // one scratch allocation: two cluster arrays (lo, hi), nn, scan output, the merge-order nodes, live[2], scan temp
  const size_t sz_box = aligned(sizeof(float4) * (size_t)n), sz_int = aligned(sizeof(int32_t) * (size_t)n);
  const size_t total = 4 * sz_box + 2 * sz_int + aligned(sizeof(int2) * (size_t)ni) + 2 * sz_int + aligned(64) +
                       aligned(scan_bytes ? scan_bytes : 16);
  char* base = nullptr;
  VSA_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&base), total));
  char* p = base;
  auto carve = [&p](size_t bytes) {
    char* q = p;
    p += bytes;
    return q;
  };
  float4* clo[2] = {reinterpret_cast<float4*>(carve(sz_box)), reinterpret_cast<float4*>(carve(sz_box))};
  float4* chi[2] = {reinterpret_cast<float4*>(carve(sz_box)), reinterpret_cast<float4*>(carve(sz_box))};
  int32_t* nn = reinterpret_cast<int32_t*>(carve(sz_int));
  uint32_t* surv = reinterpret_cast<uint32_t*>(carve(sz_int));
  int2* pchild = reinterpret_cast<int2*>(carve(aligned(sizeof(int2) * (size_t)ni)));
  int32_t* pcount = reinterpret_cast<int32_t*>(carve(sz_int));
  int32_t* pparent = reinterpret_cast<int32_t*>(carve(sz_int));
  int32_t* live = reinterpret_cast<int32_t*>(carve(aligned(64)));
  void* scan_tmp = carve(aligned(scan_bytes ? scan_bytes : 16));

  hipError_t e = hipMemsetAsync(pparent, 0xff, sizeof(int32_t) * (size_t)ni, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(bvh_ploc_init, dim3(vsa_div_up(n, PLOC_BLOCK)), dim3(PLOC_BLOCK), 0, stream, tbox, sorted, n,
                       clo[0], chi[0], live);
    e = hipGetLastError();
  }
  int rc = e == hipSuccess ? VSA_OK : (int)e;
  int m = n, cur = 0, iters = 0;
  while (rc == VSA_OK && m > 1) {
    // every iteration with >= 2 clusters merges at least one pair: n - 1 iterations always suffice
    const int batch = std::min(PLOC_BATCH, ni - iters);
    if (batch <= 0) {
      rc = VSA_ERR_UNSUPPORTED;
      break;
    }
    const int grid = vsa_div_up(m, PLOC_BLOCK);  // the count only falls: this grid covers the whole batch
    for (int b = 0; b < batch && e == hipSuccess; ++b, ++iters, cur ^= 1) {
      hipLaunchKernelGGL(bvh_ploc_nearest, dim3(grid), dim3(PLOC_BLOCK), 0, stream, clo[cur], chi[cur], live + cur,
                         radius, nn);
      e = hipGetLastError();
      if (e == hipSuccess)
        e = rocprim::exclusive_scan(scan_tmp, scan_bytes, survivors(nn, live + cur), surv, 0u, (size_t)m,
                                    rocprim::plus<uint32_t>(), stream);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(bvh_ploc_merge, dim3(grid), dim3(PLOC_BLOCK), 0, stream, clo[cur], chi[cur], nn, surv,
                           live + cur, n, clo[cur ^ 1], chi[cur ^ 1], live + (cur ^ 1), pchild, pcount, pparent);
        e = hipGetLastError();
      }
    }
    int next = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&next, live + cur, sizeof(int), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    rc = e == hipSuccess ? VSA_OK : (int)e;
    if (rc == VSA_OK && (next < 1 || next >= m)) rc = VSA_ERR_UNSUPPORTED;   // no progress: never spin on it
    m = next;
  }
  if (rc == VSA_OK) {
    hipLaunchKernelGGL(bvh_ploc_layout, dim3(vsa_div_up(ni, PLOC_BLOCK)), dim3(PLOC_BLOCK), 0, stream, n, pchild,
                       pcount, pparent, sorted, order, child, range, parent_int, parent_leaf, err, err_walk);
    e = hipGetLastError();
    rc = e == hipSuccess ? VSA_OK : (int)e;
  }
  (void)hipStreamSynchronize(stream);
  (void)hipFree(base);
  return rc;
}
