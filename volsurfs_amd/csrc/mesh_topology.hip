// The mesh stages' shared device work (declared in mesh_topology.h): the edge-key, (vertex, face), iota and root-walk
// kernels, the two host sequences built on them, and every rocPRIM sort and scan of csrc/simplify.hip, csrc/atlas.hip
// and csrc/mesh_clean.hip, so that rocPRIM is instantiated in this unit only.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cstdint>

#include "mesh_topology.h"

// ------------------------------------------------------------------------------------------------ kernels

__global__ __launch_bounds__(MT_BLOCK) void mt_edge_keys(const int32_t* __restrict__ faces, long long n3, int s,
                                                        mt::u64* __restrict__ keys, uint32_t* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= n3) return;
  const long long f = i / 3;
  const int c = (int)(i - 3 * f);
  keys[i] = fu_edge_key(faces[3 * f + c], faces[3 * f + (c == 2 ? 0 : c + 1)], s);
  if (vals) vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(MT_BLOCK) void mt_vf_pairs(const int32_t* __restrict__ faces, long long n3,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= n3) return;
  keys[i] = (uint32_t)faces[i];
  vals[i] = (uint32_t)(i / 3);
}

__global__ __launch_bounds__(MT_BLOCK) void mt_vf_ranges(const uint32_t* __restrict__ k, long long n3,
                                                        int32_t* __restrict__ vstart, int32_t* __restrict__ vend) {
  const long long i = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (i >= n3) return;
  if (i == 0 || k[i] != k[i - 1]) vstart[k[i]] = (int32_t)i;
  if (i == n3 - 1 || k[i] != k[i + 1]) vend[k[i]] = (int32_t)(i + 1);
}

__global__ __launch_bounds__(MT_BLOCK) void mt_iota(int32_t* __restrict__ par, long long F) {
  const long long f = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (f < F) par[f] = (int32_t)f;
}

__global__ __launch_bounds__(MT_BLOCK) void mt_roots(const int32_t* __restrict__ par, long long F,
                                                    int32_t* __restrict__ root, int32_t* __restrict__ flags) {
  const long long f = (long long)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (f >= F) return;
  const int r = fu_root(par, (int)f);
  root[f] = r;
  flags[f] = r == f;
}

// ------------------------------------------------------------------------------------------------ host

namespace mt {

int tmp_bytes(const TmpCounts& n, size_t* out) {
  const hipStream_t st = 0;
  const uint32_t* k32 = nullptr;
  const u64* k64 = nullptr;
  const int32_t* i32 = nullptr;
  const long long* i64 = nullptr;
  size_t t = 0, need = 16;
  if (n.pairs64) {
    VSA_HIP_TRY(rocprim::radix_sort_pairs(nullptr, t, k64, (u64*)nullptr, k32, (uint32_t*)nullptr, n.pairs64, 0, 64, st));
    need = t > need ? t : need;
  }
  if (n.pairs32) {
    VSA_HIP_TRY(rocprim::radix_sort_pairs(nullptr, t, k32, (uint32_t*)nullptr, k32, (uint32_t*)nullptr, n.pairs32, 0, 32,
                                          st));
    need = t > need ? t : need;
  }
  if (n.keys64) {
    VSA_HIP_TRY(rocprim::radix_sort_keys(nullptr, t, k64, (u64*)nullptr, n.keys64, 0, 64, st));
    need = t > need ? t : need;
  }
  if (n.keys_desc32) {
    VSA_HIP_TRY(rocprim::radix_sort_keys_desc(nullptr, t, i32, (int32_t*)nullptr, n.keys_desc32, 0, 32, st));
    need = t > need ? t : need;
  }
  if (n.xscan32) {
    VSA_HIP_TRY(rocprim::exclusive_scan(nullptr, t, i32, (int32_t*)nullptr, 0, n.xscan32, rocprim::plus<int32_t>(), st));
    need = t > need ? t : need;
  }
  if (n.iscan64) {
    VSA_HIP_TRY(rocprim::inclusive_scan(nullptr, t, i64, (long long*)nullptr, n.iscan64, rocprim::plus<long long>(), st));
    need = t > need ? t : need;
  }
  *out = need;
  return VSA_OK;
}

int sort_pairs(Tmp tmp, const u64* kin, u64* kout, const uint32_t* vin, uint32_t* vout, size_t n, int begin_bit,
               int end_bit, hipStream_t st) {
  VSA_HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tmp.bytes, kin, kout, vin, vout, n, begin_bit, end_bit, st));
  return VSA_OK;
}

int sort_pairs(Tmp tmp, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout, size_t n,
               int begin_bit, int end_bit, hipStream_t st) {
  VSA_HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tmp.bytes, kin, kout, vin, vout, n, begin_bit, end_bit, st));
  return VSA_OK;
}

int sort_keys(Tmp tmp, const u64* kin, u64* kout, size_t n, int begin_bit, int end_bit, hipStream_t st) {
  VSA_HIP_TRY(rocprim::radix_sort_keys(tmp.p, tmp.bytes, kin, kout, n, begin_bit, end_bit, st));
  return VSA_OK;
}

int sort_keys_desc(Tmp tmp, const int32_t* kin, int32_t* kout, size_t n, int begin_bit, int end_bit, hipStream_t st) {
  VSA_HIP_TRY(rocprim::radix_sort_keys_desc(tmp.p, tmp.bytes, kin, kout, n, begin_bit, end_bit, st));
  return VSA_OK;
}

int exclusive_scan(Tmp tmp, const int32_t* in, int32_t* out, size_t n, hipStream_t st) {
  VSA_HIP_TRY(rocprim::exclusive_scan(tmp.p, tmp.bytes, in, out, 0, n, rocprim::plus<int32_t>(), st));
  return VSA_OK;
}

int inclusive_scan(Tmp tmp, const long long* in, long long* out, size_t n, hipStream_t st) {
  VSA_HIP_TRY(rocprim::inclusive_scan(tmp.p, tmp.bytes, in, out, n, rocprim::plus<long long>(), st));
  return VSA_OK;
}

int edge_keys(const int32_t* faces, long long F, int s, u64* keys, uint32_t* vals, hipStream_t st) {
  hipLaunchKernelGGL(mt_edge_keys, grid(3 * F), dim3(MT_BLOCK), 0, st, faces, 3 * F, s, keys, vals);
  MT_LAUNCHED();
  return VSA_OK;
}

int sorted_edges(const int32_t* faces, long long F, int s, u64* keys, u64* sorted, uint32_t* vals, uint32_t* slot,
                 Tmp tmp, hipStream_t st) {
  MT_TRY(edge_keys(faces, F, s, keys, vals, st));
  if (vals) return sort_pairs(tmp, keys, sorted, vals, slot, 3 * (size_t)F, 0, 2 * s, st);
  return sort_keys(tmp, keys, sorted, 3 * (size_t)F, 0, 2 * s, st);
}

int vertex_rings(const int32_t* faces, long long F, long long V, int s, uint32_t* kin, uint32_t* kout, uint32_t* vin,
                 uint32_t* vff, int32_t* vstart, int32_t* vend, Tmp tmp, hipStream_t st) {
  const long long n3 = 3 * F;
  hipLaunchKernelGGL(mt_vf_pairs, grid(n3), dim3(MT_BLOCK), 0, st, faces, n3, kin, vin);
  MT_LAUNCHED();
  MT_TRY(sort_pairs(tmp, kin, kout, vin, vff, (size_t)n3, 0, s, st));
  VSA_HIP_TRY(hipMemsetAsync(vstart, 0, 4 * (size_t)V, st));
  VSA_HIP_TRY(hipMemsetAsync(vend, 0, 4 * (size_t)V, st));
  hipLaunchKernelGGL(mt_vf_ranges, grid(n3), dim3(MT_BLOCK), 0, st, kout, n3, vstart, vend);
  MT_LAUNCHED();
  return VSA_OK;
}

int iota(int32_t* par, long long F, hipStream_t st) {
  hipLaunchKernelGGL(mt_iota, grid(F), dim3(MT_BLOCK), 0, st, par, F);
  MT_LAUNCHED();
  return VSA_OK;
}

int roots(const int32_t* par, long long F, int32_t* root, int32_t* flags, hipStream_t st) {
  hipLaunchKernelGGL(mt_roots, grid(F), dim3(MT_BLOCK), 0, st, par, F, root, flags);
  MT_LAUNCHED();
  return VSA_OK;
}

}  // namespace mt
