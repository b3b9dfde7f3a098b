// What the mesh stages share (csrc/simplify.hip, csrc/atlas.hip, csrc/mesh_clean.hip), written once: the (min, max)
// edge key and the union-find over faces, the host scaffolding of a stage (workspace layout, stage timer, counter
// read-back, status mapping), and the declarations of csrc/mesh_topology.hip, which holds the shared kernels and every
// rocPRIM sort and scan of the three stages.  Internal: nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

#define MT_BLOCK 256

#define MT_TRY(expr)               \
  do {                             \
    const int r__ = (expr);        \
    if (r__ != VSA_OK) return r__; \
  } while (0)

#define MT_LAUNCHED() VSA_HIP_TRY(hipGetLastError())

// ------------------------------------------------------------------------------------------------ device

// The undirected edge (x, y) as min << s | max, s = the bits of V - 1.
__device__ __forceinline__ unsigned long long fu_edge_key(int x, int y, int s) {
  const int lo = x < y ? x : y, hi = x < y ? y : x;
  return (unsigned long long)(unsigned)lo << s | (unsigned long long)(unsigned)hi;
}

__device__ __forceinline__ int fu_find(int* par, int x) {
  while (true) {
    const int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    const int g = __hip_atomic_load(par + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g != p) __hip_atomic_store(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // halving: an ancestor
    x = p;
  }
}

// Joins the components of a and b: the larger root is hooked under the smaller by a CAS, so every parent is <= its
// child and the root of a component is its minimum face index whatever the order of the hooks.
__device__ __forceinline__ void fu_union(int* par, int a, int b) {
  while (true) {
    a = fu_find(par, a);
    b = fu_find(par, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(par + b, b, a) == b) return;
  }
}

// Root of x by a walk that only reads: `par` is left as the hooks built it while other lanes walk it, so every lane
// sees the same final forest and finds the same root.
__device__ __forceinline__ int fu_root(const int32_t* __restrict__ par, int x) {
  int p = par[x];
  while (p != x) {
    x = p;
    p = par[x];
  }
  return x;
}

// ------------------------------------------------------------------------------------------------ host

namespace mt {

typedef unsigned long long u64;

inline size_t align(size_t x) { return (x + 255) & ~(size_t)255; }

// Workspace layout: take(bytes) returns the offset of the next buffer; `o` is the total so far.
struct Bump {
  size_t o = 0;
  size_t take(size_t bytes) {
    const size_t at = o;
    o += align(bytes);
    return at;
  }
};

template <typename T>
T* at(char* ws, size_t o) {
  return reinterpret_cast<T*>(ws + o);
}

inline dim3 grid(long long n) { return dim3((unsigned)vsa_div_up(n > 0 ? n : 1, MT_BLOCK)); }

inline int bits_of(long long n) {   // the bits of n - 1, at least 1
  int s = 1;
  while ((1ll << s) < n) ++s;
  return s;
}

// The (V, F) a mesh stage takes: 3 F + 3 fits an int32.
inline int check_vf(long long V, long long F) {
  if (V < 1 || F < 1) return VSA_ERR_ARG;
  if (V > 0x7FFFFFFFll || F > 0x7FFFFFFFll / 3 - 1) return VSA_ERR_UNSUPPORTED;
  return VSA_OK;
}

// The status of a layout query as a C-ABI return value: a positive one is the HIP status of a rocPRIM size query.
inline int abi_status(int rc) { return rc > 0 ? VSA_ERR_UNSUPPORTED : rc; }

// dst[0 .. n) = the device counters src[0 .. n); blocks until the stream has drained.
inline int read_counters(hipStream_t st, const long long* src, long long* dst, int n = 1) {
  VSA_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(long long), hipMemcpyDeviceToHost, st));
  VSA_HIP_TRY(hipStreamSynchronize(st));
  return VSA_OK;
}

// Stage timing, only when the caller passes `stage_ms`: open() opens a stage, close(k) adds its device time to
// stage_ms[k].
struct StageTimer {
  hipStream_t st;
  float* ms;
  hipEvent_t ev[2];

  int create(float* stage_ms, int stages, hipStream_t stream) {
    st = stream;
    ms = stage_ms;
    if (!ms) return VSA_OK;
    for (int k = 0; k < stages; ++k) ms[k] = 0.f;
    VSA_HIP_TRY(hipEventCreate(&ev[0]));
    VSA_HIP_TRY(hipEventCreate(&ev[1]));
    return VSA_OK;
  }
  void destroy() {
    if (!ms) return;
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
  }
  int open() {
    if (ms) VSA_HIP_TRY(hipEventRecord(ev[0], st));
    return VSA_OK;
  }
  int close(int k) {
    if (!ms) return VSA_OK;
    float t = 0.f;
    VSA_HIP_TRY(hipEventRecord(ev[1], st));
    VSA_HIP_TRY(hipEventSynchronize(ev[1]));
    VSA_HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
    ms[k] += t;
    return VSA_OK;
  }
};

// ---- csrc/mesh_topology.hip

// rocPRIM's temporary storage, owned by the caller's workspace.
struct Tmp {
  void* p;
  size_t bytes;
};

// Element counts of the largest call of each kind a stage makes (0: it makes none).
struct TmpCounts {
  size_t pairs64, pairs32, keys64, keys_desc32, xscan32, iscan64;
};

// *out = the largest temporary storage any of those calls asks for, at least 16 bytes.
int tmp_bytes(const TmpCounts& n, size_t* out);

// Radix sorts over bits [begin_bit, end_bit) and scans from 0, all stable and in the caller's stream.
int sort_pairs(Tmp tmp, const u64* kin, u64* kout, const uint32_t* vin, uint32_t* vout, size_t n, int begin_bit,
               int end_bit, hipStream_t st);
int sort_pairs(Tmp tmp, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout, size_t n,
               int begin_bit, int end_bit, hipStream_t st);
int sort_keys(Tmp tmp, const u64* kin, u64* kout, size_t n, int begin_bit, int end_bit, hipStream_t st);
int sort_keys_desc(Tmp tmp, const int32_t* kin, int32_t* kout, size_t n, int begin_bit, int end_bit, hipStream_t st);
int exclusive_scan(Tmp tmp, const int32_t* in, int32_t* out, size_t n, hipStream_t st);
int inclusive_scan(Tmp tmp, const long long* in, long long* out, size_t n, hipStream_t st);

// keys[i] = the edge key of face slot i = 3 f + c (corner c to the next) at s bits per vertex; vals[i] = i unless null.
int edge_keys(const int32_t* faces, long long F, int s, u64* keys, uint32_t* vals, hipStream_t st);

// edge_keys, then the sort of their 2 s bits: `sorted`, and with `vals` the slot of every sorted key in `slot`.
int sorted_edges(const int32_t* faces, long long F, int s, u64* keys, u64* sorted, uint32_t* vals, uint32_t* slot,
                 Tmp tmp, hipStream_t st);

// The (vertex, face) list sorted by vertex (stable: ascending face within a vertex): the faces in `vff`, the sorted
// vertices in `kout`, and the ring of vertex v at vff[vstart[v] .. vend[v]) (both 0 for a vertex no face names).
int vertex_rings(const int32_t* faces, long long F, long long V, int s, uint32_t* kin, uint32_t* kout, uint32_t* vin,
                 uint32_t* vff, int32_t* vstart, int32_t* vend, Tmp tmp, hipStream_t st);

// par[f] = f.
int iota(int32_t* par, long long F, hipStream_t st);

// root[f] = the root of f by the read-only walk (a separate array: no lane writes to a node another lane walks);
// flags[f] = f is a root.
int roots(const int32_t* par, long long F, int32_t* root, int32_t* flags, hipStream_t st);

}  // namespace mt
