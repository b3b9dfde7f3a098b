// Faces joined across shared edges: the (min, max) edge key and the union-find whose root is a component's minimum
// face index, written once for csrc/atlas.hip (charts) and csrc/mesh_clean.hip (triangle clusters).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
