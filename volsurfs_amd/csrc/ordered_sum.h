// The fixed-order fp64 sum of per-wave partials, stated once (mesh_distance.hip's report, texture_transfer.hip's): the
// waves' records of N doubles added in wave order, in a shape fixed by the number of waves alone.  Lane t of the block's
// ORDERED_SUM_BLOCK adds the consecutive waves [t c, (t + 1) c), c = ceil(waves / ORDERED_SUM_BLOCK), one after the
// other; lane 0 then adds the ORDERED_SUM_BLOCK run sums in lane order.  The order of the additions is the rule: the same
// partials give the same bits.  (One lane adding every record in turn is a chain of 15 625 dependent loads and adds for
// 10^6 samples: it took as long as the walk.)
#pragma once
#include <hip/hip_runtime.h>

constexpr int ORDERED_SUM_BLOCK = 1024;

// Every lane of a block of ORDERED_SUM_BLOCK calls it, once; `total` is the sum in lane 0 (the return value says so) and
// is not meaningful in the others.  partials: nr_waves records, aligned to their 8 N bytes.  UNROLL and the width of
// the count shape the run loop's code, not its order: each kernel keeps the loop it had before the text was shared (the
// pairs' loop unrolled by 4, the one-component loop as it stands, its count an int).
template <int N, int UNROLL, typename Count>
__device__ __forceinline__ bool ordered_sum(const double* __restrict__ partials, Count nr_waves, double (&total)[N]) {
  typedef double Rec __attribute__((ext_vector_type(N)));
  __shared__ double s_run[N][ORDERED_SUM_BLOCK];
  const int t = threadIdx.x;
  const Count c = (nr_waves + ORDERED_SUM_BLOCK - 1) / ORDERED_SUM_BLOCK;
  const long long begin = (long long)t * c, end = begin + c < nr_waves ? begin + c : nr_waves;
  double s[N];
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = 0.0;
#pragma unroll UNROLL
  for (long long w = begin; w < end; ++w) {
    const Rec p = reinterpret_cast<const Rec*>(partials)[w];
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += p[k];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) s_run[k][t] = s[k], total[k] = 0.0;
  __syncthreads();
  if (t != 0) return false;
  for (int l = 0; l < ORDERED_SUM_BLOCK; ++l) {
#pragma unroll
    for (int k = 0; k < N; ++k) total[k] += s_run[k][l];
  }
  return true;
}
