// Marching cubes of K level sets of one fp32 grid (vsa_isosurface_*; rules in include/volsurfs_hip.h).
//
// Layout.  A "row" is the line of nz grid points (i, j, 0..nz-1) along the contiguous z axis; row r = i * ny + j.
// Row r owns the vertices of the crossed edges that start at its points (x, y, z edges), and the faces of the cells
// (i, j, k) whose lowest corner lies on it.  One workgroup of 256 lanes walks one row in chunks of 256 points, one
// point (and the cell above it) per lane, with the grid values of the rows it needs staged in LDS once per chunk and
// every level handled from there (the grid is read once per pass, not once per level).
//
//   count:  per row and level, the vertices its points own and the faces its cells emit -> counts [2][K][R] i32
//           (a block reduction, no atomics); a device scan (rocPRIM) turns them into offsets [2][K][R] i64 over
//           the whole array, and a one-wave kernel forms the per-level totals.
//   emit:   a cell's 12 edge ids come from the four point-rows around it, (i, j), (i+1, j), (i, j+1), (i+1, j+1);
//           a point's crossing mask needs its +x and +y neighbours too, so eight rows are staged.  The ids are the
//           row's scanned offset + a running carry over earlier chunks + the lane's exclusive prefix in the chunk
//           (one block scan of five 12-bit fields packed in 64 bits: four rows' vertex counts and the row's face
//           count) + the edge's rank among its point's crossed axes.
//
// Every output position is a function of the grid and the levels: no atomics, so the bits repeat.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <cstdint>

#include "common.h"
#include "mc_table.h"

#define ISO_BLOCK 256
#define ISO_WAVES (ISO_BLOCK / VSA_WAVE)
#define ISO_ROWS 8
#define ISO_MAX_LEVELS 16

__constant__ int8_t c_mc_tris[256][16] = VSA_MC_TRIS_INIT;
__constant__ uint8_t c_mc_ntri[256] = VSA_MC_NTRI_INIT;
static const int8_t h_mc_tris[256][16] = VSA_MC_TRIS_INIT;

struct IsoArgs {
  const float* grid;
  long long nx, ny, nz, R;   // R = nx * ny rows
  int K, inside_above;
  float level[ISO_MAX_LEVELS];
  float origin[3], spacing[3];
  int32_t* counts;           // [2][K][R]: vertices, then faces
  long long* offsets;        // [2][K][R] exclusive scan of counts over the whole array
  long long* totals;         // [2K] device: V_0, F_0, V_1, F_1, ...
  float* verts[ISO_MAX_LEVELS];
  int32_t* faces[ISO_MAX_LEVELS];
  long long vcap[ISO_MAX_LEVELS], fcap[ISO_MAX_LEVELS];
};

__device__ __forceinline__ bool iso_inside(float v, float lev, int above) { return above ? v > lev : v < lev; }

// Staged rows: 0 (i, j), 1 (i+1, j), 2 (i, j+1), 3 (i+1, j+1), 4 (i+2, j), 5 (i+2, j+1), 6 (i, j+2), 7 (i+1, j+2).
// Row m < 4 sits at (i + (m & 1), j + (m >> 1)); its +x neighbour is row XN[m], its +y neighbour YN[m].
__device__ __forceinline__ int iso_xn(int m) { return m == 0 ? 1 : m == 1 ? 4 : m == 2 ? 3 : 5; }
__device__ __forceinline__ int iso_yn(int m) { return m == 0 ? 2 : m == 1 ? 3 : m == 2 ? 6 : 7; }

// Stage `nrows` rows around (i, j) for points k0 .. k0 + ISO_BLOCK (one past the chunk: the +z neighbour).  Rows or
// points outside the grid are not read (their entries are never used).
__device__ __forceinline__ void iso_stage(const IsoArgs& a, long long i, long long j, long long k0, int nrows,
                                          float (*s)[ISO_BLOCK + 1]) {
  const int t = threadIdx.x;
  for (int m = 0; m < nrows; ++m) {
    long long di, dj;
    if (m < 4) { di = m & 1; dj = m >> 1; }
    else if (m < 6) { di = 2; dj = m - 4; }
    else { di = m - 6; dj = 2; }
    const long long ii = i + di, jj = j + dj;
    if (ii >= a.nx || jj >= a.ny) continue;
    const float* row = a.grid + (ii * a.ny + jj) * a.nz;
    const long long k = k0 + t;
    if (k < a.nz) s[m][t] = row[k];
    if (t == 0 && k0 + ISO_BLOCK < a.nz) s[m][ISO_BLOCK] = row[k0 + ISO_BLOCK];
  }
}

// Crossing mask (bit a: the edge along axis a that starts at this point is crossed) of staged row m < 4 at lane t.
__device__ __forceinline__ int iso_mask(const IsoArgs& a, float (*s)[ISO_BLOCK + 1], int m, int t, long long i,
                                        long long j, long long k, float lev) {
  const long long ii = i + (m & 1), jj = j + (m >> 1);
  if (ii >= a.nx || jj >= a.ny || k >= a.nz) return 0;
  const bool in0 = iso_inside(s[m][t], lev, a.inside_above);
  int mask = 0;
  if (ii + 1 < a.nx && in0 != iso_inside(s[iso_xn(m)][t], lev, a.inside_above)) mask |= 1;
  if (jj + 1 < a.ny && in0 != iso_inside(s[iso_yn(m)][t], lev, a.inside_above)) mask |= 2;
  if (k + 1 < a.nz && in0 != iso_inside(s[m][t + 1], lev, a.inside_above)) mask |= 4;
  return mask;
}

// Marching-cubes case of cell (i, j, k) (valid cell assumed): bit c = corner (c & 1, c >> 1 & 1, c >> 2) inside.
__device__ __forceinline__ int iso_case(const IsoArgs& a, float (*s)[ISO_BLOCK + 1], int t, float lev) {
  int c = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) c |= (int)iso_inside(s[q & 3][t + (q >> 2)], lev, a.inside_above) << q;
  return c;
}

__global__ __launch_bounds__(ISO_BLOCK) void iso_count_kernel(IsoArgs a) {
  __shared__ float s[4][ISO_BLOCK + 1];
  __shared__ int red[ISO_WAVES][2 * ISO_MAX_LEVELS];
  const long long r = blockIdx.x;
  const long long i = r / a.ny, j = r - i * a.ny;
  const int t = threadIdx.x;
  const bool row_has_cells = i + 1 < a.nx && j + 1 < a.ny;
  int nv[ISO_MAX_LEVELS], nf[ISO_MAX_LEVELS];
#pragma unroll
  for (int L = 0; L < ISO_MAX_LEVELS; ++L) nv[L] = nf[L] = 0;
  for (long long k0 = 0; k0 < a.nz; k0 += ISO_BLOCK) {
    __syncthreads();
    iso_stage(a, i, j, k0, 4, s);
    __syncthreads();
    const long long k = k0 + t;
    const bool cell = row_has_cells && k + 1 < a.nz;
#pragma unroll
    for (int L = 0; L < ISO_MAX_LEVELS; ++L) {
      if (L < a.K) {
        const float lev = a.level[L];
        nv[L] += __popc(iso_mask(a, s, 0, t, i, j, k, lev));
        if (cell) nf[L] += c_mc_ntri[iso_case(a, s, t, lev)];
      }
    }
  }
  const int lane = t & (VSA_WAVE - 1), w = t / VSA_WAVE;
#pragma unroll
  for (int L = 0; L < ISO_MAX_LEVELS; ++L) {
    int v = nv[L], f = nf[L];
    for (int o = VSA_WAVE / 2; o > 0; o >>= 1) {
      v += __shfl_xor(v, o);
      f += __shfl_xor(f, o);
    }
    if (lane == 0) {
      red[w][2 * L] = v;
      red[w][2 * L + 1] = f;
    }
  }
  __syncthreads();
  if (t < 2 * a.K) {
    int sum = 0;
    for (int q = 0; q < ISO_WAVES; ++q) sum += red[q][t];
    const int L = t >> 1, kind = t & 1;
    a.counts[((long long)kind * a.K + L) * a.R + r] = sum;
  }
}

__global__ void iso_totals_kernel(IsoArgs a) {
  const int t = threadIdx.x;
  if (t >= 2 * a.K) return;
  const int L = t >> 1, kind = t & 1;
  const long long first = ((long long)kind * a.K + L) * a.R, last = first + a.R - 1;
  a.totals[t] = a.offsets[last] + a.counts[last] - a.offsets[first];
}

#define ISO_FIELD(x, f) ((int)(((x) >> (12 * (f))) & 0xFFF))

__global__ __launch_bounds__(ISO_BLOCK) void iso_emit_kernel(IsoArgs a) {
  __shared__ float s[ISO_ROWS][ISO_BLOCK + 1];
  __shared__ unsigned long long wsum[ISO_MAX_LEVELS][ISO_WAVES];
  __shared__ long long base[ISO_MAX_LEVELS][5];   // rows 0..3: first vertex id of the chunk; 4: first face id
  const long long r = blockIdx.x;
  const long long i = r / a.ny, j = r - i * a.ny;
  const int t = threadIdx.x, lane = t & (VSA_WAVE - 1), w = t / VSA_WAVE;
  const bool row_has_cells = i + 1 < a.nx && j + 1 < a.ny;
  if (t < 5 * a.K) {
    const int L = t / 5, m = t - 5 * L;
    long long v = 0;
    if (m < 4) {
      const long long ii = i + (m & 1), jj = j + (m >> 1);
      if (ii < a.nx && jj < a.ny) {
        const long long lvl = (long long)L * a.R;
        v = a.offsets[lvl + ii * a.ny + jj] - a.offsets[lvl];
      }
    } else {
      const long long lvl = ((long long)a.K + L) * a.R;
      v = a.offsets[lvl + r] - a.offsets[lvl];
    }
    base[L][m] = v;
  }
  for (long long k0 = 0; k0 < a.nz; k0 += ISO_BLOCK) {
    __syncthreads();
    iso_stage(a, i, j, k0, ISO_ROWS, s);
    __syncthreads();
    const long long k = k0 + t;
    const bool cell = row_has_cells && k + 1 < a.nz;
#pragma unroll 1
    for (int L = 0; L < a.K; ++L) {
      const float lev = a.level[L];
      int mask[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) mask[m] = iso_mask(a, s, m, t, i, j, k, lev);
      const int cs = cell ? iso_case(a, s, t, lev) : 0;
      const int nt = cell ? c_mc_ntri[cs] : 0;
      unsigned long long packed = (unsigned long long)nt << 48;
#pragma unroll
      for (int m = 0; m < 4; ++m) packed |= (unsigned long long)__popc(mask[m]) << (12 * m);
      // block exclusive scan of the packed fields (no field exceeds 5 * 256 < 4096)
      unsigned long long inc = packed;
#pragma unroll
      for (int o = 1; o < VSA_WAVE; o <<= 1) {
        const unsigned long long y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
      }
      if (lane == VSA_WAVE - 1) wsum[L][w] = inc;
      __syncthreads();
      unsigned long long pre = inc - packed;
      for (int q = 0; q < w; ++q) pre += wsum[L][q];
      // vertices of row 0
      const float* fa_row = s[0];
      if (mask[0]) {
        long long id = base[L][0] + ISO_FIELD(pre, 0);
        const float fa = fa_row[t];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          if (!(mask[0] >> ax & 1)) continue;
          const float fb = ax == 0 ? s[1][t] : ax == 1 ? s[2][t] : s[0][t + 1];
          // IEEE division; the library builds with -ffp-contract=off, so nothing below fuses
          const float tt = (lev - fa) / (fb - fa);
          const long long idx[3] = {i, j, k};
          if (id < a.vcap[L]) {
            float* v = a.verts[L] + 3 * id;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float fi = (float)idx[c];
              v[c] = c == ax ? a.origin[c] + (fi + tt) * a.spacing[c] : a.origin[c] + fi * a.spacing[c];
            }
          }
          ++id;
        }
      }
      if (nt) {
        // edge e = 4 * axis + q is owned by row m at point k + dz
        int bx1[4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
          bx1[m] = i + (m & 1) + 1 < a.nx &&
                   iso_inside(s[m][t + 1], lev, a.inside_above) != iso_inside(s[iso_xn(m)][t + 1], lev, a.inside_above);
        long long fid = base[L][4] + ISO_FIELD(pre, 4);
        for (int q = 0; q < nt; ++q, ++fid) {
          int id3[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int e = c_mc_tris[cs][3 * q + c];
            const int ax = e >> 2, qq = e & 3;
            const int m = ax == 0 ? (qq & 1) << 1 : ax == 1 ? (qq & 1) : qq;
            const int dz = ax < 2 ? qq >> 1 : 0;
            int msk = 0;
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) msk = m == mm ? mask[mm] : msk;
            int bx = 0;
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) bx = m == mm ? bx1[mm] : bx;
            int pref = 0;
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) pref = m == mm ? ISO_FIELD(pre, mm) : pref;
            long long bm = 0;
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) bm = m == mm ? base[L][mm] : bm;
            const int rank = dz ? __popc(msk) + (ax == 1 ? bx : 0) : __popc(msk & ((1 << ax) - 1));
            id3[c] = (int)(bm + pref + rank);
          }
          if (fid < a.fcap[L]) {
            int32_t* f = a.faces[L] + 3 * fid;
            f[0] = id3[0];
            f[1] = id3[1];
            f[2] = id3[2];
          }
        }
      }
    }
    // every lane has read base[][] of this chunk: advance it by the chunk's totals
    __syncthreads();
    if (t < 5 * a.K) {
      const int L = t / 5, m = t - 5 * L;
      unsigned long long tot = 0;
      for (int q = 0; q < ISO_WAVES; ++q) tot += wsum[L][q];
      base[L][m] += ISO_FIELD(tot, m);
    }
  }
}

static int iso_check_dims(long long nx, long long ny, long long nz, int K) {
  if (nx < 2 || ny < 2 || nz < 2 || K < 1 || K > ISO_MAX_LEVELS) return VSA_ERR_ARG;
  // rows are workgroups; a row's counts are i32 (at most 5 (nz - 1) faces)
  if (nx > 0x7FFFFFFFll / ny || nz > 0x7FFFFFFFll / 5) return VSA_ERR_UNSUPPORTED;
  return VSA_OK;
}

static size_t iso_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct IsoLayout {
  size_t counts, offsets, totals, scan_tmp, scan_bytes, total;
};

static int iso_layout(long long nx, long long ny, int K, IsoLayout* l) {
  const size_t n = 2ull * K * (size_t)(nx * ny);
  size_t scan_bytes = 0;
  VSA_HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, (const int32_t*)nullptr, (long long*)nullptr, 0ll, n,
                                      rocprim::plus<long long>(), (hipStream_t)0));
  l->counts = 0;
  l->offsets = iso_align(n * sizeof(int32_t));
  l->totals = l->offsets + iso_align(n * sizeof(long long));
  l->scan_tmp = l->totals + iso_align(2 * ISO_MAX_LEVELS * sizeof(long long));
  l->scan_bytes = scan_bytes;
  l->total = l->scan_tmp + iso_align(scan_bytes ? scan_bytes : 16);
  return VSA_OK;
}

static int iso_args(const float* grid, long long nx, long long ny, long long nz, const float* levels, int K,
                    int inside_above, void* workspace, long long workspace_bytes, IsoArgs* a, IsoLayout* l) {
  if (!grid || !levels || !workspace) return VSA_ERR_ARG;
  if (inside_above != 0 && inside_above != 1) return VSA_ERR_ARG;
  int rc = iso_check_dims(nx, ny, nz, K);
  if (rc != VSA_OK) return rc;
  rc = iso_layout(nx, ny, K, l);
  if (rc != VSA_OK) return rc;
  if (workspace_bytes < (long long)l->total) return VSA_ERR_ARG;
  *a = IsoArgs{};
  a->grid = grid;
  a->nx = nx; a->ny = ny; a->nz = nz; a->R = nx * ny;
  a->K = K;
  a->inside_above = inside_above;
  for (int L = 0; L < K; ++L) a->level[L] = levels[L];
  char* ws = static_cast<char*>(workspace);
  a->counts = reinterpret_cast<int32_t*>(ws + l->counts);
  a->offsets = reinterpret_cast<long long*>(ws + l->offsets);
  a->totals = reinterpret_cast<long long*>(ws + l->totals);
  return VSA_OK;
}

extern "C" long long vsa_isosurface_workspace_bytes(long long nx, long long ny, long long nz, int nr_levels) {
  const int rc = iso_check_dims(nx, ny, nz, nr_levels);
  if (rc != VSA_OK) return rc;
  IsoLayout l;
  const int rl = iso_layout(nx, ny, nr_levels, &l);
  if (rl != VSA_OK) return rl;
  return (long long)l.total;
}

extern "C" int vsa_isosurface_count(const float* grid, long long nx, long long ny, long long nz, const float* levels,
                                    int nr_levels, int inside_above, void* workspace, long long workspace_bytes,
                                    long long* totals, void* stream) {
  if (!totals) return VSA_ERR_ARG;
  IsoArgs a;
  IsoLayout l;
  const int rc = iso_args(grid, nx, ny, nz, levels, nr_levels, inside_above, workspace, workspace_bytes, &a, &l);
  if (rc != VSA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(iso_count_kernel, dim3((unsigned)a.R), dim3(ISO_BLOCK), 0, st, a);
  VSA_HIP_TRY(hipGetLastError());
  size_t scan_bytes = l.scan_bytes;
  VSA_HIP_TRY(rocprim::exclusive_scan(static_cast<char*>(workspace) + l.scan_tmp, scan_bytes,
                                      (const int32_t*)a.counts, a.offsets, 0ll, 2ull * nr_levels * (size_t)a.R,
                                      rocprim::plus<long long>(), st));
  hipLaunchKernelGGL(iso_totals_kernel, dim3(1), dim3(2 * ISO_MAX_LEVELS), 0, st, a);
  VSA_HIP_TRY(hipGetLastError());
  VSA_HIP_TRY(hipMemcpyAsync(totals, a.totals, 2 * nr_levels * sizeof(long long), hipMemcpyDeviceToHost, st));
  VSA_HIP_TRY(hipStreamSynchronize(st));
  for (int q = 0; q < 2 * nr_levels; ++q)
    if (totals[q] >= 0x80000000ll) return VSA_ERR_UNSUPPORTED;
  return VSA_OK;
}

extern "C" int vsa_isosurface_emit(const float* grid, long long nx, long long ny, long long nz, const float* levels,
                                   int nr_levels, int inside_above, const float* origin, const float* spacing,
                                   void* workspace, long long workspace_bytes, const long long* totals,
                                   float* const* verts, int32_t* const* faces, void* stream) {
  if (!origin || !spacing || !totals || !verts || !faces) return VSA_ERR_ARG;
  IsoArgs a;
  IsoLayout l;
  const int rc = iso_args(grid, nx, ny, nz, levels, nr_levels, inside_above, workspace, workspace_bytes, &a, &l);
  if (rc != VSA_OK) return rc;
  for (int c = 0; c < 3; ++c) {
    if (!(spacing[c] > 0.0f)) return VSA_ERR_ARG;
    a.origin[c] = origin[c];
    a.spacing[c] = spacing[c];
  }
  for (int L = 0; L < nr_levels; ++L) {
    if (totals[2 * L] < 0 || totals[2 * L + 1] < 0) return VSA_ERR_ARG;
    if (totals[2 * L] >= 0x80000000ll || totals[2 * L + 1] >= 0x80000000ll) return VSA_ERR_UNSUPPORTED;
    if ((totals[2 * L] && !verts[L]) || (totals[2 * L + 1] && !faces[L])) return VSA_ERR_ARG;
    a.verts[L] = verts[L];
    a.faces[L] = faces[L];
    a.vcap[L] = totals[2 * L];
    a.fcap[L] = totals[2 * L + 1];
  }
  hipLaunchKernelGGL(iso_emit_kernel, dim3((unsigned)a.R), dim3(ISO_BLOCK), 0, (hipStream_t)stream, a);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_mc_table(int8_t* out) {
  if (!out) return VSA_ERR_ARG;
  for (int c = 0; c < 256; ++c)
    for (int q = 0; q < 16; ++q) out[16 * c + q] = h_mc_tris[c][q];
  return VSA_OK;
}
