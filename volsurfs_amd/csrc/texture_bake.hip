// Baking a field appearance model into a texture over a mesh's UV atlas (utils/texture_extraction.py:
// extract_texture_from_color_model and dilate_texture; include/volsurfs_hip.h "texture bake").  The model
// stays a Python callable; everything around it is here:
//   tb_boxes_kernel    per face: check its UVs, count the texels of its UV bounding box
//   tb_scan_kernel     one block: exclusive scan of the per-face box sizes (and, later, of the per-block row counts)
//   tb_owner_kernel    one thread per (face, texel-of-its-box) PAIR: the S samples of the texel for this face; when
//                      one is inside, atomicMax(owner[texel], face).  Pairs, not faces, are the unit of work: a
//                      face's box can hold 1 texel or 10^5, a pair always costs S sample tests.  The grid is fixed and
//                      strides over the device-side pair count, so no host read sits between the scan and this launch.
//   tb_count_kernel    one thread per texel: the inside mask of its owner's samples (64 bits), a block's rows counted
//   tb_plan_kernel     one thread: the row total, and the texel ranges of the chunks the model is evaluated in
//   tb_emit_kernel     one thread per texel: its row offset (block offset + wave scan), then the point and normal of
//                      every inside sample in sample order -- the ORDERED compaction: rows by texel, then by sample
//   tb_resolve_kernel  one thread per (texel, channel) of a chunk: the sum of the texel's rows in sample order / count
//   tb_dilate_*        the 8-neighbour dilation with a per-pixel iteration stamp (a gather: race-free in place)
// Integer atomics only (max, or): two runs give the same bytes.  fp32, no contraction (-ffp-contract=off).
#include "common.h"
#include "pcg32.h"

namespace {

constexpr int TB_BLOCK = 256;
constexpr int TB_WAVES = TB_BLOCK / VSA_WAVE;
constexpr int TB_SCAN_BLOCK = 1024;
constexpr int TB_ERR_UV = 1;          // ctl[2] bits
constexpr int TB_CTL_HEAD = 4;        // ctl: rows, chunks, error bits, unused; then the chunk table
constexpr int TB_MAX_CHUNKS = 1 << 20;

// The uniform number of (seed, face, texel, sample, axis): two multiply-xorshift rounds over the key, one PCG32
// output (include/volsurfs_hip.h states the rule; tests/texture_bake_restated.py restates it in torch).
__device__ __forceinline__ float tb_uniform(unsigned long long seed, int face, int texel, int S, int s, int axis) {
  const unsigned long long M = 0x5851f42d4c957f2dULL;
  unsigned long long h = (seed + (unsigned long long)face + 1ull) * M;
  h ^= h >> 32;
  h = (h + (((unsigned long long)texel * (unsigned)S + (unsigned)s) * 2ull + (unsigned)axis) + 1ull) * M;
  h ^= h >> 32;
  h = h * M + 1442695040888963407ULL;
  Pcg32 rng{h, 1442695040888963407ULL};
  return rng.next_float();
}

struct TbFace2d {           // barycentric_coordinates()'s per-triangle values
  float p1x, p1y, v0x, v0y, v1x, v1y, dot00, dot01, dot11, inv_denom;
  bool ok;
};

__device__ __forceinline__ TbFace2d tb_face2d(const float* __restrict__ uv6) {
  TbFace2d t;
  t.p1x = uv6[0], t.p1y = uv6[1];
  t.v0x = uv6[4] - t.p1x, t.v0y = uv6[5] - t.p1y;     // p3 - p1
  t.v1x = uv6[2] - t.p1x, t.v1y = uv6[3] - t.p1y;     // p2 - p1
  t.dot00 = t.v0x * t.v0x + t.v0y * t.v0y;
  t.dot01 = t.v0x * t.v1x + t.v0y * t.v1y;
  t.dot11 = t.v1x * t.v1x + t.v1y * t.v1y;
  const float denom = t.dot00 * t.dot11 - t.dot01 * t.dot01;
  t.ok = denom != 0.0f && isfinite(denom);
  t.inv_denom = 1.0f / denom;
  return t;
}

// (w, v, u) = bar_coords[0..2] of the point; inside as the reference tests it
__device__ __forceinline__ bool tb_bary(const TbFace2d& t, float px, float py, float b[3]) {
  const float v2x = px - t.p1x, v2y = py - t.p1y;
  const float dot02 = t.v0x * v2x + t.v0y * v2y;
  const float dot12 = t.v1x * v2x + t.v1y * v2y;
  b[2] = (t.dot11 * dot02 - t.dot01 * dot12) * t.inv_denom;
  b[1] = (t.dot00 * dot12 - t.dot01 * dot02) * t.inv_denom;
  b[0] = (1.0f - b[1]) - b[2];
  return t.ok && b[0] >= 0.0f && b[1] >= 0.0f && b[2] >= 0.0f && fabsf(((b[0] + b[1]) + b[2]) - 1.0f) < 1e-6f;
}

// Sample s of texel (ix, iy) for `face`: the centre, or the centre plus the jitter
__device__ __forceinline__ void tb_sample(int ix, int iy, int R, float half_texel, unsigned long long seed, int face,
                                          int S, int s, float& px, float& py) {
  const float fR = (float)R;
  px = (float)ix / fR + half_texel;
  py = (float)iy / fR + half_texel;
  if (s > 0) {
    const int texel = ix * R + iy;
    px = px + ((tb_uniform(seed, face, texel, S, s, 0) - 0.5f) - 1e-6f) / fR;
    py = py + ((tb_uniform(seed, face, texel, S, s, 1) - 0.5f) - 1e-6f) / fR;
  }
}

__device__ __forceinline__ unsigned long long tb_inside_mask(const float* __restrict__ faces_uvs, int face, int ix,
                                                             int iy, int R, float half_texel,
                                                             unsigned long long seed, int S) {
  const TbFace2d t = tb_face2d(faces_uvs + 6ll * face);
  if (!t.ok) return 0ull;
  unsigned long long mask = 0ull;
  for (int s = 0; s < S; ++s) {
    float px, py, b[3];
    tb_sample(ix, iy, R, half_texel, seed, face, S, s, px, py);
    if (tb_bary(t, px, py, b)) mask |= 1ull << s;
  }
  return mask;
}

// The texel box of a face: [x0, x1) x [y0, y1), clamped to the atlas
__device__ __forceinline__ void tb_box(const float* __restrict__ uv6, int R, int& x0, int& x1, int& y0, int& y1) {
  const float fR = (float)R;
  const float minu = fminf(fminf(uv6[0], uv6[2]), uv6[4]) * fR, maxu = fmaxf(fmaxf(uv6[0], uv6[2]), uv6[4]) * fR;
  const float minv = fminf(fminf(uv6[1], uv6[3]), uv6[5]) * fR, maxv = fmaxf(fmaxf(uv6[1], uv6[3]), uv6[5]) * fR;
  x0 = min(max((int)floorf(minu), 0), R), x1 = min(max((int)ceilf(maxu), 0), R);
  y0 = min(max((int)floorf(minv), 0), R), y1 = min(max((int)ceilf(maxv), 0), R);
}

__global__ void __launch_bounds__(TB_BLOCK)
tb_boxes_kernel(const float* __restrict__ faces_uvs, int F, int R, int32_t* __restrict__ box_count,
                int32_t* __restrict__ ctl) {
  const int f = blockIdx.x * TB_BLOCK + threadIdx.x;
  if (f >= F) return;
  const float* uv6 = faces_uvs + 6ll * f;
  bool good = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) good = good && uv6[k] >= 0.0f && uv6[k] <= 1.0f;   // false for NaN
  int n = 0;
  if (good) {
    int x0, x1, y0, y1;
    tb_box(uv6, R, x0, x1, y0, y1);
    n = max(x1 - x0, 0) * max(y1 - y0, 0);
  } else {
    atomicOr(&ctl[2], TB_ERR_UV);
  }
  box_count[f] = n;
}

// out[i] = in[0] + ... + in[i - 1] for i in [0, n]; one block, chunks of TB_SCAN_BLOCK with a carried total
__global__ void __launch_bounds__(TB_SCAN_BLOCK)
tb_scan_kernel(const int32_t* __restrict__ in, long long n, long long* __restrict__ out) {
  __shared__ long long wave_sum[TB_SCAN_BLOCK / VSA_WAVE];
  __shared__ long long carry_s;
  const int lane = threadIdx.x & (VSA_WAVE - 1), wave = threadIdx.x / VSA_WAVE;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (long long base = 0; base < n; base += TB_SCAN_BLOCK) {
    const long long i = base + threadIdx.x;
    const long long v = i < n ? (long long)in[i] : 0ll;
    long long incl = v;
#pragma unroll
    for (int off = 1; off < VSA_WAVE; off <<= 1) {
      const long long u = __shfl_up(incl, off);
      if (lane >= off) incl += u;
    }
    if (lane == VSA_WAVE - 1) wave_sum[wave] = incl;
    __syncthreads();
    long long before = carry_s;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    if (i < n) out[i] = before + incl - v;
    __syncthreads();
    if (threadIdx.x == TB_SCAN_BLOCK - 1) carry_s = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) out[n] = carry_s;
}

__global__ void __launch_bounds__(TB_BLOCK)
tb_owner_kernel(const float* __restrict__ faces_uvs, int F, int R, int S, unsigned long long seed, float half_texel,
                const long long* __restrict__ box_offset, const int32_t* __restrict__ ctl,
                int32_t* __restrict__ owner) {
  if (ctl[2]) return;                                   // refused UVs: nothing is baked
  const long long P = box_offset[F];
  const long long stride = (long long)gridDim.x * TB_BLOCK;
  for (long long p = (long long)blockIdx.x * TB_BLOCK + threadIdx.x; p < P; p += stride) {
    int lo = 0, hi = F - 1;                             // the last face with box_offset[f] <= p
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (box_offset[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int f = lo;
    int x0, x1, y0, y1;
    tb_box(faces_uvs + 6ll * f, R, x0, x1, y0, y1);
    const int h = y1 - y0, local = (int)(p - box_offset[f]);
    const int ix = x0 + local / h, iy = y0 + local % h;
    if (tb_inside_mask(faces_uvs, f, ix, iy, R, half_texel, seed, S)) atomicMax(&owner[ix * R + iy], f);
  }
}

__global__ void __launch_bounds__(TB_BLOCK)
tb_count_kernel(const float* __restrict__ faces_uvs, int R, int S, unsigned long long seed, float half_texel,
                const int32_t* __restrict__ owner, unsigned long long* __restrict__ mask,
                int32_t* __restrict__ block_rows) {
  __shared__ int wave_total[TB_WAVES];
  const int t = blockIdx.x * TB_BLOCK + threadIdx.x;
  unsigned long long m = 0ull;
  if (t < R * R) {
    const int f = owner[t];
    if (f >= 0) m = tb_inside_mask(faces_uvs, f, t / R, t % R, R, half_texel, seed, S);
    mask[t] = m;
  }
  int n = __popcll(m);
#pragma unroll
  for (int off = VSA_WAVE / 2; off > 0; off >>= 1) n += __shfl_xor(n, off);
  if ((threadIdx.x & (VSA_WAVE - 1)) == 0) wave_total[threadIdx.x / VSA_WAVE] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < TB_WAVES; ++w) s += wave_total[w];
    block_rows[blockIdx.x] = s;
  }
}

// ctl[0] = rows, ctl[1] = chunks, ctl[4 + 2 c] = the first texel of chunk c and ctl[5 + 2 c] its first row (entry
// `chunks`: R^2 and the row total): a chunk is the longest run of texels whose rows number <= chunk_rows (chunk_rows >=
// S, so a run holds at least one texel).  The end of a run: the last block that starts within the limit, then a walk
// over that block's texels.
__global__ void tb_plan_kernel(const unsigned long long* __restrict__ mask, const long long* __restrict__ block_offset,
                               int T, int nr_blocks, long long chunk_rows, int max_chunks,
                               int32_t* __restrict__ ctl) {
  if (blockIdx.x || threadIdx.x) return;
  ctl[0] = (int32_t)block_offset[nr_blocks];
  int c = 0, t = 0;
  long long rows_before = 0;                            // rows of the texels before t
  while (t < T && c < max_chunks) {
    ctl[TB_CTL_HEAD + 2 * c] = t;
    ctl[TB_CTL_HEAD + 2 * c + 1] = (int32_t)rows_before;
    ++c;
    const long long limit = rows_before + chunk_rows;
    int lo = t / TB_BLOCK, hi = nr_blocks;              // the last block (or the end) with block_offset <= limit
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (block_offset[mid] <= limit) lo = mid; else hi = mid - 1;
    }
    if (lo == nr_blocks) {
      t = T;
      break;
    }
    int e = lo * TB_BLOCK;
    long long r = block_offset[lo];
    while (e < T) {
      const long long r2 = r + __popcll(mask[e]);
      if (r2 > limit) break;
      r = r2;
      ++e;
    }
    t = e;
    rows_before = r;
  }
  ctl[1] = t >= T ? c : -1;
  ctl[TB_CTL_HEAD + 2 * c] = T;
  ctl[TB_CTL_HEAD + 2 * c + 1] = ctl[0];
}

__global__ void __launch_bounds__(TB_BLOCK)
tb_emit_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
               const float* __restrict__ faces_uvs, int R, int S, unsigned long long seed, float half_texel,
               const int32_t* __restrict__ owner, const unsigned long long* __restrict__ mask,
               const long long* __restrict__ block_offset, int32_t* __restrict__ row_start,
               float* __restrict__ points, float* __restrict__ normals) {
  __shared__ int wave_total[TB_WAVES];
  const int lane = threadIdx.x & (VSA_WAVE - 1), wave = threadIdx.x / VSA_WAVE;
  const int t = blockIdx.x * TB_BLOCK + threadIdx.x;
  const int T = R * R;
  const unsigned long long m = t < T ? mask[t] : 0ull;
  const int n = __popcll(m);
  int incl = n;
#pragma unroll
  for (int off = 1; off < VSA_WAVE; off <<= 1) {
    const int u = __shfl_up(incl, off);
    if (lane >= off) incl += u;
  }
  if (lane == VSA_WAVE - 1) wave_total[wave] = incl;
  __syncthreads();
  long long row = block_offset[blockIdx.x] + (incl - n);
  for (int w = 0; w < wave; ++w) row += wave_total[w];
  if (t >= T) return;
  row_start[t] = (int32_t)row;
  if (t == T - 1) row_start[T] = (int32_t)(row + n);
  if (!n) return;
  const int f = owner[t], ix = t / R, iy = t % R;
  const TbFace2d tri = tb_face2d(faces_uvs + 6ll * f);
  float A[3], B[3], C[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    A[c] = verts[3ll * faces[3ll * f] + c];
    B[c] = verts[3ll * faces[3ll * f + 1] + c];
    C[c] = verts[3ll * faces[3ll * f + 2] + c];
  }
  const float e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
  const float e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
  float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float len = fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-12f);   // F.normalize's eps
  nx = nx / len, ny = ny / len, nz = nz / len;
  for (int s = 0; s < S; ++s) {
    if (!((m >> s) & 1ull)) continue;
    float px, py, b[3];
    tb_sample(ix, iy, R, half_texel, seed, f, S, s, px, py);
    tb_bary(tri, px, py, b);
#pragma unroll
    for (int c = 0; c < 3; ++c) points[3 * row + c] = (b[0] * A[c] + b[1] * B[c]) + b[2] * C[c];
    normals[3 * row] = nx, normals[3 * row + 1] = ny, normals[3 * row + 2] = nz;
    ++row;
  }
}

// texture[t, c] for the texels [t0, t1): vals holds the rows from row_start[t0] on
__global__ void __launch_bounds__(TB_BLOCK)
tb_resolve_kernel(const float* __restrict__ vals, int C, const int32_t* __restrict__ row_start, int t0, int t1,
                  float* __restrict__ texture) {
  const long long i = (long long)blockIdx.x * TB_BLOCK + threadIdx.x;
  if (i >= (long long)(t1 - t0) * C) return;
  const int t = t0 + (int)(i / C), c = (int)(i % C);
  const int r0 = row_start[t], n = row_start[t + 1] - r0;
  if (!n) return;                                        // uncovered: the caller's zero stays
  const long long base = (long long)(r0 - row_start[t0]) * C + c;
  float sum = vals[base];
  for (int k = 1; k < n; ++k) sum = sum + vals[base + (long long)k * C];
  texture[(long long)t * C + c] = sum / (float)n;
}

// ---- dilation.  stamp: 0 = a source of iteration 1 (full), -1 = empty, -2 = neither; i >= 1 = filled in iteration i
__global__ void __launch_bounds__(TB_BLOCK)
tb_dilate_begin_kernel(const float* __restrict__ img, int HW, int C, int32_t* __restrict__ stamp,
                       int32_t* __restrict__ filled, int nr_iters) {
  const int p = blockIdx.x * TB_BLOCK + threadIdx.x;
  if (p <= nr_iters) filled[p] = p == 0 ? 1 : 0;       // filled[i]: did iteration i fill a pixel (filled[0]: go)
  if (p >= HW) return;
  int zeros = 0;
  for (int c = 0; c < C; ++c) zeros += img[(long long)p * C + c] == 0.0f ? 1 : 0;
  stamp[p] = zeros == 0 ? 0 : (zeros == C ? -1 : -2);
}

// Iteration `it`: an empty pixel copies the first neighbour, in the order (-1,-1), (-1,0), (-1,1), (0,-1), (0,1),
// (1,-1), (1,0), (1,1) of (row, column) offsets, whose stamp is it - 1.  No-op once an iteration filled nothing.
__global__ void __launch_bounds__(TB_BLOCK)
tb_dilate_step_kernel(float* __restrict__ img, int H, int W, int C, int32_t* __restrict__ stamp,
                      int32_t* __restrict__ filled, int it) {
  if (filled[it - 1] == 0) return;                       // filled[it] then stays 0: the later launches return too
  const int p = blockIdx.x * TB_BLOCK + threadIdx.x;
  if (p >= H * W || stamp[p] != -1) return;
  const int r = p / W, c = p % W;
  for (int k = 0; k < 8; ++k) {
    const int kk = k < 4 ? k : k + 1;
    const int rr = r + kk / 3 - 1, cc = c + kk % 3 - 1;
    if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
    const int q = rr * W + cc;
    if (stamp[q] != it - 1) continue;
    for (int ch = 0; ch < C; ++ch) img[(long long)p * C + ch] = img[(long long)q * C + ch];
    stamp[p] = it;
    filled[it] = 1;                                      // every writer stores the same value
    return;
  }
}

}  // namespace

static inline bool tb_shape_ok(int R, int S) {
  return R >= 1 && R <= 8192 && S >= 1 && S <= 64 && (long long)R * R * S <= 0x7FFFFFFFll;
}
static inline long long tb_align(long long n) { return (n + 255) / 256 * 256; }
static inline int tb_blocks(int R) { return vsa_div_up((long long)R * R, TB_BLOCK); }

extern "C" long long vsa_tb_max_chunks(int resolution, int nr_samples, long long chunk_rows) {
  if (!tb_shape_ok(resolution, nr_samples) || chunk_rows < nr_samples) return VSA_ERR_ARG;
  // a chunk that is not the last holds more than chunk_rows - S rows
  const long long n = (long long)resolution * resolution * nr_samples / (chunk_rows - nr_samples + 1) + 2;
  return n <= TB_MAX_CHUNKS ? n : VSA_ERR_ARG;   // the plan walks the chunks on one thread
}

extern "C" long long vsa_tb_workspace_bytes(long long nr_faces, int resolution) {
  if (nr_faces < 1 || nr_faces > 0x7FFFFFFFll - TB_BLOCK || resolution < 1 || resolution > 8192) return VSA_ERR_ARG;
  const long long T = (long long)resolution * resolution, nb = tb_blocks(resolution);
  return tb_align(4 * nr_faces) + tb_align(8 * (nr_faces + 1)) + tb_align(8 * T) + tb_align(4 * nb) +
         tb_align(8 * (nb + 1));
}

extern "C" int vsa_tb_samples(const float* faces_uvs, long long nr_faces, int resolution, int nr_samples,
                              unsigned long long seed, long long chunk_rows, void* workspace,
                              long long workspace_bytes, int32_t* owner, int32_t* ctl, int ctl_len, void* stream) {
  const long long need = vsa_tb_workspace_bytes(nr_faces, resolution);
  const long long max_chunks = vsa_tb_max_chunks(resolution, nr_samples, chunk_rows);
  if (need < 0 || max_chunks < 0 || workspace_bytes < need || ctl_len < TB_CTL_HEAD + 2 * (max_chunks + 1))
    return VSA_ERR_ARG;
  if (!faces_uvs || !workspace || !owner || !ctl) return VSA_ERR_ARG;
  const int F = (int)nr_faces, R = resolution, S = nr_samples, T = R * R, nb = tb_blocks(R);
  char* w = (char*)workspace;
  int32_t* box_count = (int32_t*)w;
  w += tb_align(4ll * F);
  long long* box_offset = (long long*)w;
  w += tb_align(8ll * (F + 1));
  unsigned long long* mask = (unsigned long long*)w;
  w += tb_align(8ll * T);
  int32_t* block_rows = (int32_t*)w;
  w += tb_align(4ll * nb);
  long long* block_offset = (long long*)w;
  hipStream_t st = (hipStream_t)stream;
  const float half_texel = (float)(1.0 / (2.0 * R));
  int cus = 0;
  if (int rc = vsa_cu_count(&cus)) return rc;
  VSA_HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(int32_t) * ctl_len, st));
  VSA_HIP_TRY(hipMemsetAsync(owner, 0xFF, sizeof(int32_t) * T, st));
  hipLaunchKernelGGL(tb_boxes_kernel, dim3(vsa_div_up(F, TB_BLOCK)), dim3(TB_BLOCK), 0, st, faces_uvs, F, R,
                     box_count, ctl);
  hipLaunchKernelGGL(tb_scan_kernel, dim3(1), dim3(TB_SCAN_BLOCK), 0, st, box_count, (long long)F, box_offset);
  hipLaunchKernelGGL(tb_owner_kernel, dim3(cus * 8), dim3(TB_BLOCK), 0, st, faces_uvs, F, R, S, seed, half_texel,
                     box_offset, ctl, owner);
  hipLaunchKernelGGL(tb_count_kernel, dim3(nb), dim3(TB_BLOCK), 0, st, faces_uvs, R, S, seed, half_texel, owner,
                     mask, block_rows);
  hipLaunchKernelGGL(tb_scan_kernel, dim3(1), dim3(TB_SCAN_BLOCK), 0, st, block_rows, (long long)nb, block_offset);
  hipLaunchKernelGGL(tb_plan_kernel, dim3(1), dim3(1), 0, st, mask, block_offset, T, nb, chunk_rows,
                     (int)max_chunks, ctl);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_tb_emit(const float* verts, const int32_t* faces, const float* faces_uvs, long long nr_faces,
                           int resolution, int nr_samples, unsigned long long seed, const void* workspace,
                           long long workspace_bytes, const int32_t* owner, int32_t* row_start, float* points,
                           float* normals, void* stream) {
  const long long need = vsa_tb_workspace_bytes(nr_faces, resolution);
  if (need < 0 || !tb_shape_ok(resolution, nr_samples) || workspace_bytes < need) return VSA_ERR_ARG;
  if (!verts || !faces || !faces_uvs || !workspace || !owner || !row_start || !points || !normals)
    return VSA_ERR_ARG;
  const int F = (int)nr_faces, R = resolution, T = R * R, nb = tb_blocks(R);
  const char* w = (const char*)workspace;
  w += tb_align(4ll * F) + tb_align(8ll * (F + 1));
  const unsigned long long* mask = (const unsigned long long*)w;
  w += tb_align(8ll * T) + tb_align(4ll * nb);
  const long long* block_offset = (const long long*)w;
  hipLaunchKernelGGL(tb_emit_kernel, dim3(nb), dim3(TB_BLOCK), 0, (hipStream_t)stream, verts, faces, faces_uvs, R,
                     nr_samples, seed, (float)(1.0 / (2.0 * R)), owner, mask, block_offset, row_start, points,
                     normals);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_tb_resolve(const float* vals, int nr_channels, const int32_t* row_start, int texel_begin,
                              int texel_end, int resolution, float* texture, void* stream) {
  if (resolution < 1 || resolution > 8192 || nr_channels < 1 || texel_begin < 0 || texel_end < texel_begin ||
      texel_end > resolution * resolution)
    return VSA_ERR_ARG;
  if (texel_end == texel_begin) return VSA_OK;
  if (!vals || !row_start || !texture) return VSA_ERR_ARG;
  const long long n = (long long)(texel_end - texel_begin) * nr_channels;
  hipLaunchKernelGGL(tb_resolve_kernel, dim3(vsa_div_up(n, TB_BLOCK)), dim3(TB_BLOCK), 0, (hipStream_t)stream, vals,
                     nr_channels, row_start, texel_begin, texel_end, texture);
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_tb_dilate(float* img, int height, int width, int nr_channels, int nr_iterations, int32_t* stamp,
                             int32_t* filled, void* stream) {
  if (height < 1 || width < 1 || nr_channels < 1 || nr_iterations < 0 || nr_iterations > 4096 ||
      (long long)height * width > 0x7FFFFFFFll - TB_BLOCK)
    return VSA_ERR_ARG;
  if (!img || !stamp || !filled) return VSA_ERR_ARG;
  const int HW = height * width;
  const dim3 grid(vsa_div_up(HW > nr_iterations + 1 ? HW : nr_iterations + 1, TB_BLOCK));
  hipLaunchKernelGGL(tb_dilate_begin_kernel, grid, dim3(TB_BLOCK), 0, (hipStream_t)stream, img, HW, nr_channels,
                     stamp, filled, nr_iterations);
  for (int it = 1; it <= nr_iterations; ++it)
    hipLaunchKernelGGL(tb_dilate_step_kernel, dim3(vsa_div_up(HW, TB_BLOCK)), dim3(TB_BLOCK), 0,
                       (hipStream_t)stream, img, height, width, nr_channels, stamp, filled, it);
  VSA_RETURN_LAUNCH_STATUS();
}
