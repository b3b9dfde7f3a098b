// Which faces does any training view see?  (The baker's `--remove_invisible_faces`, volsurfs_py/baker.py:140-144: a
// commented-out stub in the reference, so the rule is this library's own — include/volsurfs_hip.h "Face visibility",
// restated, unpinned.)
//
// vsa_face_view_counts: V cameras x H x W pixels x s x s sub-pixel samples x K shells -> one integer per face: how many
// samples had that face as the shell's closest hit.  A wave owns a tile of 64 samples of one view and one shell, makes
// its rays in registers (pinhole.h: the arithmetic of vsa_camera_rays, camera through scalar loads), walks the q16
// nodes (trace_walk.h: the walk of vsa_trace_q, same closest hit bit for bit) and adds its hits to the faces' counters:
// lanes that hit the same face are found by a ballot and add once, the popcount.  No ray, hit record or per-pixel value
// is written to memory; the only stores are the integer atomics, so the counts are exact and do not depend on scheduling.
//
// vsa_face_ring_dilate: a face mask grown by vertex rings (faces -> their vertices -> every face of those vertices), two
// passes per ring so that a ring reads the previous ring's mask only.
#include "common.h"
#include "pinhole.h"
#include "trace_walk.h"

namespace {

struct FaceBases {
  long long base[VSA_MAX_SHELLS];
};

enum { TILE_8X8 = 0, TILE_ROW = 1 };

// Samples form a grid of (s H) x (s W): sample (X, Y) is sub-pixel sample (X % s, Y % s) of pixel (X / s, Y / s).
// TILE_8X8: a wave owns 8 x 8 neighbouring samples (coherent walks); TILE_ROW: 64 consecutive samples of a sample row.
template <int STACK, int TILE>
__global__ __launch_bounds__(TRACE_BLOCK) void face_view_counts_kernel(
    const uint4* __restrict__ qnodes, const float4* __restrict__ tris, Roots roots, Frames frames, FaceBases bases,
    const float* __restrict__ c2w_all, const float* __restrict__ kinv_all, int tiles_x, int tiles_per_view,
    int samples_h, int samples_w, int supersample, float t_min, unsigned* __restrict__ counts) {
  __shared__ int s_stack[STACK][TRACE_BLOCK];
  const int lane = threadIdx.x;
  const int mesh = blockIdx.y;
  // wave-uniform: view and tile
  const int view = (int)(blockIdx.x / (unsigned)tiles_per_view);
  const int tile = (int)(blockIdx.x - (unsigned)view * (unsigned)tiles_per_view);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int X = TILE == TILE_8X8 ? tx * 8 + (lane & 7) : tx * 64 + lane;
  const int Y = TILE == TILE_8X8 ? ty * 8 + (lane >> 3) : ty;
  const bool alive = X < samples_w && Y < samples_h;      // edge tiles: the lanes outside the image sit out

  const int col = X / supersample, row = Y / supersample;
  const float s = (float)supersample;
  const float x = (float)col + ((float)(X - col * supersample) + 0.5f) / s;
  const float y = (float)row + ((float)(Y - row * supersample) + 0.5f) / s;
  const RayOut r = pinhole_ray(c2w_all + 12ll * view, kinv_all + 9ll * view, x, y);
  const float ox = r.ox, oy = r.oy, oz = r.oz, dx = r.dx, dy = r.dy, dz = r.dz;

  const QRay qr = make_qray(frames.f[mesh], ox, oy, oz, dx, dy, dz);
  Hit best = no_hit();
  int cur = alive ? roots.root[mesh] : TRACE_EMPTY;
  int sp = 0;
  q_walk<STACK, false>(qnodes, tris, qr, ox, oy, oz, dx, dy, dz, t_min, cur, sp, best, s_stack, lane, 0);

  // Count.  The wave's lanes that hit the same face add once: the first pending lane's face goes to every lane
  // (readlane), a ballot finds the lanes with that face, the leader adds their number.  A tile of a simplified shell
  // is a handful of faces: a handful of atomics per wave instead of 64.
  const bool hit = best.slot >= 0;
  const int id = best.id;
  unsigned* const mesh_counts = counts + bases.base[mesh];
  unsigned long long todo = __builtin_amdgcn_ballot_w64(hit);
  while (todo) {
    const int leader = __builtin_ctzll(todo);
    const int face = __builtin_amdgcn_readlane(id, leader);
    const unsigned long long same = __builtin_amdgcn_ballot_w64(hit && id == face);
    if (lane == leader) atomicAdd(&mesh_counts[face], (unsigned)__builtin_popcountll(same));
    todo &= ~same;
  }
}

__global__ __launch_bounds__(256) void ring_mark_vertices_kernel(const int* __restrict__ faces, long long nr_faces,
                                                                 long long nr_verts, const unsigned char* __restrict__ keep,
                                                                 unsigned char* __restrict__ vert) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= nr_faces || !keep[f]) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = faces[3 * f + c];
    if ((unsigned long long)v < (unsigned long long)nr_verts) vert[v] = 1;      // (every writer stores the same 1)
  }
}

__global__ __launch_bounds__(256) void ring_mark_faces_kernel(const int* __restrict__ faces, long long nr_faces,
                                                              long long nr_verts, const unsigned char* __restrict__ vert,
                                                              unsigned char* __restrict__ keep) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= nr_faces) return;
  bool any = false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = faces[3 * f + c];
    if ((unsigned long long)v < (unsigned long long)nr_verts) any = any || vert[v] != 0;
  }
  if (any) keep[f] = 1;
}

// process-wide tile shape of vsa_face_view_counts (vsa_face_view_counts_tile)
int& face_view_tile() {
  static int tile = TILE_8X8;
  return tile;
}

}  // namespace

extern "C" int vsa_face_view_counts_tile(int tile) {
  if (tile != TILE_8X8 && tile != TILE_ROW) return VSA_ERR_ARG;
  face_view_tile() = tile;
  return VSA_OK;
}

extern "C" int vsa_face_view_counts(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                                    const float* mesh_frames, int nr_meshes, int max_depth, const float* c2w_all,
                                    const float* intrinsics_inv_all, int nr_views, int height, int width,
                                    int supersample, float t_min, const long long* face_base, uint32_t* counts,
                                    void* stream) {
  if (const int rc = check_qtree(qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth, VSA_ERR_ARG)) return rc;
  if (!c2w_all || !intrinsics_inv_all || !face_base || !counts) return VSA_ERR_ARG;
  if (nr_views < 1 || height < 1 || width < 1 || supersample < 1 || supersample > 8) return VSA_ERR_ARG;
  // a u32 count holds every sample of every view: V H W s^2 < 2^32 (each factor checked before the next product)
  long long samples = (long long)nr_views * height;
  if (samples >= (1ll << 32)) return VSA_ERR_ARG;
  samples *= width;
  if (samples >= (1ll << 32)) return VSA_ERR_ARG;
  samples *= supersample * supersample;
  if (samples >= (1ll << 32)) return VSA_ERR_ARG;
  const QTree t = make_qtree(qnodes, tris, mesh_roots, mesh_frames, nr_meshes);
  FaceBases fb;
  for (int i = 0; i < VSA_MAX_SHELLS; ++i) {
    fb.base[i] = i < nr_meshes ? face_base[i] : 0;
    if (fb.base[i] < 0) return VSA_ERR_ARG;
  }
  const int tile = face_view_tile();
  const long long sh = (long long)height * supersample, sw = (long long)width * supersample;
  const long long tiles_x = tile == TILE_8X8 ? (sw + 7) / 8 : (sw + 63) / 64;
  const long long tiles_y = tile == TILE_8X8 ? (sh + 7) / 8 : sh;
  const long long tiles = tiles_x * tiles_y;          // <= samples of a view
  if (tiles * nr_views > 0x7fffffffll) return VSA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(tiles * nr_views), nr_meshes), block(TRACE_BLOCK);
  with_stack(max_depth, [&](auto st) {
    with_choice<TILE_8X8, TILE_ROW>(tile == TILE_8X8, [&](auto tl) {
      hipLaunchKernelGGL((face_view_counts_kernel<decltype(st)::value, decltype(tl)::value>), grid, block, 0,
                         (hipStream_t)stream, t.qnodes, t.tris, t.roots, t.frames, fb, c2w_all, intrinsics_inv_all,
                         (int)tiles_x, (int)tiles, (int)sh, (int)sw, supersample, t_min, counts);
    });
  });
  VSA_RETURN_LAUNCH_STATUS();
}

extern "C" int vsa_face_ring_dilate(const int32_t* faces, long long nr_faces, long long nr_verts, uint8_t* keep,
                                    int rings, uint8_t* vert_scratch, void* stream) {
  if (!faces || !keep || !vert_scratch || nr_faces < 1 || nr_verts < 1 || rings < 0 || rings > 16) return VSA_ERR_ARG;
  if (nr_faces > 0x7fffffffll * 256) return VSA_ERR_UNSUPPORTED;
  const dim3 grid(vsa_div_up(nr_faces, 256)), block(256);
  for (int ring = 0; ring < rings; ++ring) {
    VSA_HIP_TRY(hipMemsetAsync(vert_scratch, 0, (size_t)nr_verts, (hipStream_t)stream));
    hipLaunchKernelGGL(ring_mark_vertices_kernel, grid, block, 0, (hipStream_t)stream, faces, nr_faces, nr_verts, keep,
                       vert_scratch);
    hipLaunchKernelGGL(ring_mark_faces_kernel, grid, block, 0, (hipStream_t)stream, faces, nr_faces, nr_verts,
                       vert_scratch, keep);
  }
  VSA_RETURN_LAUNCH_STATUS();
}
