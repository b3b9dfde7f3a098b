/* volsurfs_hip.h — C-ABI of libvolsurfs_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the VolSurfs K-shell render hot path.
 * The reference's own boundary is the pybind11 module `volsurfs`
 * (/root/reference/src/PyBridge.cxx:19-139) plus three third-party native
 * modules the hot path calls (raytracelib, tinycudann, mvdatasets helpers).
 * Every entry point below is what a binding for one of those call sites would
 * bind; the reference interface it replaces is cited per function.
 *
 * Conventions
 *   - plain pointers + sizes, no torch / STL types; all pointers are DEVICE
 *     pointers unless a parameter is marked [host];
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     every launch is stream-ordered and asynchronous (the reference
 *     synchronises after every kernel, src/VolumeRendering.cu:64; callers only
 *     consume returned tensors, so async is legal — SURVEY §8b "Threading");
 *   - return value: 0 = ok, >0 = hipError_t of the failed call/launch,
 *     <0 = VSA_ERR_* argument / support error.  Nothing is printed-and-ignored;
 *   - caller owns every buffer; the library keeps no global state except
 *     objects created by *_create and destroyed by *_destroy;
 *   - fp32 row-major tensors, int32 indices (reference layout);
 *   - every device buffer starts 16-byte aligned (rows and slabs are moved with 16-byte loads,
 *     stores and LDS-DMA; any allocator's base pointer qualifies, an odd view into one may not).
 */
#ifndef VOLSURFS_HIP_H
#define VOLSURFS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSA_OK 0
#define VSA_ERR_ARG (-1)
#define VSA_ERR_UNSUPPORTED (-2)

#define VSA_MAX_SHELLS 16

/* Library version / build info (sanity check used by the loader). */
int vsa_version(void);

/* ------------------------------------------------------------------------
 * A7  Dense K-shell alpha composite.
 * Replaces the PyTorch op sequence volsurfs_py/methods/volsurfs.py:601-640 and
 * :704-708 (forward) and its autograd replay (backward).
 *   surfs_rgb   [N,K,3] f32, surfs_alpha [N,K] f32 — inner->outer shell order,
 *               zero where the ray misses the shell (volsurfs.py:455-456).
 *   rgb_bg      [N,3] f32, or [1,3] when bg_is_broadcast (volsurfs.py:688).
 *   out_rgb     [N,3]  = rgb_fg + bg_T * rgb_bg             (required)
 *   out_rgb_fg  [N,3], out_bg_transmittance [N], out_weights [N,K],
 *   out_surfs_rgb_h [N,K,3], out_surfs_alpha_h [N,K]: optional (NULL to skip);
 *               the last two are the fp16-rounded copies the reference returns
 *               (volsurfs.py:732-733).
 *   carry_f16   0: running transmittance carried in fp32, rounded per store
 *               (ATen CPU cumprod; pinned by tests/golden); 1: carried in fp16
 *               (ATen CUDA scan).
 *   1 <= K <= 9 (reference configs ship K = 1,3,5,7,9).
 */
int vsa_composite_dense_fwd(const float* surfs_rgb, const float* surfs_alpha,
                            const float* rgb_bg, int bg_is_broadcast, float* out_rgb,
                            float* out_rgb_fg, float* out_bg_transmittance, float* out_weights,
                            float* out_surfs_rgb_h, float* out_surfs_alpha_h, int nr_rays,
                            int nr_shells, int carry_f16, void* stream);

/* Backward of out_rgb w.r.t. surfs_rgb, surfs_alpha (and per-ray rgb_bg when
 * g_rgb_bg != NULL, [N,3]); forward is recomputed in registers. */
int vsa_composite_dense_bwd(const float* surfs_rgb, const float* surfs_alpha,
                            const float* rgb_bg, int bg_is_broadcast, const float* g_rgb,
                            float* g_surfs_rgb, float* g_surfs_alpha, float* g_rgb_bg,
                            int nr_rays, int nr_shells, int carry_f16, void* stream);

/* The same with the L1 image loss of utils/losses.py:14-19 fused in: the upstream gradient
 * is formed in the kernel as loss_scale * sign(pred_rgb - gt_rgb) (loss_scale = 1 / (3 N_global)
 * for the mean), saving three elementwise passes over [N,3]. */
int vsa_composite_dense_bwd_l1(const float* surfs_rgb, const float* surfs_alpha,
                               const float* rgb_bg, int bg_is_broadcast, const float* pred_rgb,
                               const float* gt_rgb, float loss_scale, float* g_surfs_rgb,
                               float* g_surfs_alpha, int nr_rays, int nr_shells, int carry_f16,
                               void* stream);

/* Forward, L1 loss and backward of a training step in ONE pass over the shells' colours: writes the
 * composited out_rgb [N,3] (bit-identical to vsa_composite_dense_fwd) and the gradients of
 * loss_scale * sum |out_rgb - gt_rgb| w.r.t. surfs_rgb / surfs_alpha (as vsa_composite_dense_bwd_l1). */
int vsa_composite_dense_fwd_bwd_l1(const float* surfs_rgb, const float* surfs_alpha,
                                   const float* rgb_bg, int bg_is_broadcast, const float* gt_rgb,
                                   float loss_scale, float* out_rgb, float* g_surfs_rgb,
                                   float* g_surfs_alpha, int nr_rays, int nr_shells, int carry_f16,
                                   void* stream);

/* The two scalar read-outs of a training iteration (csrc/reduce.hip), ONE launch each and no fill in front:
 *   vsa_count_hits: *out (i64, device) = number of entries >= 0 among hit_slot[0..n) — the sample count that
 *     steers the reference's dynamic ray count (trainer.py:293-304; there `samples_3d.shape[0]` after a
 *     boolean-mask compaction, volsurfs.py:713-716);
 *   vsa_l1_mean: *out (f32, device) = mean |pred[i] - gt[i]| over n elements (utils/losses.py:14-19, loss_l1
 *     without mask), summed in f64 in a fixed order (the same bits every call).
 * scratch: device memory of vsa_reduce_scratch_bytes() bytes, 8-byte aligned, ZEROED before its first use and
 * left ready for the next call by every call; calls that share it must be ordered on one stream.
 * hit_slot / pred / gt: 16-byte aligned. */
long long vsa_reduce_scratch_bytes(void);
int vsa_count_hits(const int32_t* hit_slot, long long n, void* scratch, int64_t* out, void* stream);
int vsa_l1_mean(const float* pred, const float* gt, long long n, void* scratch, float* out, void* stream);

/* ------------------------------------------------------------------------
 * A2  BVH build (host) + K-shell closest-hit traversal (device).
 * Replaces raytracelib.RayTracer(tensor_meshes) / .trace(rays_o, rays_d, mesh_id)
 * at volsurfs_py/methods/volsurfs.py:128 and :476-485 (raytracelib is an
 * un-vendored submodule, .gitmodules:14-17; a reference binding would wrap
 * these in a class exposing `trace`).
 *
 * vsa_bvh_build  [host pointers]  verts [nv,3] f32, faces [nf,3] i32.
 *   Binned-SAH binary BVH, leaves <= leaf_size (1..8) triangles.
 * vsa_bvh_sizes  node / triangle counts and tree depth of a built BVH.
 * vsa_bvh_export [host pointers]  nodes_out [nr_nodes,16] f32 (64-B nodes:
 *   child0 box (6), child1 box (6), ref0, ref1, cnt0, cnt1 as i32 bits;
 *   ref >= 0 inner node index, ref < 0 leaf with first triangle ~ref),
 *   tris_out [nr_tris,12] f32 in leaf order: v0.xyz, original face id (i32
 *   bits), e1.xyz, 0, e2.xyz, 0.  node_base / tri_base are added to the
 *   references so that K meshes can be concatenated into one array pair.
 */
typedef struct vsa_bvh vsa_bvh;
int vsa_bvh_build(const float* verts, const int32_t* faces, int nr_verts, int nr_faces,
                  int leaf_size, vsa_bvh** out_bvh);
int vsa_bvh_sizes(const vsa_bvh* bvh, int* nr_nodes, int* nr_tris, int* max_depth);
int vsa_bvh_export(const vsa_bvh* bvh, float* nodes_out, float* tris_out, int node_base,
                   int tri_base);
/* Quantised export for vsa_trace_q: qnodes_out [nr_nodes,8] u32 (32-B nodes: per child three
 * dwords of 6 x u16 box coordinates on the mesh's grid, rounded outward; dwords 6, 7 = the
 * children: node index >= 0, leaf code ~((first_tri << 4) | count), or 0x7fffffff = none),
 * frame_out [6] = grid origin xyz and step xyz, tris_out as vsa_bvh_export. */
int vsa_bvh_export_q(const vsa_bvh* bvh, uint32_t* qnodes_out, float* tris_out, int node_base,
                     int tri_base, float* frame_out);
/* Refit after the vertices moved (same faces, same nr_verts as the build): triangle records and
 * child boxes are recomputed in place, bottom-up; leaf order — hence every triangle slot id and any
 * per-slot table of the caller — is unchanged.  Re-export afterwards.  Closest hits through the
 * refitted tree are bit-identical to those of a fresh build (the boxes only prune).
 * Replaces re-running `RayTracer(tensor_meshes)` (volsurfs.py:82-128) when only positions changed. */
int vsa_bvh_refit(vsa_bvh* bvh, const float* verts, int nr_verts);
int vsa_bvh_destroy(vsa_bvh* bvh);

/* The same build on the GPU from the meshes' DEVICE arrays (csrc/bvh_device.hip): a Karras LBVH on 30-bit Morton
 * codes of the triangle centroids, leaves of <= leaf_size (1..8) triangles, emitted in the layouts of vsa_bvh_export
 * and vsa_bvh_export_q.  Replaces the host copy + vsa_bvh_build of raytracelib.RayTracer(tensor_meshes)
 * (volsurfs_py/methods/volsurfs.py:128) where the shells already live on the device.  Closest hits through it are
 * bit-identical to the host tree's (the boxes only prune); its SAH cost is higher.  The handle owns its device
 * buffers (a copy of verts and faces among them) until vsa_bvh_dev_destroy.
 * vsa_bvh_dev_build   verts [nv,3] f32, faces [nf,3] i32: DEVICE pointers; enqueued on `stream`, no sync.
 *   VSA_ERR_ARG on null pointers or nr_verts / nr_faces <= 0 (before any HIP call).
 * vsa_bvh_dev_sizes   synchronises the build; node / triangle counts and depth as vsa_bvh_sizes.
 *   VSA_ERR_ARG when a face indexes outside the vertices, VSA_ERR_UNSUPPORTED when max_depth >= 48 (the
 *   traversal's stack; use the host builder).  Call it once before the first export.
 * vsa_bvh_dev_export  nodes_out [nr_nodes,16] f32, qnodes_out [nr_nodes,8] u32, tris_out [nr_tris,12] f32: DEVICE;
 *   frame_out [6] [host] (vsa_trace_q takes host frames).  node_base / tri_base as vsa_bvh_export; synchronises
 *   `stream` to hand back the frame.
 * vsa_bvh_dev_refit   the vertices moved (same faces, same nr_verts, DEVICE pointer): triangle boxes, child boxes
 *   and the q16 frame are recomputed on `stream`; leaf order (every triangle slot) is unchanged.  Re-export
 *   afterwards.  Replaces re-running RayTracer(tensor_meshes) (volsurfs.py:82-128) when only positions changed. */
typedef struct vsa_bvh_dev vsa_bvh_dev;
int vsa_bvh_dev_build(const float* verts, const int32_t* faces, int nr_verts, int nr_faces, int leaf_size,
                      void* stream, vsa_bvh_dev** out_bvh);
int vsa_bvh_dev_sizes(const vsa_bvh_dev* bvh, int* nr_nodes, int* nr_tris, int* max_depth);
int vsa_bvh_dev_export(const vsa_bvh_dev* bvh, float* nodes_out, uint32_t* qnodes_out, float* tris_out,
                       int node_base, int tri_base, float* frame_out, void* stream);
int vsa_bvh_dev_refit(vsa_bvh_dev* bvh, const float* verts, int nr_verts, void* stream);
int vsa_bvh_dev_destroy(vsa_bvh_dev* bvh);
/* vsa_bvh_dev_build_ploc: the same handle, built by PLOC clustering (Meister & Bittner 2018; csrc/bvh_ploc.hip)
 * over the same Morton-sorted triangles: each cluster merges with the neighbour within `radius` positions of the
 * Morton-ordered cluster array (1..32; RayTracer's default is in DESIGN §12) whose union box has the smallest
 * surface area, until one cluster is left.  Its SAH cost lies between the LBVH's and the host tree's; the build
 * synchronises `stream` a few times (it reads the live cluster count once per batch of iterations).
 * vsa_bvh_dev_sizes / _export / _refit / _destroy serve it unchanged; refit keeps its topology and slots.
 *   VSA_ERR_ARG on null pointers, nr_verts / nr_faces <= 0 or radius outside 1..32 (before any HIP call). */
int vsa_bvh_dev_build_ploc(const float* verts, const int32_t* faces, int nr_verts, int nr_faces, int leaf_size,
                           int radius, void* stream, vsa_bvh_dev** out_bvh);

/* vsa_trace: closest hit of every ray against each of nr_meshes BVHs in ONE
 * launch (grid.y = mesh).  mesh_roots [host, nr_meshes] = root node index of
 * each mesh in `nodes`; max_depth = deepest tree (must be < 48).
 *   rays_o, rays_d [N,3] f32 (rays_d need not be normalised; t is in units of
 *   |rays_d|).  Hit iff t > t_min; closest = smallest t, ties -> smallest
 *   original face id (order independent, bit-identical to the brute-force
 *   oracle).  Outputs, mesh-major [nr_meshes, N]: hit_t (0 on miss),
 *   hit_slot (index into `tris`, -1 on miss), hit_uv [.,.,2] = barycentric
 *   weights of v1 and v2. */
int vsa_trace(const float* nodes, const float* tris, const int32_t* mesh_roots, int nr_meshes,
              int max_depth, const float* rays_o, const float* rays_d, int nr_rays, float t_min,
              float* hit_t, int32_t* hit_slot, float* hit_uv, void* stream);

/* vsa_trace on the quantised nodes of vsa_bvh_export_q (half the node bytes; identical
 * results).  mesh_frames [host, nr_meshes*6].  Valid while ray origins stay within ~60 mesh
 * extents of the mesh (fp32 error of the origin in grid units < the boxes' outward margin);
 * beyond that use vsa_trace. */
int vsa_trace_q(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                const float* mesh_frames, int nr_meshes, int max_depth, const float* rays_o,
                const float* rays_d, int nr_rays, float t_min, float* hit_t, int32_t* hit_slot,
                float* hit_uv, void* stream);
/* The same launch with NARROW waves: rays_per_wave (1 .. 64) rays per 64-lane wave, the other lanes idle.  For small
 * batches of incoherent rays (a training batch: a few ten thousand random pixels of many views): a wave walks until
 * its slowest ray is done, so fewer rays per wave mean shorter dependent chains and more waves to hide them behind —
 * the chip is mostly empty at that size anyway.  Same hits (a ray's walk does not depend on its wave). */
int vsa_trace_q_narrow(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                       const float* mesh_frames, int nr_meshes, int max_depth, const float* rays_o,
                       const float* rays_d, int nr_rays, float t_min, float* hit_t, int32_t* hit_slot,
                       float* hit_uv, int rays_per_wave, void* stream);
/* vsa_trace_q with the launch order taken from the previous call's measured cost (identical results):
 * every wave files itself, by the trips its walk took, into one of three lists of the NEXT call's
 * order; the next call dispatches the lists first (longest walks first), then everything else in the
 * natural order.  A wave's trips depend on its rays only, so for the same rays the prediction is
 * exact, and for a camera that moved a little it is close; for unrelated rays it is as good as any
 * order.  Why: the few waves that hold grazing rays walk 10-20x the median; dispatched late they leave
 * the chip draining for a third of the launch (profiles/NOTEBOOK.md A9.4).  feedback: device memory, 16-byte
 * aligned, >= vsa_trace_feedback_bytes(nr_rays, nr_meshes) (< 0 on bad arguments), ZEROED by the
 * caller before its first use, then owned by this sequence of calls with the SAME feedback_bytes
 * (a buffer sized for more rays serves fewer: a half written for another item count is recognised
 * and ignored): phase alternates 0, 1, 0, ... (the half written by one call is read by the next),
 * or phase = 2: the phase lives in the buffer itself and a one-wave kernel in front of the launch
 * flips it — the form to use inside a captured graph, where a host-side toggle would be frozen and
 * every replay would read the half the last eager call wrote;
 * calls that share a feedback buffer must be ordered on one stream.  The lists and flags a
 * call reads always partition the items, so the hits do not depend on what they were measured on. */
long long vsa_trace_feedback_bytes(int nr_rays, int nr_meshes);
int vsa_trace_q_fb(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                   const float* mesh_frames, int nr_meshes, int max_depth, const float* rays_o,
                   const float* rays_d, int nr_rays, float t_min, float* hit_t, int32_t* hit_slot,
                   float* hit_uv, void* feedback, long long feedback_bytes, int phase, void* stream);
/* The cooperative finish of vsa_trace_q_fb (same call site, volsurfs.py:476-485): a wave walks one ray per lane until
 * its slowest ray is done — a grazing ray takes 100-360 trips of the walk against a median of 9, and a small launch is
 * as long as its longest wave.  In launches of at most `max_waves` waves (nr_meshes x ceil(nr_rays / 64): training
 * batches; larger launches keep the plain walk, whose register budget holds five waves per SIMD) a wave looks every
 * `chunk` trips at how many of its lanes are still walking, and once they are at most `lanes` the WHOLE wave finishes
 * those rays together: their pending subtrees go into a queue of (node, ray) entries, every lane takes one entry per
 * round and appends the children that survive.  The hits are bit for bit those of the plain walk (the closest hit is
 * a minimum over (t, face id); a stale bound only visits more).  Process-wide setting, defaults 16 / 24 / 4096;
 * lanes = 0 switches it off.  Returns VSA_ERR_ARG for chunk < 1, lanes outside 0..64 or max_waves < 0. */
int vsa_trace_coop_config(int chunk, int lanes, long long max_waves);
/* Measurement aid (bench.py's stage_roofline.trace; not on the product path): the walk of vsa_trace_q with
 * counters.  stats (device, 5 x u64, overwritten): lane-level node visits (one 32-byte node fetch each),
 * lane-level triangle tests (48 bytes each), wave-level trips of the walk loop summed over the waves (one trip =
 * one dependent node fetch of a whole wave), waves, and the longest wave's trips. */
int vsa_trace_q_stats(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                      const float* mesh_frames, int nr_meshes, int max_depth, const float* rays_o,
                      const float* rays_d, int nr_rays, float t_min, uint64_t* stats, void* stream);
/* vsa_hit_attributes: expands one mesh's hit records [N] into the dict
 * raytracelib returns (volsurfs.py:496-501): is_hit [N] u8, triangles_id [N]
 * i32 (original face index, -1 on miss), positions [N,3] = o + t d, normals
 * [N,3] = unit geometric face normal (e1 x e2), barycentric [N,3] =
 * (1-u-v, u, v).  Any output may be NULL. */
int vsa_hit_attributes(const float* tris, const float* rays_o, const float* rays_d,
                       const float* hit_t, const int32_t* hit_slot, const float* hit_uv,
                       int nr_rays, uint8_t* is_hit, int32_t* tri_id, float* positions,
                       float* normals, float* barycentric, void* stream);

/* ------------------------------------------------------------------------
 * A3/A4/A6  Neural-texture appearance of the K shells (the "shade" stage).
 * Replaces, per shell and per model, SHNeuralTextures.forward
 * (volsurfs_py/models/sh_neural_textures.py:64-97) -> NeuralTexture.forward
 * (models/neural_texture.py:81-197) -> tcnn HashGrid + FullyFusedMLP
 * (neural_texture.py:54-77; tiny-cuda-nn is a pip dependency, absent), plus the
 * uv interpolation / alpha decay / scatter around it (methods/volsurfs.py:504-516,
 * 539-596) and the autograd replay of all of it.
 *
 * MI355X design (DESIGN.md "Texel-deduplicated shading"): NeuralTexture only
 * ever evaluates its network at TEXEL CENTRES (the 4 lerp corners), so the
 * frame's hits are reduced to the set of unique touched texels per (shell,
 * degree) first; hash encoding + MLP run once per unique texel ("slot") and
 * write the 8-bit quantised texel (exactly the value the reference computes for
 * every hit that touches it); hits then gather 4 corner rows per degree.  Hash
 * levels are processed level-major with the whole level table resident in LDS
 * (2^15 entries x half2 = 128 KiB <= 160 KiB), forward gathers and backward
 * scatter-adds never touch HBM atomics.
 *
 * Indexing: texture x = (shell*2 + type)*4 + degree, type 0 = rgb, 1 = alpha.
 * Texel domain of (shell, degree): (R_d+2)^2 texels (one-texel apron for
 * corners outside [0,1]), padded to a multiple of 4096, concatenated:
 * dom_off[shell*4 + degree].  Slots are numbered globally in domain order.
 */
#define VSA_NT_MAX_LEVELS 16
#define VSA_NT_MAX_DEG 4
#define VSA_NT_WEIGHTS_PER_TEX 8192 /* W1[64][32] W2[64][64] W3[32][64] (rows >= C' zero) */
/* Texel rows (u8) and gradient rows (f32) share one per-degree layout, counted in QUADS
 * (4 elements: 4 bytes of a texel row, 4 floats of a gradient row).  A slot of SH band d
 * (n = 2d+1 coefficients) owns VSA_NT_ROW_QUADS(d) quads: rgb coefficient c (0..3n-1) at
 * element c, alpha coefficient c (0..n-1) at element 4*VSA_NT_ALPHA_QUAD(d) + c; the rest
 * is zero padding.  The row of slot i of segment (shell, d) starts at quad
 * row_base[shell*4+d] + (i - seg_start[shell*4+d]) * VSA_NT_ROW_QUADS(d). */
#define VSA_NT_ROW_QUADS(d) ((d) == 0 ? 2 : ((d) == 1 ? 4 : 8))
#define VSA_NT_ALPHA_QUAD(d) ((d) == 0 ? 1 : ((d) == 1 ? 3 : ((d) == 2 ? 4 : 6)))

typedef struct vsa_nt_plan {
  int32_t nr_shells;                 /* K */
  int32_t rgb_degrees;               /* sh_degree+1 of the rgb models, 1..4 */
  int32_t alpha_degrees;             /* sh_degree+1 of the alpha models, 1..4 */
  int32_t inner_solid;               /* 1: shell 0 has no alpha model (alpha = 1), volsurfs.py:181-183 */
  int32_t with_alpha_decay;          /* volsurfs.py:585-594 */
  int32_t n_levels;                  /* 16 */
  int32_t tex_res[VSA_NT_MAX_DEG];   /* R_d (square textures) */
  float sh_lo[VSA_NT_MAX_DEG];       /* val_range[0] = -sh_range[d] */
  float sh_span[VSA_NT_MAX_DEG];     /* val_range[1]-val_range[0] */
  float level_scale[VSA_NT_MAX_LEVELS];
  int32_t level_res[VSA_NT_MAX_LEVELS];
  int32_t level_size[VSA_NT_MAX_LEVELS];      /* entries */
  int32_t level_offset[VSA_NT_MAX_LEVELS + 1]; /* entries */
  int64_t dom_off[VSA_MAX_SHELLS * VSA_NT_MAX_DEG + 1];
  int64_t slot_capacity;             /* rows allocated in every per-slot buffer */
  int32_t max_rays;                  /* N the buffers were sized for: a (shell,degree)
                                        segment holds <= min(4*max_rays, (R_d+2)^2) slots */
  int32_t anchor;                    /* 0: lerp of the 2x2 texel footprint (the shipped configs, neural_texture.py:106-139);
                                        1: anchor — the sample takes the ONE texel it falls in, unblended (:88-104) */
  int64_t row_base[VSA_MAX_SHELLS * VSA_NT_MAX_DEG + 1]; /* quads; multiples of 8; segment sd
                                        reserves min(4*max_rays,(R_d+2)^2)*VSA_NT_ROW_QUADS(d);
                                        the last entry is the allocation size */
  void* balance;                     /* NULL, or device memory of vsa_nt_balance_bytes() bytes, ZEROED before
                                        its first use: the persistent kernels (encode / MLP, forward and
                                        backward) stamp every workgroup's busy time there and split their
                                        work by the shares vsa_nt_rebalance derived from the previous
                                        launch's times (same pieces, same results: only who does which) */
  int32_t row_format;                /* 0: 8-bit quantised texel rows (using_sh_quantization = 1: every shipped config);
                                        1: f16 rows holding sigmoid(x) un-quantised (using_sh_quantization = 0,
                                        using_sh_squeezing = 1; neural_texture.py:159-164, 183-187) — `texels` is then an
                                        f16 array with the SAME quad layout (a quad = 4 halves = 8 bytes); forward
                                        kernels only differ, the backward is the quantised one's (round is a
                                        straight-through estimator);
                                        2: f16 rows holding the RAW network output (using_sh_squeezing = 0: no sigmoid, no
                                        quantiser, no expansion to val_range; neural_texture.py:157-169, 181-187) — layout as
                                        format 1; the backward passes the row gradient through unchanged (no sigmoid', no span).
                                        vsa_nt_encode_mlp_fwd supports format 0 only */
  int32_t grads_zeroed;              /* 1: the caller vouches that grad_tables is ALL ZERO on entry to vsa_nt_encode_bwd /
                                        _range / _phased (it cleared the buffer, or the fused Adam step did, and nothing
                                        has been accumulated since): a table plane whose slots ONE workgroup walks is then
                                        written with plain stores instead of float atomics (same values: 0 + v).  0: the
                                        launch accumulates into whatever the buffer holds */
  int32_t shared_rgb;                /* 1: are_volsurfs_colors_indep = 0 (methods/volsurfs.py:159-165, 524-527): ONE colour model
                                        `models["rgb"]` for all shells — every shell's colour textures read the parameters of
                                        texture (0*2 + 0)*4 + degree and the gradients of all K shells accumulate there.  Slots,
                                        feature planes and texel rows stay per (shell, degree): only the PARAMETER index maps */
  int32_t shared_alpha;              /* 1: are_volsurfs_alphas_indep = 0 (volsurfs.py:200-206, 553-556): the same for the alpha
                                        model (parameters of texture (0*2 + 1)*4 + degree).  With inner_solid the reference's
                                        loop stores models["alpha"] = None and leaves: NO shell has an alpha model (alpha = 1,
                                        no decay, on every shell) */
} vsa_nt_plan;

/* Measured-time rebalancing of the persistent kernels' work split (profiles/NOTEBOOK.md A9.0): once per frame,
 * before the first of them, turns the busy times the previous frame's launches stamped into
 * plan->balance into per-workgroup shares of each kernel's cost axis (a workgroup that took longer
 * than the mean gets a smaller share, damped).  No-op while nothing has been stamped.
 * vsa_nt_compact_frame does the same inside its own scan launch when plan->balance is set: a frame loop
 * built on it does not call vsa_nt_rebalance. */
long long vsa_nt_balance_bytes(void);
int vsa_nt_rebalance(const vsa_nt_plan* plan, void* stream);

/* Step 1 (per frame): per-hit texture uv + mark touched texels.
 *   hit_slot [K,N] i32, hit_uv [K,N,2] f32 from vsa_trace; face_uvs [nr_tris,6]
 *   f32 = per-corner uvs in leaf (slot) order.  Writes tex_uv [K,N,2] and sets
 *   marks[dom_off[..] + texel] = 1 for the 4 lerp corners of every degree.
 *   marks (u8 [dom_off[K*4]]) must be zero on entry; marks == NULL: tex_uv only (shading from
 *   baked textures needs no compaction). */
int vsa_nt_mark(const vsa_nt_plan* plan, const int32_t* hit_slot, const float* hit_uv,
                const float* face_uvs, int nr_rays, float* tex_uv, uint8_t* marks, void* stream);

/* Step 2 (per frame): compact marks into slots.  slot_of [dom total] i32, texel_of_slot [slot_capacity] i32
 * (domain index; may be NULL), slot_xy [slot_capacity,2] f32 (normalised texel-centre coordinates = the network
 * input of the slot), seg_start [K*4+1] i32 (first slot of each (shell,degree); last = total),
 * block_scratch [dom total/4096 + 1] i32.  slot_of is written only where a texel is marked (entries of untouched
 * texels keep whatever they held: nothing on the path reads them - shading only looks up the corners it marked),
 * and the marks are CLEARED on the way (the next vsa_nt_mark needs no fill).  At 800x800, K = 5 that is 112 MB
 * of -1 and a 28 MB fill less per frame.  The frame loop's invariant is "marks are zero between frames": a
 * vsa_nt_mark that is NOT followed by a successful vsa_nt_compact_frame (an error in between) must be followed by
 * a fill of the marks before the next frame - stale marks inflate every later frame's slot counts. */
int vsa_nt_compact_frame(const vsa_nt_plan* plan, uint8_t* marks, int32_t* slot_of,
                         int32_t* texel_of_slot, float* slot_xy, int32_t* seg_start,
                         int32_t* block_scratch, void* stream);

/* Step 3: hash-grid encode every slot of every texture, level-major with the
 * level table in LDS.  tables_h: f16 [n_tex][level_offset[n]*2];
 * features: f16x2, blocked [2 types][slot_capacity/256][n_levels][256] (slot_capacity
 * is a multiple of 256): a 32-slot MLP tile's 16 levels stay within 16 KiB. */
int vsa_nt_encode_fwd(const vsa_nt_plan* plan, const void* tables_h, const float* slot_xy,
                      const int32_t* seg_start, void* features, void* stream);

/* Step 4: MLP 32->64->64->C' of every slot of every texture on MFMA, fused with
 * sigmoid / x255 / round (neural_texture.py:156-169).  weights_h: f16
 * [n_tex][VSA_NT_WEIGHTS_PER_TEX]; texels: u8 [row_base[last]*4] (quantised texel rows,
 * layout above).  pre_out (optional, tests): f16 [slot_capacity][32], the network output
 * before the sigmoid: rgb channel c at [slot][c], alpha channel c at [slot][24+c]. */
int vsa_nt_mlp_fwd(const vsa_nt_plan* plan, const void* weights_h, const void* features,
                   const int32_t* seg_start, uint8_t* texels, void* pre_out, void* stream);

/* Steps 3 + 4 in ONE launch (the reference's `Sequential(encoding, network)` is one tiny-cuda-nn
 * call per corner batch, models/neural_texture.py:63-79, 153): a wave hash-grid encodes 64
 * consecutive slots (a lane per slot, all levels, table entries gathered through L2) and runs
 * the MLP on them straight from registers (csrc/nt_fused.hip).  Bit-identical to
 * vsa_nt_encode_fwd + vsa_nt_mlp_fwd.  features: NULL, or the blocked feature planes of
 * vsa_nt_encode_fwd, which are then written as well (vsa_nt_mlp_bwd recomputes the forward
 * from them).  pre_out: as vsa_nt_mlp_fwd (optional, tests). */
int vsa_nt_encode_mlp_fwd(const vsa_nt_plan* plan, const void* tables_h, const void* weights_h,
                          const float* slot_xy, const int32_t* seg_start, void* features,
                          uint8_t* texels, void* pre_out, void* stream);

/* Backward of step 4: recomputes the forward per 32-slot tile, back-propagates
 * grad_rows (f16, already multiplied by grad_scale) through sigmoid (round = STE)
 * and the three layers on MFMA.  Overwrites `features` IN PLACE with the feature
 * gradients (f16x2, still scaled) and accumulates grad_weights (f32
 * [n_tex][VSA_NT_WEIGHTS_PER_TEX]) += weight_grad_scale x (the scaled weight gradients), one
 * flush per workgroup; weight_grad_scale = 1 / grad_scale adds the true gradients straight to
 * weights.grad.
 * grad_rows is CONSUMED: every row read is reset to zero, so the buffer (zero
 * at allocation) is zero again outside a [vsa_nt_shade_bwd, vsa_nt_mlp_bwd] pair.
 * dfeat_abs_sum (f32 [n_tex][32], zeroed by the caller) += sum over slots of |dF| per
 * feature row: the overflow bound of vsa_nt_encode_bwd's fixed-point accumulation. */
int vsa_nt_mlp_bwd(const vsa_nt_plan* plan, const void* weights_h, void* features,
                   const int32_t* seg_start, uint16_t* grad_rows, float* grad_weights,
                   float* dfeat_abs_sum, float weight_grad_scale, void* stream);

/* Step 5: per-hit shading from the texel rows (expand LUT -> lerp -> fp16 SH
 * coefficients -> SH eval -> sigmoid -> alpha decay), scattered dense:
 * surfs_rgb [N,K,3], surfs_alpha [N,K] (zero on miss; inner->outer), optional
 * surfs_normals [N,K,3] and coeffs_out [K,N,64] (tests: 48 rgb [ch][16] + 16
 * alpha lerped fp16 SH coefficients).  tris = the tracer's triangle array.
 * act_out (optional, [K,N,4] f32): the three rgb sigmoids and the alpha sigmoid (before
 * the decay) of every hit (entries of misses are NOT written), which vsa_nt_shade_bwd can take
 * back as act_in instead of re-gathering the texel rows and re-evaluating the SH sums. */
int vsa_nt_shade_fwd(const vsa_nt_plan* plan, const int32_t* hit_slot, const float* tex_uv,
                     const float* rays_d, const float* tris, const int32_t* slot_of,
                     const int32_t* seg_start, const uint8_t* texels, int nr_rays,
                     float* surfs_rgb, float* surfs_alpha,
                     float* surfs_normals, float* coeffs_out, float* act_out, void* stream);

/* Backward of step 5: grad_rows (f16 [row_base[last]*4], same row layout as
 * texels; zero on entry, see vsa_nt_mlp_bwd) += grad_scale * dL/d(q/255)
 * (round is a straight-through estimator, utils/math.py:5-18).  act_in: NULL, or the
 * act_out of the forward call on the SAME frame and parameters. */
int vsa_nt_shade_bwd(const vsa_nt_plan* plan, const int32_t* hit_slot, const float* tex_uv,
                     const float* rays_d, const float* tris, const int32_t* slot_of,
                     const int32_t* seg_start, const uint8_t* texels, int nr_rays,
                     const float* g_surfs_rgb,
                     const float* g_surfs_alpha, float grad_scale, uint16_t* grad_rows,
                     const float* act_in, void* stream);

/* Texture export / import (csrc/texture_io.hip): the baked 8-bit texel rows <-> the RGBA8 images of the baker's
 * `--extract_textures` (volsurfs_py/baker.py:778-1009), one image per (shell, degree d, coefficient i).
 *   planes      u8, contiguous [R_d, R_d, 4] images ordered (shell, degree, coefficient): image (s, d, i) starts at
 *               byte s * S + sum_{d' < d} (2d'+1) 4 R_d'^2 + i * 4 R_d^2, S = sum_{d < rgb_degrees} (2d+1) 4 R_d^2;
 *               vsa_nt_planes_bytes(plan) = nr_shells * S (or a VSA_ERR_* code).
 *   orientation pixel (row r, column c) of image (s, d, i) holds texel (iy, ix) = (c, R-1-r) of the network's grid
 *               (the bake grid's axis 0 = u_pix flipped by np.flipud, axis 1 = v_pix), i.e. the texel a hit at uv
 *               reads under anchor addressing when r = floor(v R), c = floor(u R).  Only the R x R interior.
 *   bytes       R, G, B = the texel row's rgb elements channel * (2d+1) + i, A = its alpha element i; A = 255 on a
 *               shell without an alpha model (nt_shell_has_alpha: the solid inner shell, every shell when the alpha
 *               model is shared as well).  The stored 8-bit values unchanged.
 * vsa_nt_export_planes reads the rows through slot_of / seg_start / row_base of a baked bank (every texel marked,
 * then vsa_nt_compact_frame).  vsa_nt_import_planes is the inverse into a bank whose slots were set up the same way:
 * interior rows get the image bytes (padding zero; alpha elements zero without an alpha model), and the one-texel
 * apron is CLAMPED TO THE EDGE: apron texel (iy, ix) gets the row of interior texel (clamp(iy, 0, R-1),
 * clamp(ix, 0, R-1)) -- the border rule of renderers.TensorTexture and of a viewer sampling with CLAMP_TO_EDGE (the
 * baked bank holds the network's values there instead; lerp reads them only for uv within half a texel of the
 * border).  A texel whose slot lies outside its segment is skipped (export: written as zero bytes).
 * planes and texels must be 16-byte aligned and planes_bytes = vsa_nt_planes_bytes(plan).
 * VSA_ERR_ARG: NULL pointers, misalignment, a wrong planes_bytes, nr_shells or a resolution out of range.
 * VSA_ERR_UNSUPPORTED: alpha_degrees != rgb_degrees or row_format != 0. */
long long vsa_nt_planes_bytes(const vsa_nt_plan* plan);
int vsa_nt_export_planes(const vsa_nt_plan* plan, const int32_t* slot_of, const int32_t* seg_start,
                         const uint8_t* texels, uint8_t* planes, long long planes_bytes, void* stream);
int vsa_nt_import_planes(const vsa_nt_plan* plan, const uint8_t* planes, long long planes_bytes,
                         const int32_t* slot_of, const int32_t* seg_start, uint8_t* texels, void* stream);

/* Backward of step 3: grad_tables (f32 [n_tex][level_offset[n]][2]) +=
 * transpose-interpolation of dfeatures (f16x2, same layout as features, holding
 * grad * grad_scale).  Accumulates (caller zeroes grad_tables per optimiser step; plan->grads_zeroed
 * tells the launch that it has, see there). */
int vsa_nt_encode_bwd(const vsa_nt_plan* plan, const void* dfeatures, const float* dfeat_abs_sum,
                      float grad_scale, const float* slot_xy, const int32_t* seg_start,
                      float* grad_tables, void* stream);

/* Process-wide setting of the hash-grid encode launches (vsa_nt_encode_fwd, vsa_nt_encode_bwd, _bwd_range).
 *   sibling_groups  0: the plain walk.  1: the hashed levels are walked in SIBLING GROUPS — two (forward: colour,
 *                   alpha) or four (backward: colour, alpha x feature 0, 1) workgroups of one XCD take the same
 *                   stretch of slots at the same time, each on its own plane, so that the texel centres and dF words
 *                   they all read cross the fabric once (csrc/nt_common.h).  2: in the backward only, 3: in the
 *                   forward only.  The pieces' arithmetic is the plain walk's: features bit for bit, table gradients
 *                   equal wherever a plane is flushed by stores.  Taken when the grid is a multiple of 16 (forward) /
 *                   32 (backward), for at most 64 textures and the whole shell range; any other launch keeps the
 *                   plain walk.  Default 2: the backward fetches 1.3 GB less per 800 x 800 frame and is 6 % shorter,
 *                   the forward fetches 0.2 GB less and is 6 % LONGER.
 *   grid_override   > 0: that many workgroups instead of one per compute unit (tests: cuts and groups on small
 *                   frames); 0: the compute-unit count.
 * Returns VSA_ERR_ARG for sibling_groups outside 0..3 or grid_override outside 0..4096. */
int vsa_nt_encode_config(int sibling_groups, int grid_override);

/* Process-wide switch of the encode kernels' row terms, per direction (1 = on, 0 = off).  A lane of the backward
 * walks 8 consecutive slots, which are texels of one texture row except where the run crosses a row's end; with
 * `backward` on (the default), what the cell arithmetic derives from y alone (fract, floor, 1 - fract, the row's hash
 * products or row offset) is made once per run and again only in waves that hold a row break, instead of once per
 * slot.  The same fp32 operations on the same bits either way: the integer sums do not change.  The backward is 5.5 %
 * shorter with it.  `forward` is accepted and ignored: the forward kernel gained nothing from the same
 * walk, not even with the row terms never remade, and has the per-slot form only (default 0).
 * Call it before the step is captured into a graph.  Returns VSA_ERR_ARG for a value outside 0 / 1. */
int vsa_nt_encode_row_terms(int forward, int backward);

/* The same, restricted to the textures of shells [shell_begin, shell_end): lets a
 * data-parallel caller start the all-reduce of one shell's table gradients (a contiguous
 * slice of grad_tables) while the next shell's are still being accumulated. */
int vsa_nt_encode_bwd_range(const vsa_nt_plan* plan, const void* dfeatures,
                            const float* dfeat_abs_sum, float grad_scale, const float* slot_xy,
                            const int32_t* seg_start, float* grad_tables, int shell_begin,
                            int shell_end, void* stream);

/* Data-parallel form of vsa_nt_encode_bwd (rays shard by tile, the ranks all-reduce the
 * gradients; the reference is single-GPU, so this replaces nothing — it is what keeps the all-reduce
 * of the 113 MB of table gradients off the critical path of trainer.py:249-264's backward).
 *
 * vsa_dp_flags: n (<= VSA_MAX_SHELLS + 1) completion words, zero at creation, each its own 8-byte
 * hipMallocSignalMemory allocation (plain device memory if the runtime refuses), so that another stream
 * can wait for one through the command processor — a waiting KERNEL would park a wave on a CU whose
 * registers the persistent MLP kernels need entirely.  vsa_dp_flags_read: [host] copy of the n words
 * (synchronises the device; tests). */
typedef struct vsa_dp_flags vsa_dp_flags;
int vsa_dp_flags_create(int n, vsa_dp_flags** out);
int vsa_dp_flags_destroy(vsa_dp_flags* flags);
int vsa_dp_flags_read(const vsa_dp_flags* flags, uint32_t* host_out);

/* ONE launch: the shells are cut into n_phases groups, phase p = shells [phase_shell_end[p-1],
 * phase_shell_end[p]) ([host] array, strictly increasing, last = nr_shells); every workgroup walks its
 * share of the dense levels of all shells, then finishes its share of phase p's hashed levels before
 * it touches phase p+1, and when the LAST workgroup is through phase p the kernel stores
 * word p of `flags` = *epoch (system scope; that phase's slice of grad_tables — textures
 * [8*begin, 8*end) — is final and visible).  counters: n_phases device words, zero on entry, zero again
 * on exit.  Results equal vsa_nt_encode_bwd's up to the order of the float atomics that join two
 * workgroups' shares of one table plane (pieces are cut at other slots).
 * Another stream waits for a phase with vsa_dp_stream_wait(flags, p, epoch value).
 * reserve_cus (>= 0): the launch uses that many workgroups fewer than the device has compute units.  A
 * workgroup takes 16 waves, 128 KiB of LDS and most of a CU's vector registers: small kernels run beside it
 * (measured: a 64-workgroup and a 256 MB elementwise kernel finish 0.1-0.3 ms into the 0.65 ms launch), a kernel
 * whose waves need more than the ~64 registers per lane it leaves on a SIMD does not (the traversal: 96) — whether a
 * collective's kernels do is the communication library's business, and this is the knob for it. */
int vsa_nt_encode_bwd_phased(const vsa_nt_plan* plan, const void* dfeatures,
                             const float* dfeat_abs_sum, float grad_scale, const float* slot_xy,
                             const int32_t* seg_start, float* grad_tables, int n_phases,
                             const int32_t* phase_shell_end, vsa_dp_flags* flags, uint32_t* counters,
                             const uint32_t* epoch, int reserve_cus, void* stream);

/* Stream-ordered signal: (*epoch += 1 when advance_epoch), then word `index` of flags = *epoch at system
 * scope — a one-lane kernel, so it can sit inside a captured HIP graph (hipStreamWriteValue32 cannot).
 * The step calls it once behind vsa_nt_mlp_bwd (weights.grad is final), advancing the epoch the phased
 * encode backward then publishes. */
int vsa_dp_signal(vsa_dp_flags* flags, int index, uint32_t* epoch, int advance_epoch, void* stream);

/* Make `stream` wait until word `index` >= value.  mode 1: hipStreamWaitValue32 (on signal memory the
 * command processor polls: no compute resource), mode 2: a one-lane polling kernel ((int32)(word - value)
 * >= 0; it occupies registers of one SIMD: see above), mode 0: 1 where the words are signal memory and
 * hipDeviceAttributeCanUseStreamWaitValue says so, else 2.  ENQUEUE IT AFTER THE PRODUCER: HIP
 * multiplexes streams onto a few hardware queues, and a wait queued ahead of the kernel that
 * satisfies it on the same queue would never return. */
int vsa_dp_stream_wait(vsa_dp_flags* flags, int index, uint32_t value, int mode, void* stream);

/* ------------------------------------------------------------------------
 * A5 / A10  Encoders of the legacy appearance branch and of the background field:
 * the 2-D / 3-D multiresolution hash grid behind GridHashEncoder
 * (volsurfs_py/encodings/gridhash.py:12-92: tcnn.Encoding "Grid"/"Hash", fp32) and
 * SHEncoder.__call__ (volsurfs_py/encodings/sphericalharmonics.py:84-153).
 * tables: fp32 [level_offset[n_levels]][2]; x: fp32 [nr_points][n_dims] in [0,1];
 * out / g_out: fp32 [nr_points][n_levels*2] (level-major, as tcnn returns it).
 */
#define VSA_GRID_MAX_LEVELS 32
typedef struct vsa_grid_plan {
  int32_t n_dims;      /* 2 or 3 */
  int32_t n_levels;
  int32_t n_features;  /* 2 */
  int32_t reserved0;
  float level_scale[VSA_GRID_MAX_LEVELS];
  int32_t level_res[VSA_GRID_MAX_LEVELS];
  int32_t level_size[VSA_GRID_MAX_LEVELS];        /* entries */
  int32_t level_offset[VSA_GRID_MAX_LEVELS + 1];  /* entries */
} vsa_grid_plan;

int vsa_grid_encode_fwd(const vsa_grid_plan* plan, const float* tables, const float* x,
                        int nr_points, float* out, void* stream);
/* grad_tables (fp32, same shape as tables) += transpose-interpolation of g_out. */
int vsa_grid_encode_bwd(const vsa_grid_plan* plan, const float* x, const float* g_out,
                        int nr_points, float* grad_tables, void* stream);
/* The same gradients for LARGE batches without memory-side atomics: workgroups own (level, 2^14-entry
 * slice) fixed-point accumulators in LDS and scan the samples (csrc/grid_encode.hip).  workspace:
 * nr_points * 2 * n_levels + 32 floats (the output gradient re-laid level-major + max|g| per level). */
int vsa_grid_encode_bwd_sliced(const vsa_grid_plan* plan, const float* x, const float* g_out,
                               int nr_points, float* grad_tables, float* workspace, void* stream);
/* The same gradients for VERY large batches: the 2^D x n_levels contributions of every sample are
 * binned by (level, 2^13-entry slice) once (LDS counting sort, contiguous runs) and each bin is
 * accumulated densely in LDS fixed point.  workspace: vsa_grid_encode_bwd_binned_workspace floats
 * (~14 x 2^D x n_levels x nr_points bytes: 4.8 GB for 2.1 M samples). */
int vsa_grid_encode_bwd_binned_workspace(const vsa_grid_plan* plan, int nr_points,
                                         long long* workspace_floats);
int vsa_grid_encode_bwd_binned(const vsa_grid_plan* plan, const float* x, const float* g_out,
                               int nr_points, float* grad_tables, float* workspace, void* stream);
/* The same four with a row stride (floats) on out / g_out, for callers that keep the features
 * inside a wider row: GridHashEncoder's `torch.cat([enc, points], 1)` (gridhash.py:88-90) becomes
 * out_stride = 2 * n_levels + n_dims with append_x = 1 (the kernel writes x behind the features),
 * and the gradient of that matrix is read in place (g_stride; the x columns are ignored: positions
 * carry no gradient on this path). */
int vsa_grid_encode_fwd_ld(const vsa_grid_plan* plan, const float* tables, const float* x,
                           int nr_points, float* out, int out_stride, int append_x, void* stream);
int vsa_grid_encode_bwd_ld(const vsa_grid_plan* plan, const float* x, const float* g_out,
                           int g_stride, int nr_points, float* grad_tables, void* stream);
int vsa_grid_encode_bwd_sliced_ld(const vsa_grid_plan* plan, const float* x, const float* g_out,
                                  int g_stride, int nr_points, float* grad_tables, float* workspace,
                                  void* stream);
int vsa_grid_encode_bwd_binned_ld(const vsa_grid_plan* plan, const float* x, const float* g_out,
                                  int g_stride, int nr_points, float* grad_tables, float* workspace,
                                  void* stream);
/* out [nr_dirs][(degree+1)^2]: SH basis of each direction, degree 0..4. */
int vsa_sh_encode(const float* dirs, int nr_dirs, int degree, float* out, void* stream);

/* A10  The elementwise glue between NerfHash's two MLPs (volsurfs_py/models/nerfhash.py:72-91), one
 * pass each way instead of eleven torch launches over [samples, 64..80] floats:
 *   fwd: density [n] = softplus(y1[:, 0]);  x2 [n][nr_feat + nr_dir] = cat(gelu(y1[:, 1:1+nr_feat]), dirs_enc)
 *   bwd: dy1 [n][1 + nr_feat] from dx2 (gradient of x2; its dirs columns are ignored) and d_density
 *        (either may be NULL = zero).
 * y1 [n][y1_stride >= 1 + nr_feat] is the first MLP's output (r6: a row stride, so that the rows can be padded to a
 * multiple of 4 floats — the MLP kernels then move them as 16-byte accesses), dy1 has the same stride and its padding
 * columns are written as zeros; dirs_enc [n][nr_dir] the encoded directions. */
int vsa_field_head_fwd(const float* y1, int y1_stride, const float* dirs_enc, long long nr_points, int nr_feat,
                       int nr_dir, float* x2, float* density, void* stream);
int vsa_field_head_bwd(const float* y1, int y1_stride, const float* dx2, const float* d_density, long long nr_points,
                       int nr_feat, int nr_dir, float* dy1, void* stream);

/* A5 / A10  Fused fp32 MLP (Linear + bias, exact GELU between layers, last layer linear) on the
 * fp32-input matrix cores: `MLP` (volsurfs_py/models/mlp.py:8-69) as used by RGB (models/rgb.py:139),
 * ColorSH (models/color_sh.py) and NerfHash (models/nerfhash.py:44-56).  Layer l maps dims[l] ->
 * dims[l+1] with w[l] [dims[l+1]][dims[l]] row-major (torch.nn.Linear.weight) and b[l] [dims[l+1]]
 * or NULL; every width <= 128, hidden widths multiples of 32.  All pointers are device pointers.
 *   vsa_mlp_workspace: sizes (floats) of packed_ws (weights in MFMA fragment order, rewritten by
 *     every call), of each of z_ws / a_ws / dz_ws (nr_points x sum of hidden widths) and of
 *     partial_ws (per-workgroup weight-gradient blocks).
 *   vsa_mlp_fwd: y [nr_points][y_stride] = MLP(x [nr_points][x_stride]); z_ws receives the hidden
 *     pre-activations (NULL: inference), a_ws the activations GELU(z) when the backward of this network is
 *     the two-kernel one (vsa_mlp_bwd_needs_act() == 1; otherwise pass NULL: nothing is stored).
 *   vsa_mlp_bwd: from dy = dL/dy and the z_ws (/ a_ws) of the matching forward: dx (optional), and
 *     grads->dw[l] / db[l] (NULL entries are skipped): overwritten, or added to what the buffers
 *     hold when grads->accumulate != 0 (a caller that owns persistent .grad buffers lets the
 *     kernel add into them instead of running one accumulation kernel per parameter).
 *     Networks up to 96 wide whose weights fit the LDS (NerfHash's two, models/nerfhash.py:44-56) take ONE fused
 *     persistent launch — data gradients, weight gradients and bias sums from z alone (GELU and GELU' from one
 *     evaluation), nothing but dx written per sample (csrc/mlp_f32_fused.h): a_ws and dz_ws are then not read and
 *     may be NULL.  It needs 16-byte rows: x, dy (and dx) 16-byte aligned with a stride that is a multiple of 4 floats
 *     (pad the rows: the padding columns of x are ignored, those of dx receive zeros).  Wider networks (RGB / ColorSH:
 *     128) and unaligned rows run mlp_dgrad + mlp_wgrad as before.  Every kernel moves x / y / dy rows as 16-byte
 *     groups when their stride allows it and element by element otherwise.
 *   vsa_mlp_bwd_needs_act(plan, x_stride, dx_stride (0: no dx)): 1 if vsa_mlp_bwd of this plan with rows of these
 *     strides (bases 16-byte aligned) reads a_ws / dz_ws, 0 if not, < 0: VSA_ERR_*. */
#define VSA_MLP_MAX_LAYERS 6
typedef struct vsa_mlp_plan {
  int32_t n_layers;
  int32_t dims[VSA_MLP_MAX_LAYERS + 1];
  const float* w[VSA_MLP_MAX_LAYERS];
  const float* b[VSA_MLP_MAX_LAYERS];
} vsa_mlp_plan;
typedef struct vsa_mlp_grads {
  float* dw[VSA_MLP_MAX_LAYERS];
  float* db[VSA_MLP_MAX_LAYERS];
  int32_t accumulate; /* 0: dw / db are overwritten, else added to */
} vsa_mlp_grads;

int vsa_mlp_workspace(const vsa_mlp_plan* plan, long long nr_points, long long* packed_floats,
                      long long* act_floats, long long* partial_floats);
int vsa_mlp_bwd_needs_act(const vsa_mlp_plan* plan, int x_stride, int dx_stride);
int vsa_mlp_fwd(const vsa_mlp_plan* plan, const float* x, int x_stride, int nr_points, float* y,
                int y_stride, float* z_ws, float* a_ws, float* packed_ws, void* stream);
int vsa_mlp_bwd(const vsa_mlp_plan* plan, const float* x, int x_stride, int nr_points,
                const float* dy, int dy_stride, const float* z_ws, float* dz_ws, const float* a_ws,
                float* packed_ws, float* partial_ws, float* dx, int dx_stride,
                const vsa_mlp_grads* grads, void* stream);

/* The same two for up to 8 networks of ONE architecture in one set of launches: the K per-shell
 * models of the legacy appearance branch (volsurfs_py/methods/volsurfs.py:402-470), each applied to
 * its own shell's hits.  Group g owns rows [sum nr_points[0..g), +nr_points[g]) of x / y / dy / dx
 * and the matching rows x (sum of hidden widths) floats of z_ws / dz_ws / a_ws; packed_ws holds
 * nr_groups x packed_floats, partial_ws nr_groups x the partial_floats vsa_mlp_workspace reports
 * for the largest group; grads [nr_groups] (one `accumulate` setting for all).  plans / nr_points /
 * grads are HOST arrays.  vsa_mlp_fwd / vsa_mlp_bwd are the one-group case. */
int vsa_mlp_fwd_grouped(const vsa_mlp_plan* plans, int nr_groups, const int* nr_points,
                        const float* x, int x_stride, float* y, int y_stride, float* z_ws,
                        float* a_ws, float* packed_ws, float* packed_bwd_ws, void* stream);
/* packed_bwd_ws (optional, as large as packed_ws): the forward's packing launch also writes the
 * transposed fragment order the backward needs; handed to vsa_mlp_bwd_grouped as packed_ws with
 * packed_ready = 1 (the weights must not have changed in between) it saves that pass its own. */
int vsa_mlp_bwd_grouped(const vsa_mlp_plan* plans, int nr_groups, const int* nr_points,
                        const float* x, int x_stride, const float* dy, int dy_stride,
                        const float* z_ws, float* dz_ws, const float* a_ws, float* packed_ws,
                        int packed_ready, float* partial_ws, float* dx, int dx_stride,
                        const vsa_mlp_grads* grads, void* stream);

/* A13  Fused multi-tensor Adam step: apex.optimizers.FusedAdam(betas (0.9, 0.99), eps 1e-15,
 * weight_decay 0) of volsurfs_py/methods/base_method.py:87-94, stepped at trainer.py:278 (the
 * same update as torch.optim.Adam).  One launch for all parameter tensors:
 *   tensors_dev [T] descriptors in DEVICE memory (param / grad / exp_avg / exp_avg_sq: fp32, n
 *   elements, 16-byte aligned; param_f16: optional f16 compute copy refreshed from the new
 *   parameter, or NULL);  chunks_dev [nr_chunks][2] int32 in device memory = (tensor index,
 *   chunk index within the tensor), one workgroup per chunk of vsa_adam_chunk_elems() elements.
 *   step = 1 for the first update (bias correction 1 - beta^step); grad_scale multiplies the
 *   gradient as it is read (1 = as is); zero_grads != 0 clears the gradient after reading it
 *   (the next iteration's zero_grad, trainer.py:118). */
typedef struct vsa_adam_tensor {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  void* param_f16; /* _Float16* or NULL */
  int64_t n;
} vsa_adam_tensor;

int vsa_adam_chunk_elems(void);
int vsa_adam_step(const vsa_adam_tensor* tensors_dev, const int32_t* chunks_dev, int nr_chunks,
                  float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                  int zero_grads, void* stream);
/* The same update from at most max_workgroups workgroups (256 threads each) that stride over the chunks
 * (0: one workgroup per chunk = vsa_adam_step).  One workgroup per chunk queues thousands of workgroups that
 * take every wave slot of the chip until the update drains; a bounded grid leaves room on every CU for
 * the kernels of ANOTHER stream — the next iteration's ray batch, traversal and texel compaction, which
 * read no parameter (optim.FusedAdam.step(stream=...)). */
int vsa_adam_step_shared(const vsa_adam_tensor* tensors_dev, const int32_t* chunks_dev, int nr_chunks,
                         float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                         int zero_grads, int max_workgroups, void* stream);

/* The glue of the legacy appearance branch around its encoders and MLPs, one launch each way (csrc/legacy_glue.hip;
 * volsurfs.py:486-599; as torch expressions: 18 + 21 launches per training iteration of BASELINE configs[2]).
 *   hit_shell / hit_ray [nr_hits] i64 = shell and ray of every hit, sorted by shell then ray (the two columns of
 *   torch.nonzero(hit_slot >= 0), which torch lays out column by column).
 * vsa_legacy_hit_prep: pts = rays_o + hit_t * rays_d (:507), dirs = rays_d of the hit's ray, normals =
 *   normalize(cross(e1, e2)) of the hit triangle (tris as vsa_bvh_export; F.normalize's 1e-12 floor); [nr_hits,3] each.
 * vsa_legacy_shade_out_fwd: into surfs_rgb [N,K,3] / surfs_alpha [N,K] / surfs_normals [N,K,3] — ZEROED by the caller
 *   (entries where nothing was hit keep that zero, volsurfs.py:486-490; one fill of one allocation in the mirror) — at
 *   every hit: sigmoid(y_rgb[i][0..3)) (row stride ld_rgb >= 3), the hit's normal, and alpha = 1 for rows < alpha_first_row
 *   (a solid inner shell) or when y_alpha is NULL, else sigmoid(y_alpha[i - alpha_first_row][0]) times, if
 *   with_alpha_decay, 2 sigmoid(10 clamp(-d.n, 0, 1)) - 1 (:585-594).  sig_rgb [nr_hits,3], sig_alpha / decay
 *   [nr_hits - alpha_first_row]: what the backward needs.
 * vsa_legacy_shade_out_bwd: dy_rgb / dy_alpha (same strides; channels beyond the used ones zeroed) from the gradients
 *   of the dense arrays: g * s (1 - s), the alpha one through the decay. */
int vsa_legacy_hit_prep(const float* rays_o, const float* rays_d, const float* hit_t, const int32_t* hit_slot,
                        const float* tris, const int64_t* hit_shell, const int64_t* hit_ray, int nr_hits, int nr_rays,
                        float* pts, float* dirs, float* normals, void* stream);
int vsa_legacy_shade_out_fwd(const float* y_rgb, int ld_rgb, const float* y_alpha, int ld_alpha, int alpha_first_row,
                             const int64_t* hit_shell, const int64_t* hit_ray, const float* dirs, const float* normals,
                             int nr_hits, int nr_rays,
                             int nr_shells, int with_alpha_decay, float* surfs_rgb, float* surfs_alpha,
                             float* surfs_normals, float* sig_rgb, float* sig_alpha, float* decay, void* stream);
int vsa_legacy_shade_out_bwd(const float* g_surfs_rgb, const float* g_surfs_alpha, const int64_t* hit_shell,
                             const int64_t* hit_ray, const float* sig_rgb, const float* sig_alpha, const float* decay, int nr_hits, int nr_shells,
                             int alpha_first_row, float* dy_rgb, int ld_rgb, float* dy_alpha, int ld_alpha, void* stream);

/* A5  Permutohedral-lattice hash encoding: `PermutoHashEncoder`
 * (volsurfs_py/encodings/permutohash.py:28-37, 68-96) = permutohedral_encoding.PermutoEncoding
 * (un-vendored fork, .gitmodules:7-9; published algorithm restated, parity unpinned).
 * lattice_values [n_levels][capacity][2] f32; x [N][pos_dim] f32 (the wrapper maps the bounding
 * box to [0,1] first); window [n_levels] f32 (Coarse2Fine) or NULL (= ones);
 * out[b*out_stride + 2*l + f] (out_stride >= 2*n_levels, even: the caller may own a wider row
 * that also holds the concatenated points).  scale_factor[l][i] = 1 / (sigma_l * sqrt((i+1)(i+2))),
 * sigma_l = the level's scale (np.geomspace(coarsest, finest, n_levels), permutohash.py:27). */
typedef struct vsa_permuto_plan {
  int32_t pos_dim;     /* 2..4 */
  int32_t n_levels;    /* <= VSA_GRID_MAX_LEVELS */
  int32_t n_features;  /* 2 */
  int32_t capacity;    /* entries per level (2^18) */
  float scale_factor[VSA_GRID_MAX_LEVELS][4];
  float random_shift[VSA_GRID_MAX_LEVELS][4];
} vsa_permuto_plan;

int vsa_permuto_encode_fwd(const vsa_permuto_plan* plan, const float* lattice_values,
                           const float* x, const float* window, int nr_points, float* out,
                           int out_stride, void* stream);
/* grad_values (fp32, same shape as lattice_values) += transpose of the interpolation applied to
 * g_out[b*g_stride + 2*l + f].  Positions carry no gradient on this path (hit points). */
int vsa_permuto_encode_bwd(const vsa_permuto_plan* plan, const float* x, const float* window,
                           const float* g_out, int g_stride, int nr_points, float* grad_values,
                           void* stream);

/* Up to 8 encodings of one geometry (the position encoders of the K per-shell models,
 * volsurfs_py/methods/volsurfs.py:402-470) in one launch each way: group g owns the rows after the
 * first g groups' in x / out / g_out.  plan_host: group 0's plan (levels, dimension, capacity are
 * shared); plans_dev: the nr_groups plans in DEVICE memory (the per-level shifts may differ);
 * lattice_values / grad_values: HOST arrays of nr_groups device pointers; nr_points: host [nr_groups]. */
int vsa_permuto_encode_fwd_grouped(const vsa_permuto_plan* plan_host, const vsa_permuto_plan* plans_dev,
                                   const float* const* lattice_values, int nr_groups,
                                   const int* nr_points, const float* x, const float* window,
                                   float* out, int out_stride, void* stream);
int vsa_permuto_encode_bwd_grouped(const vsa_permuto_plan* plan_host, const vsa_permuto_plan* plans_dev,
                                   int nr_groups, const int* nr_points, const float* x,
                                   const float* window, const float* g_out, int g_stride,
                                   float* const* grad_values, void* stream);

/* ------------------------------------------------------------------------
 * A8 / A9 / A11  Packed (ragged) per-ray sample ops of the background path:
 * what render_contracted_bg (volsurfs_py/utils/background.py:31-141) calls in the
 * reference's pybind module `volsurfs` (src/PyBridge.cxx:70-138).  A pack is the
 * SoA of include/volsurfs/RaySamplesPacked.cuh:7-80; here its tensors are passed
 * individually: ray_start_end_idx [N,2] i32, per-sample [S,*] f32, per-ray [N,*] f32.
 * A ray is owned by a 32-lane half-wave (lanes = consecutive samples).
 */
/* VolumeRendering::cumprod_one_minus_alpha_to_transmittance (src/VolumeRendering.cu:30-78):
 * T_i = prod_{j<i} a_j, bg_T = T_{n-1}; caller pre-fills T with 0 and bg_T with 1. */
int vsa_packed_cumprod_fwd(const int32_t* start_end, const float* one_minus_alpha,
                           float* transmittance, float* bg_transmittance, int nr_rays,
                           void* stream);
/* ..._backward (:671-718): g_a_i = (cumsumLV_{i+1} + g_bgT*bgT)/max(a_i,1e-6), 0 for the last. */
int vsa_packed_cumprod_bwd(const int32_t* start_end, const float* g_bg_transmittance,
                           const float* one_minus_alpha, const float* bg_transmittance,
                           const float* cumsum_lv, float* g_one_minus_alpha, int nr_rays,
                           void* stream);
/* VolumeRendering::cumsum_over_rays (:326-370), inverse = suffix sums. */
int vsa_packed_cumsum(const int32_t* start_end, const float* values, int inverse, float* out,
                      int nr_rays, void* stream);
/* integrate_with_weights_{1d,3d} (:80-176) and their backward (:720-818); dim in {1,3};
 * bug_compat=1 reproduces VolumeRenderingGPU.cuh:1021 (z lane reads column 1). */
int vsa_packed_integrate_fwd(const int32_t* start_end, const float* values, const float* weights,
                             float* out, int nr_rays, int dim, void* stream);
int vsa_packed_integrate_bwd(const int32_t* start_end, const float* g_out, const float* values,
                             const float* weights, float* g_values, float* g_weights,
                             int nr_rays, int dim, int bug_compat, void* stream);
/* The background composite of render_contracted_bg (volsurfs_py/utils/background.py:93-111) as one
 * launch each way: alpha = 1 - exp(-density dt), T = cumprod_one_minus_alpha_to_transmittance(
 * (1 - alpha) + 1e-6) (VolumeRenderingGPU.cuh:28-78), w = alpha T, pred_rgb =
 * integrate_with_weights_3d(rgb, w) (:127-177); backward = integrate_with_weights_3d_backward
 * (:987-1033, bug_compat as above), the suffix sums of cumsum_over_rays(inverse) (:305-361) and
 * cumprod_..._backward (:896-943) with a zero bg-transmittance gradient.  Bit-identical to the chain
 * of the single ops above.  density, dt: [S] (or [S,1]); rgb, g_rgb: [S,3]; weights (optional out,
 * what median_depth_over_rays takes): [S]; scratch: 2 S floats. */
int vsa_packed_composite_fwd(const int32_t* start_end, const float* density, const float* dt,
                             const float* rgb, float* pred_rgb, float* weights, int nr_rays,
                             void* stream);
int vsa_packed_composite_bwd(const int32_t* start_end, const float* density, const float* dt,
                             const float* rgb, const float* g_pred_rgb, float* g_rgb,
                             float* g_density, float* scratch, int nr_rays, int bug_compat,
                             void* stream);
/* NeRF's foreground render (volsurfs_py/methods/nerf.py render_fg_volumetric and the bg blend of
 * render_rays) as one launch each way (csrc/nerf_render.hip states the summation orders).  Forward:
 * alpha = 1 - exp(-density dt), T = cumprod((1 - alpha) + 1e-6), w = alpha T; rgb_fg [N,3] =
 * integrate_with_weights_3d(rgb, w), weights_sum [N] = sum_over_rays(w), depth [N] =
 * integrate_with_weights_1d(samples_z, w); with rgb_bg (NULL: none) rgb_out [N,3] = rgb_fg +
 * (1 - weights_sum) rgb_bg, where rgb_bg is [N,3] (bg_per_ray = 1) or one colour [3] (0); weights
 * [S] is optional.  Backward: g_rgb [N,3] (the gradient of rgb_out, or of rgb_fg without a
 * background), g_weights_sum [N] or NULL -> g_density [S], g_rgb_samples [S,3], g_rgb_bg [N,3]
 * (optional; needs rgb_bg and the forward's weights_sum); bug_compat as in
 * vsa_packed_integrate_bwd; scratch: 2 S floats.  Bit-identical to the chain of the single ops
 * above (cumprod, integrate_3d, sum_over_rays and their backward).  The per-sample arrays may be NULL
 * when the pack has no samples. */
int vsa_nerf_composite_fwd(const int32_t* start_end, const float* density, const float* dt,
                           const float* samples_z, const float* rgb, const float* rgb_bg, int bg_per_ray,
                           float* rgb_fg, float* rgb_out, float* weights_sum, float* depth, float* weights,
                           int nr_rays, void* stream);
int vsa_nerf_composite_bwd(const int32_t* start_end, const float* density, const float* dt,
                           const float* rgb, const float* rgb_bg, int bg_per_ray, const float* weights_sum,
                           const float* g_rgb, const float* g_weights_sum, float* g_density,
                           float* g_rgb_samples, float* g_rgb_bg, float* scratch, int nr_rays,
                           int bug_compat, void* stream);
/* importance_sampling_nerf (volsurfs_py/utils/nerf_utils.py:61-82) from the uniform samples'
 * densities [S] and dt [S] to cdf [S]: clamped alpha, the cumprod with +1e-6, w = alpha T,
 * w / max(sum_over_rays(w), 1e-6), compute_cdf.  Bit-identical to that chain of single ops. */
int vsa_nerf_coarse_cdf(const int32_t* start_end, const float* density, const float* dt, float* cdf,
                        int nr_rays, void* stream);
/* The Surf method's foreground render (volsurfs_py/methods/surf.py render_fg_volumetric with
 * VolumeRenderingNeuS, and the bg blend of render_rays) as one launch each way (csrc/surf_render.hip
 * states the summation orders).  Forward: the NeuS alpha of compute_alphas_from_logistic_beta from
 * sdf [S], sdf_grad [S,3], dirs [S,3] and dt [S] with the scalars cos_anneal_ratio and logistic_beta,
 * T = cumprod((1 - alpha) + 1e-6), w = alpha T; rgb_fg [N,3] = integrate_with_weights_3d(rgb, w),
 * weights_sum [N] = sum_over_rays(w), depth [N] = integrate_with_weights_1d(samples_z, w),
 * normals_out [N,3] = integrate_with_weights_3d(normals, w); with rgb_bg (NULL: none) rgb_out [N,3]
 * = rgb_fg + (1 - weights_sum) rgb_bg, rgb_bg [N,3] (bg_per_ray = 1) or one colour [3] (0); weights
 * [S] and alpha [S] are optional.  Backward: g_rgb [N,3] (of rgb_out, or of rgb_fg without a
 * background), g_weights_sum [N] or NULL -> g_sdf [S], g_sdf_grad [S,3], g_rgb_samples [S,3],
 * g_rgb_bg [N,3] (optional; needs rgb_bg and the forward's weights_sum); depth and normals pass no
 * gradient; bug_compat as in vsa_packed_integrate_bwd; scratch: 2 S floats.  The per-sample arrays
 * may be NULL when the pack has no samples. */
int vsa_neus_composite_fwd(const int32_t* start_end, const float* sdf, const float* sdf_grad,
                           const float* dirs, const float* dt, const float* samples_z,
                           const float* normals, const float* rgb, const float* rgb_bg, int bg_per_ray,
                           double cos_anneal_ratio, double logistic_beta, float* rgb_fg, float* rgb_out,
                           float* weights_sum, float* depth, float* normals_out, float* weights,
                           float* alpha, int nr_rays, void* stream);
int vsa_neus_composite_bwd(const int32_t* start_end, const float* sdf, const float* sdf_grad,
                           const float* dirs, const float* dt, const float* rgb, const float* rgb_bg,
                           int bg_per_ray, double cos_anneal_ratio, double logistic_beta,
                           const float* weights_sum, const float* g_rgb, const float* g_weights_sum,
                           float* g_sdf, float* g_sdf_grad, float* g_rgb_samples, float* g_rgb_bg,
                           float* scratch, int nr_rays, int bug_compat, void* stream);
/* One round of importance_sampling_sdf (volsurfs_py/utils/sdf_utils.py:87-109, :153-175) from the
 * pack's sdf [S] and dt [S] to cdf [S]: sdf2alpha with the scalar logistic_beta (the caller passes
 * beta / 2 or beta), the cumprod with +1e-6, w = alpha T, w / max(sum_over_rays(w), 1e-6),
 * compute_cdf.  Bit-identical to that chain of single ops. */
int vsa_sdf_coarse_cdf(const int32_t* start_end, const float* sdf, const float* dt, float logistic_beta,
                       float* cdf, int nr_rays, void* stream);
/* The OffsetsSurfs method's foreground render (volsurfs_py/methods/offsets_surfs.py render_fg_volumetric,
 * and the bg blend of render_rays) as one launch each way (csrc/offsets_render.hip states the summation
 * orders).  K = nr_surfs in 1..16 (VSA_ERR_UNSUPPORTED otherwise); per-sample arrays are [S, K] sample-major,
 * column k the k-th surface inner to outer.  Forward, per surface: the NeuS alpha of vsa_neus_composite_fwd
 * from sdfs [S,K], sdfs_grad [S,K,3], dirs [S,3], dt [S]; T = cumprod((1 - alpha) + 1e-6), w = alpha T;
 * surfs_rgb [N,K,3] = integral of rgb [S,K,3], surfs_alpha [N,K] = integral of transparency [S,K] (times
 * sigmoid(f clamp(-d.n, 0, 1)) 2 - 1 with f = alpha_decay_factor when with_alpha_decay, n = normals [S,K,3]),
 * surfs_depths [N,K], surfs_normals [N,K,3], surfs_weight_sum [N,K].  Then the blend outer to inner:
 * surfs_transmittance [N,K], surfs_blending_weights [N,K], rgb_fg [N,3], bg_transmittance [N] and rgb_out
 * [N,3] = rgb_fg + rgb_bg bg_transmittance (rgb_bg NULL: rgb_fg; [N,3] with bg_per_ray = 1 or one colour);
 * alpha [S,K], the per-sample NeuS alpha, is optional.
 * Backward: g_rgb [N,3] of rgb_out -> g_sdfs [S,K], g_sdfs_grad [S,K,3], g_rgb_samples [S,K,3],
 * g_transparency [S,K], g_rgb_bg [N,3] (optional); depths, normals and weight sums pass no gradient, nor does
 * the decay; bug_compat as in vsa_packed_integrate_bwd; scratch: 2 S K floats.  The per-sample arrays may be
 * NULL when the pack has no samples. */
int vsa_offsets_composite_fwd(const int32_t* start_end, int nr_surfs, const float* sdfs, const float* sdfs_grad,
                              const float* normals, const float* rgb, const float* transparency, const float* dirs,
                              const float* dt, const float* samples_z, const float* rgb_bg, int bg_per_ray,
                              double cos_anneal_ratio, double logistic_beta, int with_alpha_decay,
                              double alpha_decay_factor, float* surfs_rgb, float* surfs_normals, float* surfs_depths,
                              float* surfs_weight_sum, float* surfs_alpha, float* surfs_transmittance,
                              float* surfs_blending_weights, float* rgb_fg, float* bg_transmittance, float* rgb_out,
                              float* alpha, int nr_rays, void* stream);
int vsa_offsets_composite_bwd(const int32_t* start_end, int nr_surfs, const float* sdfs, const float* sdfs_grad,
                              const float* normals, const float* rgb, const float* transparency, const float* dirs,
                              const float* dt, const float* rgb_bg, int bg_per_ray, double cos_anneal_ratio,
                              double logistic_beta, int with_alpha_decay, double alpha_decay_factor,
                              const float* surfs_rgb, const float* surfs_alpha, const float* surfs_transmittance,
                              const float* bg_transmittance, const float* g_rgb, float* g_sdfs, float* g_sdfs_grad,
                              float* g_rgb_samples, float* g_transparency, float* g_rgb_bg, float* scratch,
                              int nr_rays, int bug_compat, void* stream);
/* One round of importance_sampling_sdfs_iter (volsurfs_py/utils/sdfs_utils.py:12-64) from the pack's sdfs
 * [S,K] and dt [S] to cdf [S]: per surface the round of vsa_sdf_coarse_cdf with the transmittance clipped to
 * [0, 1], the K CDFs summed in order and divided by K.  Bit-identical to that chain of single ops.  K in
 * 1..16 (VSA_ERR_UNSUPPORTED otherwise). */
int vsa_sdfs_coarse_cdf(const int32_t* start_end, int nr_surfs, const float* sdfs, const float* dt,
                        float logistic_beta, float* cdf, int nr_rays, void* stream);
/* median_depth_over_rays (:372-416); fallback_compat=1 reproduces VolumeRenderingGPU.cuh:407. */
int vsa_packed_median_depth(const int32_t* start_end, const float* samples_z,
                            const float* weights, float threshold, float* out, int nr_rays,
                            int fallback_compat, void* stream);
/* RaySamplesPacked::update_dt (src/RaySamplesPacked.cu:396-461). */
int vsa_packed_update_dt(const int32_t* start_end, const float* ray_max_dt, const float* ray_exit,
                         const float* samples_z, int is_background, float* samples_dt,
                         int nr_rays, void* stream);
/* RaySampler::compute_samples_bg (src/RaySampler.cu:70-156): n samples per ray at
 * t = t_start + 1/(s+1e-6) - 1, s: 1 -> 0; jitter uses PCG32 (state, inc) exactly as the
 * reference's by-value copy of m_rng (advance(ray) before every draw). */
int vsa_sample_bg(const float* rays_o, const float* rays_d, const float* ray_t_start,
                  float ray_t_far, int nr_samples_per_ray, int jitter, uint64_t rng_state,
                  uint64_t rng_inc, float* ray_max_dt, float* samples_3d, float* samples_dirs,
                  float* samples_z, int32_t* ray_start_end_idx, int nr_rays, void* stream);
/* RaySampler::contract_samples kernel (src/RaySampler.cu:336-381; update_dt is a separate call). */
int vsa_contract_samples(const float* ray_o, const int32_t* start_end, const float* samples_3d,
                         const float* samples_z, float* out_samples_3d, float* out_samples_z,
                         int nr_rays, void* stream);

/* Ops of the sibling methods reached through the same pybind module.
 * VolumeRendering::sum_over_rays (src/VolumeRendering.cu:231-324): values [S,dim], dim in
 * {1,2,3,32} -> sum_per_ray [N,dim] and the same sum repeated per sample [S,dim]; backward
 * g_values = g_sum_per_ray[ray] + g_sum_per_sample (kernels/volsurfs/VolumeRenderingGPU.cuh:1036-1077). */
int vsa_packed_sum_over_rays(const int32_t* start_end, const float* values, float* sum_per_ray,
                             float* sum_per_sample, int nr_rays, int dim, void* stream);
int vsa_packed_sum_over_rays_bwd(const int32_t* start_end, const float* g_sum_per_ray,
                                 const float* g_sum_per_sample, float* g_values, int nr_rays,
                                 int dim, void* stream);
/* VolumeRendering::sdf2alpha (src/VolumeRendering.cu:178-229): alpha [S,1] (zero-initialised by
 * the caller; the last sample of a ray is not written) from samples_dt, samples_sdf and the
 * per-sample logistic beta. */
int vsa_packed_sdf2alpha(const int32_t* start_end, const float* samples_dt, const float* samples_sdf,
                         const float* logistic_beta, float* alpha, int nr_rays, void* stream);
/* VolumeRendering::compute_cdf (src/VolumeRendering.cu:418-465): cdf [S,1], zero-initialised by
 * the caller. */
int vsa_packed_compute_cdf(const int32_t* start_end, const float* weights, float* cdf, int nr_rays,
                           void* stream);

/* RaySampler::compute_samples_fg (src/RaySampler.cu:158-240, kernels/volsurfs/RaySamplerGPU.cuh:141-270):
 * uniform steps >= min_dist between t_entry and t_exit, at most max_n per ray, rays with fewer
 * than min_n samples get none; ray i writes slots [i*max_n, ...).  Outputs as the
 * RaySamplesPacked fields (caller-initialised to the constructor's values); compact afterwards. */
int vsa_sample_fg(const float* rays_o, const float* rays_d, const float* ray_t_entry,
                  const float* ray_t_exit, float min_dist_between_samples,
                  int min_nr_samples_per_ray, int max_nr_samples_per_ray, int jitter,
                  uint64_t rng_state, uint64_t rng_inc, float* ray_max_dt, int32_t* samples_idx,
                  float* samples_3d, float* samples_dirs, float* samples_z,
                  int32_t* ray_start_end_idx, int nr_rays, void* stream);
/* RaySamplesPacked::compact_to_valid_samples (src/RaySamplesPacked.cu:188-273): out_start [N] =
 * exclusive scan of the per-ray sample counts (caller). */
int vsa_pack_compact(const int32_t* start_end, const int32_t* out_start, const int32_t* samples_idx,
                     const float* samples_3d, const float* samples_dirs, const float* samples_z,
                     const float* samples_dt, const float* samples_values, int values_dim,
                     int32_t* out_idx, float* out_3d, float* out_dirs, float* out_z, float* out_dt,
                     float* out_values, int32_t* out_start_end, int nr_rays, void* stream);
/* VolumeRendering::importance_sample (src/VolumeRendering.cu:467-560): nr_importance_samples new
 * depths per ray by inverting the ray's cdf; ray i writes slots [i*n, (i+1)*n). */
int vsa_importance_sample(const float* rays_o, const float* rays_d, const int32_t* start_end,
                          const float* samples_z, const float* samples_cdf,
                          int nr_importance_samples, int jitter, uint64_t rng_state,
                          uint64_t rng_inc, float* out_3d, float* out_dirs, float* out_z,
                          int32_t* out_start_end, int nr_rays, void* stream);

/* RaySampler::uncontract_samples (src/RaySampler.cu:383-428): inverse of vsa_contract_samples. */
int vsa_uncontract_samples(const float* ray_o, const int32_t* start_end, const float* samples_3d,
                           const float* samples_z, float* out_samples_3d, float* out_samples_z,
                           int nr_rays, void* stream);

/* VolumeRendering::combine_ray_samples_packets (src/VolumeRendering.cu:562-670): depth-ordered
 * merge of two compacted packs over the same rays, dropping samples closer than min_dist to the
 * previous kept one.  out_start [N] = exclusive scan of (count_1 + count_2); compact afterwards. */
int vsa_combine_packs(const int32_t* start_end_1, const int32_t* idx_1, const float* s3d_1,
                      const float* dirs_1, const float* z_1, const float* values_1,
                      const int32_t* start_end_2, const int32_t* idx_2, const float* s3d_2,
                      const float* dirs_2, const float* z_2, const float* values_2,
                      const int32_t* out_start, float min_dist_between_samples, int values_dim,
                      int32_t* out_idx, float* out_3d, float* out_dirs, float* out_z,
                      float* out_values, int32_t* out_start_end, int nr_rays, void* stream);

/* A1  Ray / bounding-primitive intersection: `intersect_bounding_primitive`
 * (volsurfs_py/utils/raycasting.py:4-36) -> mvdatasets BoundingBox / BoundingSphere .intersect
 * (absent: parity unpinned; the primitive is chosen at utils/volsurfs_utils.py:234-272).
 * kind 0 = origin-centred cube of HALF side `size`, kind 1 = origin-centred sphere of radius
 * `size`.  is_hit [N] u8, t_near / t_far [N] (0 on a miss, t_near clamped to >= 0),
 * points_near / points_far [N,3] (optional).  VolSurfs consumes t_far (volsurfs.py:688-693). */
int vsa_intersect_primitive(const float* rays_o, const float* rays_d, int nr_rays, int kind,
                            float size, uint8_t* is_hit, float* t_near, float* t_far,
                            float* points_near, float* points_far, void* stream);

/* ---- ray generation (mvdatasets is an empty submodule: parity unpinned) ----
 * Pinhole rays of one camera, replacing mvdatasets.utils.raycasting.get_camera_rays as called at
 * methods/base_method.py:389-394 and renderers/base_renderer.py:59.  c2w [3,4] and
 * intrinsics_inv [3,3] are DEVICE arrays, row-major.  Ray i = (row * width + col) *
 * nr_rays_per_pixel + s goes through (col + jx, row + jy), (jx, jy) = (0.5, 0.5) or two PCG32
 * draws of the stream (rng_state, rng_inc) advanced by 2 i.  rays_o / rays_d [n,3], points_2d
 * [n,2] (may be NULL). */
int vsa_camera_rays(const float* c2w, const float* intrinsics_inv, int height, int width,
                    int nr_rays_per_pixel, int jitter_pixels, uint64_t rng_state, uint64_t rng_inc,
                    float* rays_o, float* rays_d, float* points_2d, void* stream);

/* Training batch, replacing TensorReel.get_next_rays_batch as called at trainer.py:176-190:
 * batch_size uniformly drawn (camera, pixel) pairs of a resident stack of nr_cameras equally
 * sized views (c2w_all [C,3,4], intrinsics_inv_all [C,3,3], rgb_all [C,H,W,3], mask_all [C,H,W]
 * or NULL), nr_rays_per_pixel rays each.  camera_idx [B], rays_o / rays_d [B*R,3], gt_rgb [B,3]
 * and gt_mask [B] (each may be NULL), points_2d [B*R,2] (may be NULL). */
int vsa_reel_next_rays_batch(const float* c2w_all, const float* intrinsics_inv_all,
                             const float* rgb_all, const float* mask_all, int nr_cameras, int height,
                             int width, int batch_size, int nr_rays_per_pixel, int jitter_pixels,
                             uint64_t rng_state, uint64_t rng_inc, int32_t* camera_idx,
                             float* rays_o, float* rays_d, float* gt_rgb, float* gt_mask,
                             float* points_2d, void* stream);

/* ---- Teacher distillation: virtual hemisphere cameras (trainer.py:132-166, 209-214 of the reference) ----
 * `sample_cameras_on_hemisphere` lives in mvdatasets, an empty submodule: parity unpinned, the rule is this library's
 * own (csrc/hemisphere_camera.h, restated in tests/distill_restated.py), fp32, + - * / sqrt only, in a fixed order:
 *   camera c owns draws [32 c, 32 c + 32) of the call's PCG32 stream (rng_state, rng_inc): up to 16 candidate pairs
 *   (a, b) = (2u - 1, 2v - 1), s = a a + b b; the first with s < 1 and min_height <= |1 - 2s| <= max_height gives the
 *   direction (2a sqrt(1 - s), 2b sqrt(1 - s), |1 - 2s|) / its length, uniform by area over the band of heights; if
 *   all 16 are refused (3e-10 of the cameras at [0, 0.95]): height (min_height + max_height) / 2, azimuth 0.
 *   The third component is along the height axis up_sign * e[up_axis] (up_axis 0..2, up_sign +-1), the first and second
 *   along the axes (up_axis + 1) % 3 and (up_axis + 2) % 3.  The centre is radius * direction; the pose looks at the
 *   origin with the height axis as world up, columns x right, y down, z forward.
 * Refused (VSA_ERR_ARG): radius not positive and finite, min_height < 0, min_height > max_height, max_height >= 1.
 *
 * vsa_hemisphere_cameras: the nr_cameras poses of a stream, c2w_out [C,3,4] (device), one lane per camera. */
int vsa_hemisphere_cameras(int nr_cameras, float radius, int up_axis, int up_sign, float min_height, float max_height,
                           uint64_t rng_state, uint64_t rng_inc, float* c2w_out, void* stream);

/* One training batch from those cameras without a pose table: sample b draws (camera, col, row[, jx, jy]) as
 * vsa_reel_next_rays_batch does, at stream position 32 nr_cameras + b (3 + 2 jitter_pixels), makes that camera's pose in
 * registers and emits ONE ray through (col + jx, row + jy), (jx, jy) = (0.5, 0.5) unjittered.  All cameras share
 * intrinsics_inv [3,3] (device).  camera_idx [B], rays_o / rays_d [B,3], points_2d [B,2] (may be NULL). */
int vsa_virtual_rays_batch(const float* intrinsics_inv, int nr_cameras, int height, int width, float radius,
                           int up_axis, int up_sign, float min_height, float max_height, int batch_size,
                           int jitter_pixels, uint64_t rng_state, uint64_t rng_inc, int32_t* camera_idx,
                           float* rays_o, float* rays_d, float* points_2d, void* stream);

/* The mixed batch [virtual | real] of a distilled iteration in one launch.  Rays 0 .. nr_virtual - 1 are
 * vsa_virtual_rays_batch(batch_size = nr_virtual)'s from the stream (virtual_rng_state, virtual_rng_inc), bit for bit;
 * rays nr_virtual + b R + s are ray b R + s of vsa_reel_next_rays_batch(batch_size = nr_real) from (rng_state, rng_inc),
 * bit for bit.  rays_o / rays_d [nr_virtual + nr_real R, 3]; gt_rgb [same, 3], gt_mask [same] and points_2d [same, 2]
 * may be NULL.  Ground truth is per RAY here: the real half repeats its pixel's colour and mask for each of the R
 * rays (mask 1 where mask_all is NULL); the virtual half's gt_rgb is left unwritten for the teacher, its mask is 1.
 * virtual_camera_idx [nr_virtual], real_camera_idx [nr_real].  Either half may be empty. */
int vsa_distill_rays_batch(const float* virtual_intrinsics_inv, int nr_virtual_cameras, float radius, int up_axis,
                           int up_sign, float min_height, float max_height, int nr_virtual, int jitter_virtual,
                           uint64_t virtual_rng_state, uint64_t virtual_rng_inc, const float* c2w_all,
                           const float* intrinsics_inv_all, const float* rgb_all, const float* mask_all,
                           int nr_cameras, int height, int width, int nr_real, int nr_rays_per_pixel,
                           int jitter_pixels, uint64_t rng_state, uint64_t rng_inc, int32_t* virtual_camera_idx,
                           int32_t* real_camera_idx, float* rays_o, float* rays_d, float* gt_rgb, float* gt_mask,
                           float* points_2d, void* stream);

/* ------------------------------------------------------------------------
 * The training iteration as ONE replayed HIP graph (round 6): device-side control block.
 *
 * The reference's loop (volsurfs_py/trainer.py:118-308) changes four things from one iteration to the next that a
 * launch sequence would carry as kernel ARGUMENTS — the ray count of the dynamic batch (:288-304), the loss
 * normalisation 1 / (3 n), the learning rate of the warm-up + MultiStepLR schedule (:306-308, schedulers/warmup.py,
 * base_method.py:71-76) with Adam's step count, and the sampler's random stream (:176-190) — and reads the hit count
 * back on the host to size the next batch.  Here they live in device memory: every kernel of the iteration runs at
 * a fixed CAPACITY of rays, the `_ctl` entry points read what varies from this block, and a one-lane kernel at the
 * end of the iteration (vsa_train_ctl_tick) applies the reference's rules for the next one.  The iteration is then
 * a static graph: no host read, no host write, no launch gap inside it.
 * Rays beyond nr_rays (up to the capacity) are DUMMY rays: the sampler points them away from the scene (they hit
 * nothing: no texel is marked, nothing is shaded), the composite gives them no gradient, the loss does not count them. */
typedef struct vsa_train_ctl {
  int32_t iter;            /* 0-based number of the iteration that runs next (= times the schedule has been stepped) */
  int32_t nr_rays;         /* active rays of that iteration, 1 .. capacity */
  int32_t capacity;        /* rays every launch is sized for */
  int32_t adam_step;       /* Adam updates applied or pending so far: the pending one's 1-based step count */
  float loss_scale;        /* loss_weight / (3 nr_rays): d mean|gt - pred| / d pred, as trainer.train_step forms it */
  float adam_lr;           /* learning rate of the pending Adam update = lr_at(iteration it belongs to) */
  float loss;              /* mean |gt - pred| of the last finished iteration (vsa_l1_mean_ctl) */
  int32_t clamped;         /* how often the dynamic rule asked for more than `capacity` rays (the host re-captures) */
  uint64_t rng_state, rng_inc;   /* the sampler's PCG32 stream (advanced by 2^32 per iteration, as TensorReel does) */
  int64_t nr_hits;         /* hits of the last finished iteration (vsa_count_hits writes here) */
  int32_t target_hits;     /* target_nr_of_training_samples (0: the ray count stays) */
  int32_t nr_warmup;       /* warm-up iterations of the schedule */
  int32_t nr_milestones;   /* <= 8 */
  int32_t milestone[8];    /* MultiStepLR milestones, sorted */
  float lr_stage[9];       /* (float)(base_lr * gamma^k), k = 0 .. nr_milestones: formed on the host, in double */
  int32_t adam_pending;    /* 1: an iteration has finished whose update vsa_adam_step_ctl has not applied yet (set by the tick) */
  double lr_base;          /* base learning rate (the warm-up ramp is lr_base * (it / nr_warmup) in double, as the host's) */
  double loss_weight;      /* 1 (a data-parallel rank: its share of the global batch) */
  int64_t sum_rays, sum_hits;    /* running totals over the finished iterations (the tick adds; a bench reads the difference) */
} vsa_train_ctl;

/* End of an iteration (stream-ordered behind vsa_count_hits / vsa_l1_mean_ctl of that iteration): the pending Adam
 * update becomes this iteration's (adam_step += 1, adam_lr = lr_at(iter)); nr_rays = int(nr_rays * (target_hits /
 * nr_hits)) (trainer.py:288-304; clamped to 1 .. capacity, counted in `clamped`); loss_scale follows; iter += 1; the
 * random stream advances by 2^32.  One lane. */
int vsa_train_ctl_tick(vsa_train_ctl* ctl, void* stream);

/* vsa_reel_next_rays_batch at a fixed launch size: `capacity` (the host's copy of ctl->capacity: it sizes the grids of
 * the `_ctl` launches) samples are written, the first
 * ctl->nr_rays drawn exactly as vsa_reel_next_rays_batch(batch_size = nr_rays) draws them from (ctl->rng_state,
 * ctl->rng_inc); the rest are dummy rays: origin dummy_o[3], direction dummy_d[3] (host arrays: a ray that misses
 * every shell), gt_rgb = dummy_rgb[3]. */
int vsa_reel_next_rays_batch_ctl(const float* c2w_all, const float* intrinsics_inv_all, const float* rgb_all,
                                 const float* mask_all, int nr_cameras, int height, int width, int capacity,
                                 int nr_rays_per_pixel, int jitter_pixels, const vsa_train_ctl* ctl,
                                 const float* dummy_o, const float* dummy_d, const float* dummy_rgb,
                                 int32_t* camera_idx, float* rays_o, float* rays_d, float* gt_rgb,
                                 float* gt_mask, float* points_2d, void* stream);

/* vsa_composite_dense_fwd_bwd_l1 over ctl->capacity rays with loss_scale = ctl->loss_scale; rays >= ctl->nr_rays get
 * zero gradients (their colour is still written). */
int vsa_composite_dense_fwd_bwd_l1_ctl(const float* surfs_rgb, const float* surfs_alpha, const float* rgb_bg,
                                       int bg_is_broadcast, const float* gt_rgb, const vsa_train_ctl* ctl,
                                       float* out_rgb, float* g_surfs_rgb, float* g_surfs_alpha, int capacity,
                                       int nr_shells, int carry_f16, void* stream);

/* vsa_l1_mean over the first 3 * ctl->nr_rays elements of pred / gt ([capacity, 3]); the mean goes to ctl->loss. */
int vsa_l1_mean_ctl(const float* pred, const float* gt, int capacity, void* scratch, vsa_train_ctl* ctl, void* stream);

/* vsa_adam_step_shared with lr = ctl->adam_lr and step = ctl->adam_step read on the device (the bias corrections
 * are formed there, in double); a launch that finds adam_pending == 0 (the first replay of a loop) does nothing. */
int vsa_adam_step_ctl(const vsa_adam_tensor* tensors_dev, const int32_t* chunks_dev, int nr_chunks, float beta1,
                      float beta2, float eps, float grad_scale, int zero_grads, int max_workgroups,
                      const vsa_train_ctl* ctl, void* stream);

/* Re-orders a row-major per-pixel array [height*width, channels] (channels 1..4, f32) into
 * 8x8-pixel-tile-major order (inverse = 0), or back (inverse = 1).  height and width must be
 * multiples of 8.  Inside a tile the pixels run boustrophedon: element j of a tile is pixel row
 * j/8 and pixel column j%8 on even rows, 7 - j%8 on odd rows, so consecutive elements are always
 * neighbouring pixels.  Used on the rays of a full frame before the traversal (a wave then covers
 * a square patch of pixels instead of a 64x1 strip) and on the rendered colours after it. */
int vsa_tile_order(const float* src, float* dst, int height, int width, int channels, int inverse,
                   void* stream);
/* The same forward re-ordering for the three per-ray inputs of a frame ([H*W,3] each; gt_rgb
 * and gt_rgb_tiled may be NULL) in one launch. */
int vsa_tile_order_rays(const float* rays_o, const float* rays_d, const float* gt_rgb,
                        float* rays_o_tiled, float* rays_d_tiled, float* gt_rgb_tiled, int height,
                        int width, void* stream);

/* ---- OccupancyGrid: include/volsurfs/OccupancyGrid.cuh:9-68 -----------------
 * A cubic grid of nr_voxels_per_dim^3 voxels (a power of two <= 1024) in Morton order, centred on
 * the origin, with side lengths extent_{x,y,z}: grid_values f32 [n^3], grid_occupancy / grid_roi
 * u8 (torch.bool) [n^3].  Kernels: kernels/volsurfs/OccupancyGridGPU.cuh, occ_grid_helpers.h.
 * Every ray marcher is capped at 65536 steps (the reference's loops are unbounded). */

/* get_grid_lower_left_voxels_vertices (centre_of_voxel = 0) / get_grid_samples,
 * get_random_grid_samples(_in_roi) (centre_of_voxel = 1, optional jitter inside the voxel):
 * positions [nr_points,3] of the voxels point_indices (NULL = 0..nr_points-1).
 * OccupancyGridGPU.cuh:31-119. */
int vsa_occ_grid_points(const int32_t* point_indices, int nr_points, int nr_voxels_per_dim,
                        float extent_x, float extent_y, float extent_z, int centre_of_voxel, int jitter,
                        uint64_t rng_state, uint64_t rng_inc, float* out_points, void* stream);
/* update_grid_values: grid[idx] = max(values, grid[idx] * decay).  OccupancyGridGPU.cuh:122-151. */
int vsa_occ_update_values(const int32_t* point_indices, const float* values, int nr_points, float decay,
                          float* grid_values, void* stream);
/* update_grid_occupancy_with_density_values (:153-225): occupied = value > thresh (any of the 27
 * neighbours when check_neighbours). */
int vsa_occ_update_occupancy_density(const int32_t* point_indices, int nr_points, int nr_voxels_per_dim,
                                     float extent_x, float extent_y, float extent_z,
                                     float occupancy_thresh, int check_neighbours,
                                     const float* grid_values, uint8_t* grid_occupancy, void* stream);
/* update_grid_occupancy_with_sdf_values (:229-315): NeuS logistic density of the smallest |sdf|
 * reachable in the voxel > thresh; logistic_beta [nr_points]. */
int vsa_occ_update_occupancy_sdf(const int32_t* point_indices, const float* logistic_beta, int nr_points,
                                 int nr_voxels_per_dim, float extent_x, float extent_y, float extent_z,
                                 float occupancy_thresh, const float* grid_values,
                                 uint8_t* grid_occupancy, void* stream);
/* check_occupancy (:376-413): per point (roi && occupied) and the voxel's value (false / 0 outside). */
int vsa_occ_check(const float* points, int nr_points, int nr_voxels_per_dim, float extent_x,
                  float extent_y, float extent_z, const float* grid_values,
                  const uint8_t* grid_occupancy, const uint8_t* grid_roi, uint8_t* out_occupancy,
                  float* out_values, void* stream);
/* get_rays_t_near_t_far (:318-374). */
int vsa_occ_rays_t_near_t_far(const float* rays_o, const float* rays_d, const float* ray_t_entry,
                              const float* ray_t_exit, int nr_rays, int nr_voxels_per_dim,
                              float extent_x, float extent_y, float extent_z,
                              const uint8_t* grid_occupancy, const uint8_t* grid_roi, float* out_t_near,
                              float* out_t_far, void* stream);
/* get_first_rays_sample_start_of_grid_occupied_regions (:505-581): pack of one sample per ray. */
int vsa_occ_first_sample(const float* rays_o, const float* rays_d, const float* ray_t_entry,
                         const float* ray_t_exit, int nr_rays, int nr_voxels_per_dim, float extent_x,
                         float extent_y, float extent_z, const uint8_t* grid_occupancy,
                         const uint8_t* grid_roi, float* samples_3d, float* samples_dirs,
                         float* samples_z, float* samples_dt, int32_t* ray_start_end_idx, void* stream);
/* advance_ray_sample_to_next_occupied_voxel (:415-503); new_samples_3d may alias samples_3d. */
int vsa_occ_advance_samples(const float* samples_dirs, const float* samples_3d, int nr_points,
                            int nr_voxels_per_dim, float extent_x, float extent_y, float extent_z,
                            const uint8_t* grid_occupancy, const uint8_t* grid_roi,
                            float* new_samples_3d, uint8_t* is_within_bounds, void* stream);
/* RaySampler::compute_samples_fg_in_grid_occupied_regions (src/RaySampler.cu:243-334, kernel
 * RaySamplerGPU.cuh:275-457): equidistant samples in occupied-space arc length; outputs as
 * vsa_sample_fg. */
int vsa_sample_fg_occupied(const float* rays_o, const float* rays_d, const float* ray_t_entry,
                           const float* ray_t_exit, float min_dist_between_samples,
                           int min_nr_samples_per_ray, int max_nr_samples_per_ray, int jitter_samples,
                           uint64_t rng_state, uint64_t rng_inc, int nr_voxels_per_dim, float extent_x,
                           float extent_y, float extent_z, const uint8_t* grid_occupancy,
                           const uint8_t* grid_roi, float* ray_max_dt, int32_t* samples_idx,
                           float* samples_3d, float* samples_dirs, float* samples_z,
                           int32_t* ray_start_end_idx, int nr_rays, void* stream);

/* ------------------------------------------------------------------------
 * Held-out-view evaluation (csrc/image_metrics.hip): per-image PSNR and SSIM of B image pairs of one size, piq
 * 0.8.0's `psnr(x, y, data_range=1.)` and `ssim(x, y, data_range=1.)` with their defaults as the reference calls
 * them (volsurfs_py/utils/evaluation.py:167-168; piq is unpinned here, the definitions are restated in DESIGN §13).
 *   pred, gt      [B,H,W,3] HWC RGB, contiguous, 16-byte aligned; each fp32 (flag 0, values in [0,1]) or uint8
 *                 (flag 1, read as u8 / 255).
 *   pool          SSIM's average-pooling factor f >= 1 (piq: max(1, round(min(H, W) / 256)); 1 = downsample off);
 *                 the pooled image (H / f) x (W / f) must be at least 11 x 11.
 *   quantize_pred 1: the 8-bit rule trunc(clamp(x, 0, 1) * 255) / 255 on an fp32 pred as it is loaded (the PNG
 *                 round trip of rendering.py:15-33 without a PNG); ignored for a uint8 pred.
 *   workspace     vsa_image_metrics_workspace_bytes(...) bytes of device memory, 8-byte aligned; no state is kept
 *                 in it between calls.
 *   psnr_out, ssim_out  [B] f64: -10 log10(mse + 1e-8) over the 3 H W values; the mean SSIM map over channels
 *                 and pixels.  Every sum runs in a fixed order: the same bits every call and for every B.
 * VSA_ERR_ARG (before any HIP call): a NULL pointer, B / H / W < 1, pool < 1, a pooled size under 11, a dtype or
 * quantize flag other than 0 / 1, an unaligned pointer, a workspace smaller than asked for.  VSA_ERR_UNSUPPORTED:
 * a pooled row run of pred + gt that does not fit the kernel's staging area (pool above 18 for two fp32 inputs).
 * The workspace query returns the byte count or one of those two codes.
 */
long long vsa_image_metrics_workspace_bytes(int B, int H, int W, int pool, int pred_u8, int gt_u8);
int vsa_image_metrics(const void* pred, int pred_u8, const void* gt, int gt_u8, int B, int H, int W, int pool,
                      int quantize_pred, void* workspace, long long workspace_bytes, double* psnr_out,
                      double* ssim_out, void* stream);

/* ------------------------------------------------------------------------
 * Marching cubes (csrc/isosurface.hip): the K level sets of one grid, the mesh extraction of the reference's baker
 * (volsurfs_py/baker.py:324-452, utils/mesh_extraction.py:224-373, which runs skimage on the host once per level).
 *   grid          [nx, ny, nz] f32, C-contiguous: value (i, j, k) = f(x_i, y_j, z_k) (indexing "ij"), finite (the
 *                 caller checks: NaN has no inside / outside); grid point (i, j, k) sits at origin + (i, j, k) * spacing.
 *   levels        [host] K f32, 1 <= K <= 16, any order; inside_above 0 / 1.
 * Rules (the output is a function of the grid and the levels only; tests/test_isosurface.py restates them in numpy):
 *   inside        a grid point is inside when value < level (strict), or value > level when inside_above.
 *   vertices      one per crossed grid edge (endpoints differ in inside status), shared by every cell around the
 *                 edge.  With a the edge's lower-index endpoint and b the other, t = (level - f_a) / (f_b - f_a) in
 *                 fp32 (IEEE division, no contraction); along the edge's axis origin + (idx_a + t) * spacing, the
 *                 other two coordinates origin + idx * spacing.  Order: by owning point a in C order, then by axis
 *                 x, y, z.
 *   faces         [F, 3] i32 vertex ids local to the level; order: by cell (i, j, k) in C order, then by table order.
 *                 The table (vsa_mc_table, volsurfs_amd/isosurface.py:build_mc_table) resolves every ambiguous face
 *                 by one rule, so closed surfaces come out watertight; (v1 - v0) x (v2 - v0) points out of the inside
 *                 region (towards increasing value for an SDF: mesh.icosphere's winding).  Zero-area faces (a grid
 *                 value exactly at the level) are kept.
 * Two passes:
 *   vsa_isosurface_count  per-row counts, a device scan into per-row offsets and the per-level totals in the
 *                 workspace, then the 2K totals (V_0, F_0, V_1, F_1, ...) copied to [host] `totals`: the call
 *                 synchronises `stream` once.  VSA_ERR_UNSUPPORTED when a level's V or F reaches 2^31.
 *   vsa_isosurface_emit   with the same grid, levels, flag and workspace right after the count: writes verts[L]
 *                 [V_L, 3] f32 and faces[L] [F_L, 3] i32 ([host] arrays of K device pointers; NULL allowed for an
 *                 empty array), never past the V_L / F_L of `totals`; origin, spacing [host] 3 f32, spacing > 0.
 *   workspace     vsa_isosurface_workspace_bytes(nx, ny, nz, K) bytes: 12 bytes per row (nx * ny) and level plus the
 *                 scan's temporary storage -- O(K nx ny), never O(nx ny nz).
 * VSA_ERR_ARG (before any HIP call): a NULL pointer, a dimension < 2, K outside 1..16, inside_above other than 0 / 1,
 * a spacing <= 0 (or NaN), a workspace smaller than asked for.  VSA_ERR_UNSUPPORTED: nx * ny >= 2^31 rows or
 * nz >= 2^31 / 5.  The workspace query returns the byte count or one of those codes.
 */
long long vsa_isosurface_workspace_bytes(long long nx, long long ny, long long nz, int nr_levels);
int vsa_isosurface_count(const float* grid, long long nx, long long ny, long long nz, const float* levels,
                         int nr_levels, int inside_above, void* workspace, long long workspace_bytes,
                         long long* totals, void* stream);
int vsa_isosurface_emit(const float* grid, long long nx, long long ny, long long nz, const float* levels,
                        int nr_levels, int inside_above, const float* origin, const float* spacing, void* workspace,
                        long long workspace_bytes, const long long* totals, float* const* verts,
                        int32_t* const* faces, void* stream);
/* The marching-cubes triangle table compiled into the library: out [host] 256 x 16 int8 (case c: bit b set when
 * cube corner b = dx | dy << 1 | dz << 2 is inside; up to five triangles of edge ids, -1 padded). */
int vsa_mc_table(int8_t* out);

/* ------------------------------------------------------------------------
 * Mesh simplification (csrc/simplify.hip): parallel Garland-Heckbert quadric edge collapse, in rounds, down to a
 * face count -- the baker's `--simplify_meshes` step (pymeshlab's quadric edge-collapse decimation in the reference,
 * volsurfs_py/baker.py:682-724, utils/mesh_extraction.py:492-537).
 *   verts [V, 3] f32 and faces [F, 3] i32 on the device: finite, indices in [0, V), no index twice in one face (the
 *   caller checks).  V, F >= 1.  target_faces >= 0: the caller's int(F * ratio).
 * Rules (the output is a function of the input mesh and the target only; tests/test_simplify.py restates them in
 * numpy and the kernels are held to it bit for bit; every float operation below is IEEE fp64 unless said, in the
 * order written, with no contraction):
 *   quadrics      face f's plane quadric: n = (p1 - p0) x (p2 - p0), u = n / |n|, d = -(u.p0), Q_f = (|n| / 2) *
 *                 (u, d)(u, d)^T (zero for |n| = 0), stored as the upper triangle xx xy xz xd yy yz yd zz zd dd, each
 *                 entry w * (p_i * p_j).  A boundary edge (one face) c: pi -> pj of face f adds to both its endpoints
 *                 the plane through the edge along n: m = (pj - pi) x n, u = m / |m|, weight 10 |pj - pi|^2 (zero for
 *                 |m| = 0).  Q_v = the sum over the faces at v in ascending face index of Q_f, then the penalties of
 *                 f's boundary edges at v in corner order c = 0, 1, 2 (a sorted (vertex, face) list, no float
 *                 atomics).  Computed once from the input; a collapse of b into a sets Q_a := Q_a + Q_b.
 *   edges         per round, the unique undirected edges of the current faces; id = rank in (min, max) order; the
 *                 edge's face count from the faces.  Boundary vertex: on an edge with one face; frozen: on an edge
 *                 with more than two.  Edge (a, b) has a < b; b collapses into a.
 *   placement     Q = Q_a + Q_b.  Exactly one endpoint on a boundary: that endpoint.  Otherwise the 3x3 system
 *                 [xx xy xz; xy yy yz; xz yz zz] x = -(xd, yd, zd) by cofactors (c00 = yy zz - yz yz, c01 = xz yz -
 *                 xy zz, c02 = xy yz - xz yy, c11 = xx zz - xz xz, c12 = xy xz - xx yz, c22 = xx yy - xy xy, det =
 *                 xx c00 + xy c01 + xz c02, x = (c00 r0 + c01 r1 + c02 r2) / det, ...) when det > 1e-10 tr^3 (tr = xx +
 *                 yy + zz); else the cheapest of a, b and fp32((a + b) * 0.5), ties in that order.  The position is
 *                 rounded to fp32 and the cost evaluated there: t_i = row i of Q . (x, y, z, 1), cost = t0 x + t1 y +
 *                 t2 z + t3.
 *   candidate     an edge is one when all hold: neither endpoint frozen; no pinching (an edge with two faces between
 *                 two boundary vertices); a finite position and a non-NaN cost; the link condition (the number of
 *                 distinct common neighbours of a and b equals the edge's face count); no flip (every face at a or b
 *                 without both, with the moved vertex at the new position: dot(n_before, n_after) > 0, a face with
 *                 n_before = 0 exempt); no duplicated face (no face at a without b equals, as a vertex set, a face at
 *                 b without a with b renamed a -- this also keeps a closed component from shrinking below a
 *                 tetrahedron).
 *   key           (fp32 bits of max(cost, 0) rounded up) << 32 | edge id; UINT64_MAX for a non-candidate.
 *   winners       m1(v) = min key over the edges at v; m2(v) = min m1 over the vertices of the faces at v (64-bit
 *                 atomicMin: a minimum does not depend on arrival order).  (a, b) wins when key == m2(a) == m2(b).
 *                 Two winners share no face and no vertex, and no winner's endpoint lies in another's ring; the global
 *                 minimum always wins.
 *   target        a round accepts winners in ascending key order while the faces still to remove (F - target) are
 *                 positive; each removes the faces that contain both its endpoints.  The loop ends when F <= target
 *                 or a round has no candidate (`stalled`).  So F_out <= target unless stalled, and F_out >= target - 1
 *                 when every accepted edge has at most two faces.
 *   collapse      b is replaced by a in place in every face (winding kept); faces with both are dropped; surviving
 *                 faces keep ascending input order.
 *   output        out_verts: the vertices referenced by a surviving face, in ascending input index; out_faces: the
 *                 surviving faces in ascending input face index, renumbered.  out_verts [V, 3] f32 and out_faces
 *                 [F, 3] i32 are sized for the input; the first V_out / F_out rows are written.
 *   stats         [host] 5 long long: rounds (rounds that collapsed), collapses, stalled (0 / 1), V_out, F_out.
 *   stage_ms      [host] 6 floats or NULL: device ms of init, edges, cost, select, collapse, compact (events, with one
 *                 stream synchronisation per stage; NULL: none).
 * The host reads one small counter pair per round (W, faces removed), and one more in the last round; the call
 * synchronises `stream` before it returns.
 *   workspace     vsa_simplify_workspace_bytes(V, F): 120 bytes per vertex and 156 per face plus rocPRIM's temporary
 *                 storage (its radix sorts of 3F keys) -- O(V + F).
 * VSA_ERR_ARG: a NULL pointer, V or F < 1, target < 0, a workspace smaller than asked for.  VSA_ERR_UNSUPPORTED:
 * V >= 2^31 or 3 F + 3 >= 2^31.  The workspace query returns the byte count or one of those codes.
 */
long long vsa_simplify_workspace_bytes(long long nr_verts, long long nr_faces);
int vsa_simplify(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                 long long target_faces, void* workspace, long long workspace_bytes, float* out_verts,
                 int32_t* out_faces, long long* stats, float* stage_ms, void* stream);
/* Guarded simplification: vsa_simplify with G = nr_guards guard meshes that the simplified mesh must not
 * newly cross -- a shell's neighbours in a stack (volsurfs_amd/simplify.py:simplify_shells).  Every rule above holds
 * unchanged; one condition is appended to `candidate`:
 *   guard         for every face at a or b that does not contain both (the faces the flip rule enumerates), taken in
 *                 its corner order with the moved vertex at the fp32 position p: that triangle, as A, must not cross
 *                 any face of any guard mesh, as B.  "Cross" is the rule of "Mesh crossings" below (tri_cross of
 *                 csrc/cross_walk.h): fp64 determinants of the fp32 bits; touching, coplanar, zero-area and NaN faces
 *                 cross nothing; a guard face with an index outside its vertex array is no face.
 * A candidate that fails gets the key UINT64_MAX like any other non-candidate; selection, acceptance order and
 * stalling are unchanged.  Winners share no face and no vertex and no winner's endpoint lies in another's ring, so the
 * faces one winner creates are untouched by the others: judging each candidate alone is exact for the mesh after the
 * round.  Faces of the input that already cross a guard are not judged: they go only when a collapse removes or
 * replaces them.  The verdict is an OR over all (new face, guard face) pairs: it does not depend on a guard's tree,
 * its builder or the order of the guards, and with guards that reject nothing the output is vsa_simplify's bit for
 * bit.  tests/simplify_guarded_restated.py restates the rule; the kernels are held to it bit for bit.
 *   guards        [host] arrays of nr_guards (1..4) entries, guard g: guard_qnodes[g], guard_tris[g] = the device
 *                 arrays of a q16 tree that holds the guard (vsa_bvh_quantize's nodes and the triangle records whose
 *                 v0.w is the face id), guard_roots[g] its root node, guard_frames[6 g .. 6 g + 6) its grid (lo, step),
 *                 guard_max_depths[g] its depth (< 48), guard_vertices[g] [V_g, 3] f32 and guard_faces[g] [F_g, 3]
 *                 i32 the guard mesh on the device, guard_nr_verts[g] = V_g, guard_nr_faces[g] = F_g, both >= 1.
 *                 This is the guard block (nr_guards and the nine arrays, in this order) of every entry point that
 *                 takes guards: one check and one device struct (cross_guards_bind, CrossGuards of csrc/cross_walk.h).
 *                 VSA_ERR_ARG: nr_guards outside 1..4, a NULL guard array or guard pointer, a negative root, a depth
 *                 >= 48, V_g or F_g < 1; then VSA_ERR_UNSUPPORTED: V_g >= 2^31 or 3 F_g + 3 >= 2^31.
 *   stats        [host] 6 long long: the five of vsa_simplify, then guard_rejected = the number of (round, edge)
 *                 verdicts the guard turned down (one integer atomicAdd per wave).
 *   stage_ms      [host] 7 floats or NULL: init, edges, cost, guard, select, collapse, compact.
 *   workspace     vsa_simplify_guarded_workspace_bytes(V, F) = vsa_simplify_workspace_bytes(V, F): the guard stage
 *                 places the vertex again as the collapse does and keeps no buffer of its own.
 * No blocking read is added to a round.  VSA_ERR_ARG, before any HIP call: the guard block's cases, and every case of
 * vsa_simplify. */
long long vsa_simplify_guarded_workspace_bytes(long long nr_verts, long long nr_faces);
int vsa_simplify_guarded(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                         long long target_faces, int nr_guards, const uint32_t* const* guard_qnodes,
                         const float* const* guard_tris, const int32_t* guard_roots, const float* guard_frames,
                         const int32_t* guard_max_depths, const float* const* guard_vertices,
                         const long long* guard_nr_verts, const int32_t* const* guard_faces,
                         const long long* guard_nr_faces, void* workspace, long long workspace_bytes,
                         float* out_verts, int32_t* out_faces, long long* stats, float* stage_ms, void* stream);

/* ------------------------------------------------------------------------
 * UV atlas (csrc/atlas.hip): box-projection charts of one uv-less, consistently wound triangle mesh, packed into one
 * square atlas -- the baker's `--compute_meshes_xatlas` step (xatlas in the reference, volsurfs_py/baker.py:727-776,
 * utils/texture_extraction.py::compute_o3d_mesh_atlas).
 *   verts [V, 3] f32 and faces [F, 3] i32 on the device: finite, indices in [0, V), no index twice in one face (the
 *   caller checks).  V, F >= 1.  resolution R in [8, 16384] (the atlas is R x R texels); padding p >= 0, 2p < R.
 * Rules (the output is a function of the mesh, R and p only; tests/test_atlas.py::restate restates them in numpy and
 * the kernels are held to it bit for bit; fp32 unless said, in the order written, with no contraction):
 *   label         n_f = (p1 - p0) x (p2 - p0) (e1 = p1 - p0, e2 = p2 - p0, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z,
 *                 e1x e2y - e1y e2x)).  N_v = 0 + the n_f of the faces at v in ascending face index (a sorted
 *                 (vertex, face) list); s_f = (N_a + N_b) + N_c.  Directions d = +x, -x, +y, -y, +z, -z (labels 0..5);
 *                 the candidate is the argmax of s_f . d (a component or its negation), ties to the earlier direction.
 *                 It is kept when n_f . d >= 0.5 |n_f|, evaluated in fp64 as c >= 0 and 4 (c c) >= (nx nx + ny ny) +
 *                 nz nz (c = n_f . d); otherwise the label is the argmax of n_f . d.  n_f = 0: label 0.  So a face keeps
 *                 at least half its area in projection and never flips.
 *   charts        faces f < g join when they share an undirected edge that has exactly two face corners, traverse it
 *                 in opposite directions, have the same label and the same split code, and the code is not 0.  A chart
 *                 is a connected component of the joins; its id is its minimum face index (union-find hooks the larger
 *                 root under the smaller), and charts are numbered 0 .. C-1 in ascending id.
 *   projection    by label: +x -> (u, v) = (y, z), -x -> (z, y), +y -> (z, x), -y -> (x, z), +z -> (x, y), -z -> (y, x)
 *                 (coordinates picked: exact; a face's projected signed area is >= 0).  Chart box: min / max of the
 *                 corners' u and v over its faces (as ordered float bits: -0 < +0).  w = umax - umin, h = vmax - vmin;
 *                 a chart with h > w is rotated by 90 degrees: local (x, y) = (vmax - v, u - umin), else (u - umin,
 *                 v - vmin); extents (ew, eh) = (h, w) rotated, else (w, h).
 *   pack          at density s (texels per unit), side(e) = ceil(e * s) + 2p, or R + 1 when ceil(e * s) > R; a chart's
 *                 rectangle is side(ew) x side(eh).  Rectangles sorted by (height desc, width desc, chart) are laid on
 *                 next-fit shelves of width R: a shelf starts at y = the heights of the shelves before it, takes
 *                 rectangles while their widths sum to <= R (a rectangle wider than R does not fit), and its height is
 *                 its first rectangle's.  The pack fits when the shelves' heights sum to <= R.  s = 0 fits when p = 0
 *                 or ceil(C / floor(R / 2p)) 2p <= R (else VSA_ERR_ATLAS_FULL); then s is the fp32 whose bit pattern
 *                 ends a bisection over bits lo = 0 (fits), hi = 0x7F800000 (never tried): mid = lo + (hi - lo) / 2
 *                 while hi - lo > 1, lo = mid when it fits, else hi = mid.
 *   uv            a corner of a face of chart c at offset (ox, oy): ((x * s + (float)(ox + p)) / R, (y * s +
 *                 (float)(oy + p)) / R), in [0, 1].  Chart contents lie p texels inside their rectangles, so two
 *                 charts' contents are at least 2p texels apart.
 *   raster        corners snapped in fp64: X = rint(clamp(u, 0, 1) * 256 R), Y likewise (int64, 1/256 texel, ties to
 *                 even).  Texel (i, j) (i along u, j along v; index j R + i) has centre (256 i + 128, 256 j + 128); it
 *                 is covered by a face with A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) > 0 when for every edge a -> b
 *                 (0 -> 1, 1 -> 2, 2 -> 0), e = dx (py - ay) - dy (px - ax) > 0, or e = 0 on a top-left edge (dy < 0, or
 *                 dy = 0 and dx < 0).  Faces with A <= 0 cover nothing.  A shared edge's points count once.
 *   overlap       after a pack, per-texel coverage counts of all faces; a chart holding a texel counted twice overlaps
 *                 itself (packed rectangles are disjoint).  Every face of such a chart: code 0 (one chart per face)
 *                 when its code is >= 2^24 (depth cap 24); else code = 2 code + side, side = 1 when (c0 + c1) + c2 >
 *                 1.5 (lo + hi) in fp64, with c_k the corners' coordinates along the chart box's longer side (u when
 *                 w >= h) and [lo, hi] the box on it.  Codes start at 1.  Charts are rebuilt and packed again, until
 *                 no chart overlaps itself.  VSA_ERR_UNSUPPORTED when a split changes no face's code (the next round
 *                 would repeat this one) or when round 100 (split rounds + 1) still finds an overlapping chart.
 *   output        out_faces_uvs [F, 3, 2] f32; out_chart [F] i32 (chart number); [host] scale: s; [host] stats 4 long
 *                 long: charts C, split rounds, covered texels (count >= 1), and on VSA_ERR_ATLAS_FULL the smallest
 *                 resolution at which C charts fit at s = 0 (else 0).
 *   stage_ms      [host] 5 floats or NULL: device ms of label, charts, pack, emit, raster (the overlap passes and the
 *                 split included) (events, one stream synchronisation per stage; NULL: none).
 * The host reads the chart count once per round, one fit flag per bisection step (31), the tile total and the number
 * of overlapping charts; the call synchronises `stream` before it returns.
 *   workspace     vsa_atlas_workspace_bytes(V, F, R): 20 bytes per vertex, 216 per face and 4 R^2 plus rocPRIM's
 *                 temporary storage (radix sorts of 3F keys) -- O(V + F + R^2).
 * VSA_ERR_ARG: a NULL pointer, V or F < 1, R outside [8, 16384], p < 0 or 2p >= R, a workspace smaller than asked for.
 * VSA_ERR_UNSUPPORTED: V >= 2^31 or 3 F + 3 >= 2^31 (and from the queries, a failed rocPRIM size query: no device).
 * VSA_ERR_ATLAS_FULL: C charts do not fit even at s = 0.  The
 * workspace query returns the byte count or one of those codes.
 *
 * vsa_atlas_rasterize: the raster rule above on any faces_uvs [F, 3, 2] f32 (device): out_face_id [R, R] i32 (the lowest
 * covering face, -1 when none) and out_count [R, R] i32 (covering faces), row j = v.  Workspace
 * vsa_atlas_rasterize_workspace_bytes(F) (16 bytes per face plus a scan's storage).  Synchronises `stream`.
 *
 * vsa_atlas_merged: vsa_atlas with its box charts merged into plane-projected groups first.  A connected
 * patch of box charts whose faces all fit one cone of directions is projected along its own summed normal, with the
 * box rule's kind of guarantee: every face keeps at least min_cos of its area and none flips.  Arguments: vsa_atlas's,
 * plus min_cos in (0, 1] and merge_rounds >= 0 (0: vsa_atlas's output, bit for bit).  Everything not named here is
 * vsa_atlas's rule unchanged, in the same operations and the same order; tests/atlas_merge_restated.py restates it.
 *   start         labels and charts as in vsa_atlas, all codes 1.  Every chart is a group, named by its minimum face,
 *                 unmerged, with the area vector A_g = 0 + the n_f of its faces (the label stage's fp32 normals, as
 *                 fp64) in ascending face index, per component, in fp64.
 *   adjacency     two groups are adjacent when faces of theirs share an undirected edge that has exactly two face
 *                 corners and is traversed in opposite directions (the join rule's edge test without the label test);
 *                 the weight of the pair is the number of such edges.
 *   validity      an adjacent pair a < b is valid when, with D = A_a + A_b (fp64, per component) and t2 = min_cos *
 *                 min_cos, every face f of both groups has n_f = 0, or c = (nx Dx + ny Dy) + nz Dz > 0 and c c >=
 *                 (t2 ((nx nx + ny ny) + nz nz)) ((Dx Dx + Dy Dy) + Dz Dz), all in fp64.  No square root is taken.
 *                 (A valid pair has D != 0, so no frame divides by zero: faces with n_f = 0 all carry label 0, adjacent
 *                 ones are one box chart already, and so no two adjacent groups consist of such faces only; a pair
 *                 with D = 0 and a face of n_f != 0 has c = 0 and fails.)
 *   round         every group picks, among its valid pairs, the neighbour of largest weight, ties to the smaller group
 *                 id.  Two groups that pick each other merge: the id is the smaller one (a), A_a becomes A_a + A_b (the
 *                 D that was tested, bit for bit), and the group is marked merged.  Picks are taken from the state at
 *                 the start of the round; the merging pairs are disjoint.  While a valid pair exists a round merges at
 *                 least one (the valid pair of largest weight, least smaller id, least other id is mutual).  Rounds
 *                 repeat until one finds no valid pair (it counts as a round run) or merge_rounds rounds have run;
 *                 every intermediate state is a valid set of groups.
 *   frames        an unmerged group keeps its label's coordinate pick.  A merged group with D = A_g: k = the index of
 *                 the smallest |D_k| (ties to the earlier); t = e_k x D, written out: k = 0: (0, -Dz, Dy), k = 1: (Dz, 0,
 *                 -Dx), k = 2: (-Dy, Dx, 0); b = D x t = (Dy tz - Dz ty, Dz tx - Dx tz, Dx ty - Dy tx); each divided by
 *                 the square root of its own squared length ((x x + y y) + z z), in fp64.  A corner's plane coordinates
 *                 are ((Px tx + Py ty) + Pz tz, (Px bx + Py by) + Pz bz) in fp64, each rounded once to fp32.  (t, b, D)
 *                 is right-handed, so a valid face's projected signed area is >= 0; both kinds of frame are isometries
 *                 of the plane, so one density s serves all charts.
 *   after         the join rule's "same label" reads "same group"; chart boxes, the 90 degree turn, the pack, the UV
 *                 formula, the raster and the overlap test are vsa_atlas's on the plane coordinates, and the split reads
 *                 the corners' coordinates along the box's longer side from them, so splits act inside groups.
 *   output        vsa_atlas's; [host] stats 8 long long: the four of vsa_atlas, then box charts before merging, groups
 *                 after it, merge rounds run, and valid pairs left when the rounds stopped.
 *   stage_ms      [host] 6 floats or NULL: vsa_atlas's five, then merge.
 * The host reads, on top of vsa_atlas's reads, the edge and box-chart counts once, the valid-pair count once per merge
 * round, and the merge count once.
 *   workspace     vsa_atlas_merged_workspace_bytes(V, F, R): vsa_atlas's plus 190 bytes per face -- O(V + F + R^2).
 * VSA_ERR_ARG: as vsa_atlas, and min_cos outside (0, 1] or NaN, merge_rounds < 0.  Other codes as vsa_atlas.
 */
#define VSA_ERR_ATLAS_FULL (-3)
long long vsa_atlas_workspace_bytes(long long nr_verts, long long nr_faces, int resolution);
int vsa_atlas(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces, int resolution,
              int padding, void* workspace, long long workspace_bytes, float* out_faces_uvs, int32_t* out_chart,
              long long* stats, float* scale, float* stage_ms, void* stream);
long long vsa_atlas_merged_workspace_bytes(long long nr_verts, long long nr_faces, int resolution);
int vsa_atlas_merged(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces, int resolution,
                     int padding, double min_cos, int merge_rounds, void* workspace, long long workspace_bytes,
                     float* out_faces_uvs, int32_t* out_chart, long long* stats, float* scale, float* stage_ms,
                     void* stream);
long long vsa_atlas_rasterize_workspace_bytes(long long nr_faces);
int vsa_atlas_rasterize(const float* faces_uvs, long long nr_faces, int resolution, void* workspace,
                        long long workspace_bytes, int32_t* out_face_id, int32_t* out_count, void* stream);

/* ---- sphere tracing (volsurfs_py/utils/sphere_tracing.py:112-152; csrc/sphere_trace.hip) ----
 * The round bookkeeping around an SDF that the host evaluates between the calls.  An item is one (ray, slot) pair,
 * item = slot * nr_rays + ray, M = nr_rays * nr_slots items (M + 256 < 2^31); slot s reads column slot_cols[s] of the
 * [rows, nr_columns] SDF block.  Buffers: pts [M,3] f32 (every item's current point), flags [M] u8 (bit 0 hit, bit 1
 * done), two live lists [M] i32 and two dense point blocks [M,3] f32 (ping-pong), keep [M] u8, block_counts
 * [ceil(M / 256)] i32, one i32 live count per round.
 *   vsa_st_begin   every item starts at its ray's points_near [N,3] row, flags 0, live = 0..M-1 ascending, dense = the
 *                  points, *count = M.
 *   vsa_st_step    one round.  `bound` (host) >= the device's *count_in: rows [0, *count_in) of `sdf` belong to the
 *                  live items live_in[j], in ascending item order; rows up to `bound` are padding and are not read.
 *                  Per live item, fp32 without contraction: p += d * (sdf * sdf_multiplier); newly = |sdf| < thresh;
 *                  hit |= newly; done |= newly; done |= !inside(p), inside = the closed test of the origin-centred cube
 *                  of HALF side `size` (kind 0) or sphere of radius `size` (kind 1).  Then the items that are not done,
 *                  in ascending item order, to live_out, their points to rows [0, *count_out) of dense_out; rows
 *                  [*count_out, bound) of dense_out take the same rows of dense_in.  Two launches (step, ordered
 *                  compaction); no atomics: the same inputs give the same bytes.
 *   vsa_st_finish  z [M] = ||p - rays_o[ray]||, hit [M] u8 = the hit flag (or not done, when unconverged_are_hits),
 *                  hit_list = the hit items in ascending order, *hit_count their number.
 *   vsa_st_scatter dst[(item % N) * S + item / N, :] = src[h, :] for item = ids[h], h < nr_ids (host), rows of
 *                  nr_channels f32.
 *   vsa_st_blend   methods/offsets_surfs.py:810-858 for surfs_rgb [N,K,3] and surfs_alpha [N,K,1], surfaces inner to
 *                  outer: surfs_transmittance, surfs_blending_weights [N,K,1], rgb_fg [N,3], bg_transmittance [N,1];
 *                  one thread per ray, the K products taken one after the other from the outer shell inwards and the
 *                  sum over the surfaces as four interleaved partial sums (torch's device orders: bit-identical). */
int vsa_st_begin(const float* points_near, int nr_rays, int nr_slots, float* pts, uint8_t* flags, int32_t* live,
                 float* dense, int32_t* count, void* stream);
int vsa_st_step(const int32_t* live_in, const int32_t* count_in, const float* sdf, int nr_columns,
                const int32_t* slot_cols, int nr_rays, const float* rays_d, float sdf_multiplier, float thresh,
                int kind, float size, float* pts, uint8_t* flags, uint8_t* keep, int32_t* block_counts,
                const float* dense_in, int32_t* live_out, float* dense_out, int32_t* count_out, int bound,
                void* stream);
int vsa_st_finish(const float* pts, const float* rays_o, int nr_rays, int nr_slots, const uint8_t* flags,
                  int unconverged_are_hits, float* z, uint8_t* hit, uint8_t* keep, int32_t* block_counts,
                  int32_t* hit_list, int32_t* hit_count, void* stream);
int vsa_st_scatter(const int32_t* ids, long long nr_ids, const float* src, int nr_channels, int nr_rays,
                   int nr_slots, float* dst, void* stream);
int vsa_st_blend(const float* surfs_rgb, const float* surfs_alpha, int nr_rays, int nr_surfs,
                 float* surfs_transmittance, float* surfs_blending_weights, float* rgb_fg, float* bg_transmittance,
                 void* stream);

/* ---- texture bake (volsurfs_py/utils/texture_extraction.py: extract_texture_from_color_model, dilate_texture;
 *      csrc/texture_bake.hip) ----
 * Turns an appearance model that is a 3-D field into a texture [R, R, C] over a mesh's UV atlas.  The model stays the
 * host's (a Python callable evaluated between vsa_tb_emit and vsa_tb_resolve); the sampling, the ownership of texels,
 * the ordered list of rows the model is evaluated on and the mean per texel are here.
 *   faces_uvs [F, 3, 2] f32 per-corner UVs in [0, 1]; verts [V, 3] f32; faces [F, 3] i32 (indices in [0, V): the caller
 *   checks; volsurfs_amd/texture_bake.py does).  R in [1, 8192] texels a side, S in [1, 64] samples per texel, R^2 S < 2^31, F < 2^31 - 256.
 * Texel (ix, iy), ix along u and iy along v, has index t = ix R + iy: the texture is [ix, iy, c], the reference's layout.
 * Rules (fp32, in the order written, no contraction; tests/texture_bake_restated.py restates them in torch and the
 * kernels are held to it bit for bit):
 *   box       face f visits ix in [floor(min_u R), ceil(max_u R)), iy likewise with v, both clamped to [0, R] (min / max
 *             over its three corners, the product in fp32).
 *   samples   sample 0 of a texel is its centre ((float)ix / (float)R + h, (float)iy / (float)R + h), h = (float)(1.0 /
 *             (2.0 R)) (the reference's `ix / R + 1 / (2 R)`).  Sample s in 1 .. S-1 is centre + ((r - 0.5f) - 1e-6f) /
 *             (float)R per axis.  r = r(seed, f, t, s, axis) is counter based (the reference draws from torch's global
 *             generator): with M = 0x5851f42d4c957f2d, I = 1442695040888963407 and 64-bit unsigned wrap-around,
 *               h = (seed + f + 1) M;  h ^= h >> 32;  h = (h + ((t S + s) 2 + axis) + 1) M;  h ^= h >> 32;  h = h M + I;
 *               x = (uint32)(((h >> 18) ^ h) >> 27);  k = h >> 59;  o = (x >> k) | (x << ((32 - k) & 31))  (PCG32's
 *               output of state h, csrc/pcg32.h);  r = bits_as_float((o >> 9) | 0x3f800000) - 1.0f in [0, 1).
 *             So a sample depends on nothing but its key, and S = 1 draws no number.
 *   inside    with (p1, p2, p3) the face's corner UVs: v0 = p3 - p1, v1 = p2 - p1, v2 = p - p1; dotab = va.x vb.x +
 *             va.y vb.y; inv = 1.0f / (dot00 dot11 - dot01 dot01); b2 = (dot11 dot02 - dot01 dot12) inv; b1 = (dot00
 *             dot12 - dot01 dot02) inv; b0 = (1.0f - b1) - b2.  Inside: b0, b1, b2 >= 0 and |((b0 + b1) + b2) - 1.0f| <
 *             1e-6f.  A face whose denominator is 0 or not finite has no inside sample (the reference's NaN / inf
 *             barycentrics fail the test the same way, except a few inf cases that are not reproduced).
 *   owner     a texel is covered by f when one of its S samples for f is inside; its owner is the HIGHEST such f (the
 *             reference writes faces in ascending order, each over the last), -1 when none.  (vsa_atlas_rasterize
 *             reports the lowest face under another fill rule: it is not this map.)
 *   rows      the owner's inside samples of every covered texel, ordered by t and then by s: point = (b0 A + b1 B) +
 *             b2 C per component for the face's vertices A, B, C; normal = n / max(sqrt((nx nx + ny ny) + nz nz), 1e-12)
 *             with n = (B - A) x (C - A) = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), the same for all
 *             the face's rows.  row_start [R^2 + 1] i32: rows of texel t are [row_start[t], row_start[t + 1]).
 *   mean      texture[t, c] = (vals[r0, c] + vals[r0 + 1, c] + ...) / (float)count, summed from the first row on;
 *             texels without rows are not written (the caller zeroes the texture).
 * vsa_tb_samples: boxes -> a one-block scan of the box sizes -> one thread per (face, texel of its box) pair, by binary
 *   search in the scanned sizes, over a fixed grid that strides to the device's pair total (work is proportional to the
 *   summed box areas, whatever the spread of the faces' sizes; atomicMax on owner, the only atomic besides the error
 *   flag) -> per texel the 64-bit inside mask of its owner and the rows per 256 texels -> a one-block scan of those ->
 *   the plan.  Six launches and two memsets whatever F; nothing is read back.  ctl [ctl_len >= 4 + 2 (max_chunks + 1)]
 *   i32 receives [0] the number of rows M, [1] the number of chunks n (-1: the table overflowed), [2] bit 0 set when a UV
 *   is NaN, inf or outside [0, 1] (then nothing is baked: owner is -1 everywhere and M = 0), [4 + 2 c] the first texel
 *   of chunk c and [5 + 2 c] its first row, entry n being (R^2, M): chunk c is the longest run of texels from its first
 *   whose rows number <= chunk_rows (chunk_rows >= S), so chunks never split a texel's rows.  owner [R, R] i32.
 *   vsa_tb_max_chunks bounds n: R^2 S / (chunk_rows - S + 1) + 2, VSA_ERR_ARG when that exceeds 2^20 (the plan walks the
 *   chunks on one thread).
 *   workspace: vsa_tb_workspace_bytes(F, R) = 12 bytes per face and 8 per texel plus 12 per 256 texels, kept for
 *   vsa_tb_emit.
 * vsa_tb_emit: row_start, points [M, 3] and normals [M, 3] by an ordered compaction (block offsets from the scan, a
 *   shuffle scan inside the block); same arguments and workspace as the vsa_tb_samples call before it.
 * vsa_tb_resolve: the mean of the texels [texel_begin, texel_end) from vals [rows, C], whose first row is row
 *   row_start[texel_begin].
 * vsa_tb_dilate: dilate_texture on img [H, W, C] in place.  A pixel is full when all its channels are != 0, empty when
 *   all are == 0, and never a source or a destination otherwise.  Iteration 1's sources are the full pixels, iteration
 *   i's the pixels filled in iteration i - 1; an empty pixel with a source among its 8 neighbours copies the first one
 *   in the order (-1,-1), (-1,0), (-1,1), (0,-1), (0,1), (1,-1), (1,0), (1,1) of (row, column) offsets (the source the
 *   reference's np.unique keeps).  stamp [H W] i32 (the iteration that filled a pixel: a gather, race-free in place)
 *   and filled [nr_iterations + 1] i32 are scratch; once an iteration fills nothing the remaining launches return at
 *   once (the reference's early stop), nr_iterations + 1 launches, at most 4097.
 * VSA_ERR_ARG: a NULL pointer, a size outside the ranges above, chunk_rows < S, a workspace or ctl smaller than asked. */
long long vsa_tb_workspace_bytes(long long nr_faces, int resolution);
long long vsa_tb_max_chunks(int resolution, int nr_samples, long long chunk_rows);
int vsa_tb_samples(const float* faces_uvs, long long nr_faces, int resolution, int nr_samples,
                   unsigned long long seed, long long chunk_rows, void* workspace, long long workspace_bytes,
                   int32_t* owner, int32_t* ctl, int ctl_len, void* stream);
int vsa_tb_emit(const float* verts, const int32_t* faces, const float* faces_uvs, long long nr_faces, int resolution,
                int nr_samples, unsigned long long seed, const void* workspace, long long workspace_bytes,
                const int32_t* owner, int32_t* row_start, float* points, float* normals, void* stream);
int vsa_tb_resolve(const float* vals, int nr_channels, const int32_t* row_start, int texel_begin, int texel_end,
                   int resolution, float* texture, void* stream);
int vsa_tb_dilate(float* img, int height, int width, int nr_channels, int nr_iterations, int32_t* stamp,
                  int32_t* filled, void* stream);

/* ---- TSDF fusion (volsurfs_py/utils/mesh_from_depth.py:220-300: compute_sdf_perframe, compute_unbounded_tsdf;
 *      csrc/tsdf_fuse.hip) ----
 * The background mesh of the baker: V depth maps fused into a truncated signed distance at query points.  The
 * reference makes V passes of torch ops over all points; here a point walks the views i = 0 .. V-1 IN ORDER with its
 * state in registers and is written once.
 *   proj [V, 4, 4] f32 row-major: the `full_proj_transform` of to_cam_open3d (mesh_from_depth.py:122-147),
 *   getProjectionMatrix(0.1, 100, fovx, fovy) @ w2c, the fovs from intrinsic_to_fov with the image size taken as
 *   (2 cx, 2 cy); volsurfs_amd/bg_mesh.py builds it.  depth [V, H, W] f32 (camera z, 0 where nothing was hit),
 *   rgb_maps [V, 3, H, W] f32.  H, W in [1, 2^15], V in [1, 2^20].
 * Rule per point p and view i (fp32, in the order written, no contraction; tests/bg_mesh_restated.py restates it in
 * torch as the reference formulates it).  State: tsdf = 1, rgb = 0, w = 1 (the initial 1 counts as a sample).
 *   h_r   = ((p.x P[r][0] + p.y P[r][1]) + p.z P[r][2]) + P[r][3] for r = 0, 1, 3;  z = h_3;  u = h_0 / z;  v = h_1 / z
 *   mask  = u > -1 and u < 1 and v > -1 and v < 1 and z > 0
 *   d     = grid_sample(depth_i, (u, v), bilinear, align_corners=True): ix = ((u + 1) / 2) (W - 1), iy likewise with
 *           H, clamped to the image; x0 = floor(ix), y0 = floor(iy); weights nw = ((x0 + 1) - ix) ((y0 + 1) - iy),
 *           ne = (ix - x0) ((y0 + 1) - iy), sw = ((x0 + 1) - ix) (iy - y0), se = (ix - x0) (iy - y0); d = the sum of
 *           tap * weight in the order nw, ne, sw, se from 0, a tap outside the image left out
 *   sdf   = d - z;  mask = mask and sdf > -sdf_trunc;  s = min(max(sdf / sdf_trunc, -1), 1)
 *   under the mask: tsdf = (tsdf w + s) / (w + 1);  rgb_c = (rgb_c w + colour_c) / (w + 1) with colour_c the same
 *           four taps of channel c;  w = w + 1
 * `uncontract`: the query position is the inverse contraction of the given point (RaySamplerGPU.cuh:595-650 without
 *   the ray part, as vsa_uncontract_samples: q = 2 p, norm = sqrt((q.x q.x + q.y q.y) + q.z q.z); when norm > 1,
 *   factor = 1 / (2 - norm) and p = (factor p) / norm).  A point with norm >= 2 lies outside the contraction's image:
 *   it is not fused and keeps tsdf = 1, rgb = 0.  (The reference has this line commented out, mesh_from_depth.py:264.)
 * vsa_tsdf_fuse_lattice: the points are the lattice (axis[i], axis[j], axis[k]), axis [n] f32 on the device (the values
 *   of torch.linspace in fp32, as isosurface.sample_grid builds them), n in [2, 4096]; out_tsdf [n, n, n] f32,
 *   C-contiguous (what vsa_isosurface_count takes).  A wave is a 4 x 4 x 4 brick of the lattice.
 * vsa_tsdf_fuse_points: points [P, 3] f32 -> out_tsdf [P] and, when rgb_maps and out_rgb are given (both or neither),
 *   out_rgb [P, 3]: the vertex-colour pass.  P = 0 is fine.  The same device function: the lattice entry and this one
 *   give the same bits on the same positions.
 * vsa_tsdf_uncontract_points: the vertex step of the extraction: out [P, 3] = the inverse contraction of points
 *   [P, 3], clipped per component to +-max_range; a point with norm >= 2 goes to infinity along its own direction
 *   before the clip (+-max_range in its non-zero components, 0 in the others).  In place is fine.
 * No atomics: the same inputs give the same bytes.
 * VSA_ERR_ARG: a NULL pointer, nr_views < 1, n < 2, sdf_trunc <= 0 or not finite, a size outside the ranges above,
 *   one of rgb_maps / out_rgb without the other, max_range <= 0 or not finite. */
int vsa_tsdf_fuse_lattice(const float* proj, const float* depth, int nr_views, int height, int width,
                          const float* axis, int n, float sdf_trunc, int uncontract, float* out_tsdf, void* stream);
int vsa_tsdf_fuse_points(const float* proj, const float* depth, const float* rgb_maps, int nr_views, int height,
                         int width, const float* points, long long nr_points, float sdf_trunc, int uncontract,
                         float* out_tsdf, float* out_rgb, void* stream);
int vsa_tsdf_uncontract_points(const float* points, long long nr_points, float max_range, float* out, void* stream);

/* ---- Mesh cleaning (volsurfs_py/utils/mesh_extraction.py:18-46 `post_process_mesh`; csrc/mesh_clean.hip) ----
 * Connected triangle clusters of a plain mesh and the removal of the small ones ("floaters").  The reference calls
 * Open3D (cluster_connected_triangles, remove_triangles_by_mask, remove_unreferenced_vertices,
 * remove_degenerate_triangles), which is absent: the rule is restated here and in tests/mesh_clean_restated.py, and is
 * UNPINNED against Open3D itself.
 *   verts [V, 3] f32 and faces [F, 3] i32 on the device: finite, indices in [0, V) (the caller checks).  V, F >= 1.  A
 *   face may name a vertex twice.
 * Rules (the outputs are a function of the mesh and the arguments only):
 *   adjacency     two faces are adjacent when they share an undirected edge: the same unordered pair of vertex
 *                 INDICES (key = min << s | max, s = the bits of V - 1) among their three corner pairs (0, 1), (1, 2),
 *                 (2, 0).  Every face of an edge with three or more faces is joined; faces that share only a vertex are
 *                 not.  A face (a, a, b) has the pairs (a, a), (a, b), (a, b) and takes part through them.
 *   clusters      the connected components of the adjacency, numbered 0 .. C-1 in ascending order of their smallest
 *                 face index (union-find hooks the larger root under the smaller, so a root is its component's minimum
 *                 face whatever the order of the hooks).  triangle_clusters [F] i32; cluster_n_triangles [C] i32
 *                 (integer atomics).
 *   areas         cluster_area [C] f64: the sum over the cluster's faces of 0.5 sqrt((nx nx + ny ny) + nz nz), n = (p1 -
 *                 p0) x (p2 - p0) as e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x, every operation in fp64 on
 *                 the fp32 coordinates, no contraction.  The faces are taken in ascending index (a stable sort by
 *                 cluster); sorted positions are cut into chunks of 2048, a chunk is summed by 256 lanes (8 consecutive
 *                 faces each, in order, then a Hillis-Steele segmented scan of the lanes), and a cluster that spans
 *                 several chunks adds its pieces by one wave (lane l the pieces l, l + 64, ... in order, then a shuffle
 *                 tree).  The shape is fixed: same mesh, same bits.
 *   threshold     (mode 2) n = max(the k-th largest cluster_n_triangles, min_cluster_faces), k = min(cluster_to_keep,
 *                 C) -- the reference indexes the sorted counts with cluster_to_keep itself and raises when C is
 *                 smaller; this is the one departure.  A face passes when its cluster has >= n faces (the reference
 *                 removes on a strict <), so clusters tied at n all stay.
 *   filter        mode 0: every face passes; 1: face f passes when keep_mask[f] != 0 (u8 [F]); 2: the threshold.  Then,
 *                 in the reference's order: drop_unreferenced keeps the vertices named by a passing face (else all),
 *                 in input order with their bits, and the faces are renumbered; drop_degenerate then drops the passing
 *                 faces that name a vertex twice -- the vertices such a face named stay.  Faces keep input order.
 *   output        out_verts [V, 3] f32 and out_faces [F, 3] i32 sized for the input, the first V_out / F_out rows
 *                 written; out_vertex_map [V] and out_face_map [F] i32: old -> new index, -1 for a dropped one.
 *                 stats [host] 6 long long: V_out, F_out, C, n, the clusters with >= n faces (the three 0 unless mode
 *                 2), the faces that passed (degenerate ones included).
 *   stage_ms      [host] 9 floats or NULL: device ms of edges, sort, hook, roots, number, areas (vsa_mesh_clusters
 *                 only), threshold, mask, compact (vsa_mesh_filter only) (events, one stream synchronisation per
 *                 stage; NULL: none).
 * Blocking reads: C once (vsa_mesh_clusters, and vsa_mesh_filter in mode 2), then the totals once; their number does
 * not depend on F or C.  Both calls synchronise `stream` before they return.
 *   workspace     vsa_mesh_clusters_workspace_bytes(V, F), for both calls: 96 bytes per face and 8 per max(V, F) plus 4
 *                 per vertex of this library's arrays, and rocPRIM's temporary storage, which for its sort of the 3F
 *                 (u64, u32) pairs is itself about 36 bytes per face -- about 140 bytes per face in all, O(V + F).
 * vsa_mesh_clusters: out_triangle_clusters [F] i32; out_cluster_n_triangles [F] i32 and out_cluster_area [F] f64, the
 *   first C entries meaningful; out_nr_clusters [host] one long long.
 * vsa_mesh_compact_rows: out[map[i]] = rows[i] for map[i] >= 0, rows of row_words 32-bit words: the per-vertex and
 *   per-corner attributes through a map of vsa_mesh_filter.  nr_rows = 0 is fine.
 * VSA_ERR_ARG: a NULL pointer (keep_mask only in mode 1; stage_ms may be NULL), V or F < 1, mode outside 0..2,
 *   cluster_to_keep < 1 or min_cluster_faces < 0 in mode 2, a workspace smaller than asked for, row_words < 1,
 *   nr_rows < 0.  VSA_ERR_UNSUPPORTED: V >= 2^31 or 3 F + 3 >= 2^31 (and from the query, a failed rocPRIM size query: no
 *   device).  The outputs are untouched on either.  The workspace query returns the byte count or one of those codes. */
long long vsa_mesh_clusters_workspace_bytes(long long nr_verts, long long nr_faces);
int vsa_mesh_clusters(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces,
                      void* workspace, long long workspace_bytes, int32_t* out_triangle_clusters,
                      int32_t* out_cluster_n_triangles, double* out_cluster_area, long long* out_nr_clusters,
                      float* stage_ms, void* stream);
int vsa_mesh_filter(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces, int mode,
                    const uint8_t* keep_mask, long long cluster_to_keep, long long min_cluster_faces,
                    int drop_unreferenced, int drop_degenerate, void* workspace, long long workspace_bytes,
                    float* out_verts, int32_t* out_faces, int32_t* out_vertex_map, int32_t* out_face_map,
                    long long* stats, float* stage_ms, void* stream);
int vsa_mesh_compact_rows(const void* rows, long long nr_rows, int row_words, const int32_t* map, void* out,
                          void* stream);

/* ---- Face visibility (volsurfs_py/baker.py:140-144 `--remove_invisible_faces`, a stub in the reference;
 *      csrc/face_visibility.hip) ----
 * Which faces of K shells are some view's closest hit.  The reference never implemented the stage: the rule below is
 * this library's own, restated and UNPINNED.
 * vsa_face_view_counts: qnodes / tris / mesh_roots / mesh_frames / max_depth as vsa_trace_q takes them (q16 nodes);
 *   c2w_all [V, 3, 4] and intrinsics_inv_all [V, 3, 3] f32 on the device, all views height x width.
 *   samples       pixel (col, row) has supersample^2 samples: (i, j) goes through the point x = col + (i + 0.5f) / s,
 *                 y = row + (j + 0.5f) / s (fp32, in that order); its ray is vsa_camera_rays' pinhole ray of (x, y).
 *                 s = 1 is col + 0.5f: the unjittered ray of vsa_camera_rays bit for bit.
 *   hit           per shell on its own (other shells do not occlude), the closest hit of vsa_trace_q: smallest t, ties
 *                 to the smallest original face id, a hit iff t > t_min.
 *   counts        [device] u32, zeroed by the caller: counts[face_base[k] + f] += 1 for every sample of every view whose
 *                 closest hit on shell k is face f (the original id, word 3 of the triangle record).  face_base [host]
 *                 nr_meshes long long >= 0.  Integer atomics only: exact, the same for every schedule.  Nothing else is
 *                 written to memory.
 *   One launch of one wave per (view, tile of 64 samples, shell); the tile is 8 x 8 samples, or 64 samples of a row after
 *   vsa_face_view_counts_tile(1) (process-wide; 0 = 8 x 8, the default; the counts do not depend on it).
 *   VSA_ERR_ARG (before any HIP call): a NULL pointer, nr_meshes outside 1..16, nr_views / height / width < 1,
 *   supersample outside 1..8, max_depth >= 48, nr_views * height * width * supersample^2 >= 2^32 (a u32 count could
 *   wrap), a negative face_base.  VSA_ERR_UNSUPPORTED: more than 2^31 - 1 tiles over all views (within the sample bound
 *   only images a few samples wide or high, whose tiles are mostly empty, get there).
 * vsa_face_ring_dilate: keep [F] u8 in / out grown by `rings` (0..16) vertex rings of faces [F, 3] i32 (indices in
 *   [0, V): the caller checks).  Per ring: vert_scratch [V] u8 cleared; every face with keep != 0 sets vert_scratch = 1
 *   at its three vertices; then every face with a set vertex sets keep = 1.  Two passes, so a ring reads the previous
 *   ring's mask only: the result is a function of the mesh and the mask.  rings = 0 touches nothing.
 *   VSA_ERR_ARG (before any HIP call): a NULL pointer, nr_faces or nr_verts < 1, rings outside 0..16. */
int vsa_face_view_counts(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                         const float* mesh_frames, int nr_meshes, int max_depth,
                         const float* c2w_all, const float* intrinsics_inv_all,
                         int nr_views, int height, int width, int supersample, float t_min,
                         const long long* face_base, uint32_t* counts,
                         void* stream);
int vsa_face_view_counts_tile(int tile);
int vsa_face_ring_dilate(const int32_t* faces, long long nr_faces, long long nr_verts, uint8_t* keep,
                         int rings, uint8_t* vert_scratch, void* stream);

/* ---- Mesh distance (no counterpart in the reference; csrc/mesh_distance.hip, csrc/closest_walk.h) ----
 * The closest point of a mesh to a query point, an area-weighted surface sampler, and the two fused into the
 * statistics of a sampled surface-to-surface distance.  The reference has no such stage: the rule below is this
 * library's own, restated in tests/mesh_distance_restated.py and UNPINNED.
 * qnodes / tris / mesh_roots / mesh_frames / max_depth as vsa_trace_q takes them (q16 nodes, leaf-ordered records
 * v0.xyz, id | e1.xyz, - | e2.xyz, -).
 *   closest point per point p and record (fp32, in the order written, no contraction): a = p - v0; d1 = e1.a, d2 = e2.a;
 *                 b = a - e1; d3 = e1.b, d4 = e2.b; c = a - e2; d5 = e1.c, d6 = e2.c (x.y = (x0 y0 + x1 y1) + x2 y2);
 *                 vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.  The first region that holds, in
 *                 Ericson's order, gives the weights (u, v) of v1 and v2:
 *                   A   d1 <= 0 and d2 <= 0                                        (0, 0)
 *                   B   d3 >= 0 and d4 <= d3                                       (1, 0)
 *                   AB  vc <= 0, d1 >= 0, d3 <= 0, d1 - d3 > 0                     (d1 / (d1 - d3), 0)
 *                   C   d6 >= 0 and d5 <= d6                                       (0, 1)
 *                   AC  vb <= 0, d2 >= 0, d6 <= 0, d2 - d6 > 0                     (0, d2 / (d2 - d6))
 *                   BC  va <= 0, s = d4 - d3 >= 0, t = d5 - d6 >= 0, s + t > 0     v = s / (s + t), u = 1 - v
 *                   in  (va + vb) + vc > 0                                         (vb, vc) * (1 / ((va + vb) + vc))
 *                   otherwise (0, 0).  The positive denominators are the handling of zero-area records: a record
 *                 with a zero edge falls through to the next region, e1 = e2 = 0 ends in A (the point v0).
 *                 r = (a - u e1) - v e2 per component; d2 = r.r.
 *   closest triangle  the minimum over (d2, original face id) of all records of the mesh: tri_test's tie rule.  A
 *                 query with a NaN coordinate has no closest triangle: slot -1, dist +inf.
 *   walk          one query per lane over the q16 nodes, a child pruned when a lower bound of its box's squared
 *                 distance exceeds the best d2 so far.  The bound (grid gap x step per axis, squared, summed, scaled by
 *                 1 - 2^-18; the boxes' one-unit margin) never exceeds the fp32 d2 of a triangle inside the box for
 *                 queries within ~60 mesh extents of the mesh, the domain of vsa_trace_q: there the result is that of
 *                 brute force over all records, bit for bit.  Beyond it a nearer triangle may be missed.
 * vsa_closest_point_q: points [N, 3] f32 -> dist [K, N] f32 = sqrtf(d2), slot [K, N] i32 (index into tris), bary
 *   [K, N, 2] f32 = (u, v) or NULL.  One launch, grid.y = mesh.  No atomics.
 * vsa_closest_point_q_stats: the same walk with counters (measurement): counters [device] 3 long long = node visits,
 *   triangle tests, queries, summed over the K meshes; nothing else is written.
 * vsa_surface_area_prefix: area_prefix [nr_slots] i64 = the inclusive prefix of the integer weights of the records
 *   [first_slot, first_slot + nr_slots).  area = 0.5 sqrt((nx nx + ny ny) + nz nz), n = e1 x e2, in fp64 on the fp32
 *   edges; weight = floor(area 2^k) with 2^k the power of two that puts the largest area in [2^30, 2^31) (a step of at
 *   most 2^-30 of the largest area; the total stays below 2^62); a zero or non-finite area weighs 0; when no area is
 *   positive every record weighs 1.  Integers: the prefix is exact whatever the scan's shape.  workspace =
 *   vsa_surface_area_prefix_workspace_bytes(nr_slots) bytes.
 * vsa_surface_sample: sample i of n: a Pcg32 stream keyed by (seed, i) (state = splitmix64's finaliser of seed +
 *   0x9E3779B97F4A7C15 (i + 1), one output discarded) draws xi, u, v in [0, 1); position = floor(((i + xi) / n) total) in
 *   fp64, clamped to total - 1; the record is the first whose prefix exceeds the position (a weight-0 record is never
 *   chosen); u + v > 1 folds to (1 - u, 1 - v); point = (v0 + u e1) + v e2 in fp32.  points [n, 3] f32, slot [n] i32
 *   (index into tris) or NULL, bary [n, 2] f32 or NULL.  A function of (tris, n, seed): the same bytes on every call.
 * vsa_surface_distance: the statistics of the distances from n samples of the source records to the destination mesh
 *   (one tree: its root, its frame of 6 floats [host], its depth), fused: the device functions of the two entry points
 *   above, no sample and no distance written.  stats [device] 12 64-bit words: the bits of the smallest and of the
 *   largest fp32 distance (integer atomics on the bits, which order as the non-negative values do), sum d and sum d^2
 *   as fp64 (every wave adds its 64 lanes by a fixed tree into partials [ceil(n / 64), 2] f64; a second kernel adds
 *   the pairs in wave order in a shape fixed by the wave count: 1024 lanes each add a run of consecutive waves, one lane
 *   adds the 1024 run sums in order), within[j] = #{d <= thresholds[j]} (integer atomics), j < 8.  thresholds [host].  No float
 *   atomics: the same inputs give the same bytes.
 * vsa_closest_walk_config(keep_bounds): process-wide; a stack entry can carry its child's bound and be dropped on the
 *   pop when the best d2 has passed it (a second LDS word per entry), or hold the node only, which is then fetched and
 *   its children tested.  1 (default): bounds with the 24-entry stack (max_depth < 24), node only with the 48-entry one;
 *   0: node only; 2: bounds always.  The results do not depend on it; tools/mesh_distance_bench.py measures 0 and 2.
 * VSA_ERR_ARG (before any HIP call): a NULL pointer (bary, and slot of vsa_surface_sample, may be NULL; thresholds when
 *   nr_thresholds = 0), nr_meshes outside 1..16, nr_points / nr_slots / nr_samples < 1, a negative first_slot or root,
 *   max_depth >= 48, nr_thresholds outside 0..8, a negative or NaN threshold; a workspace smaller than asked for.
 *   VSA_ERR_UNSUPPORTED: slots beyond 2^31 - 1, more than 2^31 - 1 waves (and from the query, a failed rocPRIM size
 *   query: no device). */
int vsa_closest_point_q(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                        const float* mesh_frames, int nr_meshes, int max_depth, const float* points,
                        long long nr_points, float* dist, int32_t* slot, float* bary, void* stream);
int vsa_closest_point_q_stats(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                              const float* mesh_frames, int nr_meshes, int max_depth, const float* points,
                              long long nr_points, long long* counters, void* stream);
int vsa_closest_walk_config(int keep_bounds);
long long vsa_surface_area_prefix_workspace_bytes(long long nr_slots);
int vsa_surface_area_prefix(const float* tris, long long first_slot, long long nr_slots, void* workspace,
                            long long workspace_bytes, long long* area_prefix, void* stream);
int vsa_surface_sample(const float* tris, long long first_slot, long long nr_slots, const long long* area_prefix,
                       long long nr_samples, unsigned long long seed, float* points, int32_t* slot, float* bary,
                       void* stream);
int vsa_surface_distance(const float* src_tris, long long src_first_slot, long long src_nr_slots,
                         const long long* src_area_prefix, const uint32_t* dst_qnodes, const float* dst_tris,
                         int dst_root, const float* dst_frame, int dst_max_depth, long long nr_samples,
                         unsigned long long seed, const float* thresholds, int nr_thresholds,
                         unsigned long long* stats, double* partials, void* stream);

/* ---- Mesh signed distance (no counterpart in the reference; csrc/mesh_sdf.hip, csrc/closest_walk.h) ----
 * The distance of "Mesh distance" with a sign: negative inside a closed mesh whose faces wind outward (as
 * marching cubes and icosphere wind them).  The sign is that of r . N, N the angle-weighted pseudonormal of the closest
 * feature (Baerentzen & Aanaes 2005).  The reference has no such stage: the rule below is this library's own, restated
 * in tests/mesh_sdf_restated.py and UNPINNED.  The sign means inside / outside for closed, consistently oriented
 * meshes; for any other mesh it is whatever the rule gives.
 *   region        the region of the closest record that "Mesh distance" chose, as a code: A 0, B 1, C 2 (the vertices
 *                 v0, v1, v2), AB 3, AC 4, BC 5 (the edges), in 6; "otherwise" is A.  It comes out of the same chain of
 *                 tests as (u, v), never from (u, v) afterwards; r = (a - u e1) - v e2 is the residual formed there.
 *   face normal   n_f = (e1 x e2) / |e1 x e2| with e1 = v1 - v0, e2 = v2 - v0, the cross product (a.y b.z - a.z b.y, ..),
 *                 |n| = sqrt((nx nx + ny ny) + nz nz), every operation in fp64 on the fp32 vertices; 0 when |n| is not
 *                 positive and finite (a zero-area face contributes nothing anywhere).
 *   pseudonormal  in:     n_f.
 *                 edge:   the sum of n_f over every face corner whose undirected edge key (min, max vertex) is the
 *                         edge's, in ascending face id: one face on a boundary, two on a manifold edge, or more.
 *                 vertex: the sum over the (vertex, face) ring of the vertex, in ascending face id, of alpha n_f, alpha =
 *                         atan2(|a x b|, a . b) of the two edges a, b that leave the vertex in that face (at the first
 *                         corner that names it), a . b = (a0 b0 + a1 b1) + a2 b2.
 *                 Sums in fp64 from 0, each stored rounded to fp32.
 *   sign          s = r . N = (r0 N0 + r1 N1) + r2 N2 in fp32; the signed distance is -sqrtf(d2) when s < 0, else
 *                 +sqrtf(d2): a point on the surface gets +0, a NaN query keeps slot -1 and +inf.
 * vsa_mesh_pseudonormals: vertices [V, 3] f32, faces [F, 3] i32 (indices in [0, V): the caller checks) -> table
 *   [F, 7, 3] f32, row f = original face id, entry = region code.  Vertex rings and sorted edges of csrc/mesh_topology.hip,
 *   one thread per vertex / per sorted face corner, no float atomics: the same inputs give the same bytes.  workspace =
 *   vsa_mesh_pseudonormals_workspace_bytes(V, F) bytes.
 * vsa_signed_distance_q: vsa_closest_point_q with the tables: table [sum F_k, 7, 3] f32 (the meshes' tables one after
 *   the other), table_face_base [host, nr_meshes] = the first row of each mesh.  The same outputs, dist signed; |dist|,
 *   slot and bary are vsa_closest_point_q's bits.
 * vsa_mesh_sdf_grid: grid [nx, ny, nz] f32 (C order) = clamp(signed distance at (x[i], y[j], z[k]), -band, band) to ONE
 *   mesh (its root, its frame of 6 floats [host], its first table row).  x / y / z are device arrays of the axis values
 *   themselves.  band = +inf: the whole field, one wave per 4 x 4 x 4 brick of lattice points, nothing else.  A finite
 *   band: one lane per brick first takes d_c at the brick's centre (per axis the mean of the brick's first and last
 *   value) and rho = the distance from the centre to the brick's farthest lattice point; a brick with |d_c| > band +
 *   (4/3) rho is FAR and filled with copysignf(band, d_c) (the distance is 1-Lipschitz: every point of it has |d| >=
 *   |d_c| - rho > band and lies on the centre's side), the others are compacted in ascending brick order (flags,
 *   exclusive scan, scatter) and walked.  brick_counts [host, 2] = near, far bricks, through one blocking read of the
 *   stream (none with band = +inf).  workspace = vsa_mesh_sdf_grid_workspace_bytes(nx, ny, nz) bytes (may be NULL with
 *   band = +inf).
 * The walk's stack form follows vsa_closest_walk_config.
 * VSA_ERR_ARG (before any HIP call): a NULL pointer (bary may be NULL), V, F, nr_points or an axis length < 1,
 *   nr_meshes outside 1..16, max_depth >= 48, a negative root or table row, band <= 0 or NaN; a workspace smaller than
 *   asked for.  VSA_ERR_UNSUPPORTED: 3 F + 3 beyond int32, more than 2^31 - 1 waves or bricks (and from the queries, a
 *   failed rocPRIM size query: no device). */
long long vsa_mesh_pseudonormals_workspace_bytes(long long nr_verts, long long nr_faces);
int vsa_mesh_pseudonormals(const float* vertices, long long nr_verts, const int32_t* faces, long long nr_faces,
                           void* workspace, long long workspace_bytes, float* table, void* stream);
int vsa_signed_distance_q(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                          const float* mesh_frames, int nr_meshes, int max_depth, const float* table,
                          const long long* table_face_base, const float* points, long long nr_points, float* dist,
                          int32_t* slot, float* bary, void* stream);
long long vsa_mesh_sdf_grid_workspace_bytes(int nx, int ny, int nz);
int vsa_mesh_sdf_grid(const uint32_t* qnodes, const float* tris, int root, const float* frame, int max_depth,
                      const float* table, long long table_face_base, const float* x, const float* y, const float* z,
                      int nx, int ny, int nz, float band, float* grid, void* workspace, long long workspace_bytes,
                      long long* brick_counts, void* stream);

/* ---- Mesh winding number (no counterpart in the reference; csrc/mesh_winding.hip, csrc/winding_walk.h) ----
 * A sign for meshes that are not closed: the generalised winding number w(q) = sum over the faces of Omega_f(q) / 4 pi
 * (Jacobson et al. 2013), about 1 inside and about 0 outside, with the far field of Barill et al. 2018 at order 0.  The
 * reference has no such stage: the rule below is this library's own and UNPINNED; the exact sum is restated in float64
 * in tests/mesh_sdf_restated.py (winding_number).
 *   exact term    for a triangle record (v0, e1, e2) and the query q: a = v0 - q, b = a + e1, c = a + e2,
 *                 Omega = 2 atan2f(a . (b x c), den), den = (((|a| |b|) |c| + (a . b) |c|) + (b . c) |a|) + (c . a) |b|,
 *                 in fp32: x . y = (x0 y0 + x1 y1) + x2 y2, |x| = sqrtf(x . x), b x c = (b1 c2 - b2 c1, b2 c0 - b0 c2,
 *                 b0 c1 - b1 c0), no fused multiply-add.  atan2f(0, 0) = 0: a query on a vertex, and a face without
 *                 area, contribute 0.
 *   moments       every subtree of the q16 tree carries N = sum 1/2 e1 x e2, the area-weighted centroid p = sum (area
 *                 centroid) / sum area (area = |1/2 e1 x e2|, centroid = v0 + (e1 + e2) / 3) and a radius r: no vertex
 *                 of the subtree is farther than r from p.  The sums are fp64 on the fp32 records, a leaf's triangles in
 *                 slot order, an inner subtree child 0 plus child 1; each is stored once, rounded to fp32.  r of a leaf
 *                 is the largest distance (fp64) from the stored p to a vertex (v0, v0 + e1, v0 + e2), r of an inner
 *                 subtree the largest |p - p_c| + r_c over its children; both times 1 + 10^-6, rounded up.  A subtree
 *                 without area has N as summed (0 for faces without area), p = the first vertex of its first record
 *                 (inner: its first child's p) and its r.
 *   table         a leaf has no node of its own (it is a code in its parent's child word), so the table has one entry
 *                 per CHILD SLOT of every inner node, entry 2 n + c for child c of node n (node indices as in qnodes,
 *                 all meshes), then one per mesh root: entry 2 nr_nodes + m.  An entry is 8 floats, 32 bytes: N.xyz, r,
 *                 p.xyz, 0: the two 16-byte loads of a visit, aligned.  A missing child's entry is all 0.
 *   walk          depth first from the root's entry, child 0 before child 1.  With d = p - q, L = sqrtf(d . d): when
 *                 L > beta r (strict) and (d . d) L > 0 the subtree adds (d . N) / ((d . d) L) and is not opened; otherwise an inner node's
 *                 children are judged in turn and a leaf's triangles add their Omega in slot order.  One fp32
 *                 accumulator from 0 in that order; w = the sum times fl(1 / 4 pi).  beta = +inf: no subtree is far,
 *                 every leaf is summed.  The same tree, point and beta give the same bytes on every call, whichever
 *                 other points share the launch.  A NaN query gives NaN.
 * vsa_mesh_winding_moments: the table [2 nr_nodes + nr_meshes, 8] f32 of all the meshes of a tracer (qnodes [nr_nodes,
 *   8] u32, tris [nr_tris, 12] f32, mesh_roots [host, nr_meshes]).  Bottom up without parent pointers in the nodes: one
 *   pass writes parent[child], then a thread per child slot that holds a leaf (or nothing) writes its entry and climbs;
 *   at each inner node an integer arrival counter decides: the first arriver leaves, the second (after a device-scope
 *   fence) combines child 0 then child 1 and goes on.  No thread waits for another; no float atomics: two builds give
 *   the same bytes, for any builder's node order.  workspace = vsa_mesh_winding_moments_workspace_bytes(nr_nodes,
 *   nr_meshes) bytes.
 * vsa_winding_number_q: w [nr_meshes, nr_points] f32 of points [nr_points, 3] f32; moment_roots [host, nr_meshes] = each
 *   mesh's root entry.  One lane per point, one-wave workgroups, the stack of entries in LDS ([24 or 48][64] by
 *   max_depth), no scratch.  vsa_winding_number_q_stats: the same walk, counters [3] i64 (device) = entries judged,
 *   exact triangle terms, queries.
 * vsa_signed_distance_w_q: vsa_closest_point_q's outputs with the sign from w: dist = -sqrtf(d2) when w > 1/2, else
 *   +sqrtf(d2); |dist|, slot and bary are vsa_closest_point_q's bits.  A NaN query keeps slot -1 and +inf.
 * vsa_mesh_sdf_grid_w: vsa_mesh_sdf_grid with this sign, for ONE mesh (its root, frame and root entry): grid = the point
 *   query at (x[i], y[j], z[k]) clamped to [-band, band], bit for bit, with or without a band.  A finite band: one lane
 *   per brick takes the UNSIGNED distance d_c at the brick's centre; a brick with d_c > band + (4/3) rho is FAR, skips
 *   the closest-point walk and writes -band where its point's OWN w > 1/2, else +band (w crosses 1/2 away from the
 *   surface, on the membrane that closes a hole: a far brick can hold both signs); the others walk both.  brick_counts
 *   [host, 2] = near, far bricks, through one blocking read of the stream (none with band = +inf).  workspace =
 *   vsa_mesh_sdf_grid_w_workspace_bytes(nx, ny, nz) bytes (may be NULL with band = +inf).
 * vsa_mesh_edge_census: counts [host, 3] = the undirected edges with one face (boundary), with more than two
 *   (non-manifold), and with two faces that traverse them in the same direction (inconsistent winding), over the faces
 *   with a positive finite area (vsa_mesh_pseudonormals' rule), from the sorted edge keys of csrc/mesh_topology.hip.
 *   One blocking read.  workspace = vsa_mesh_edge_census_workspace_bytes(V, F) bytes.
 * VSA_ERR_ARG (before any HIP call): a NULL pointer (bary may be NULL), nr_nodes, nr_tris, nr_points, V, F or an axis
 *   length < 1, nr_meshes outside 1..16, max_depth >= 48, a root outside [0, nr_nodes), a negative root or root entry,
 *   beta <= 1 or NaN, band <= 0 or NaN, a workspace smaller than asked for.  VSA_ERR_UNSUPPORTED: 2 nr_nodes + 16 or
 *   3 F + 3 beyond int32, nr_tris >= 2^27, more than 2^31 - 1 waves or bricks. */
long long vsa_mesh_winding_moments_workspace_bytes(long long nr_nodes, int nr_meshes);
int vsa_mesh_winding_moments(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots, int nr_meshes,
                             long long nr_nodes, long long nr_tris, void* workspace, long long workspace_bytes,
                             float* moments, void* stream);
int vsa_winding_number_q(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots, int nr_meshes,
                         int max_depth, const float* moments, const long long* moment_roots, float beta,
                         const float* points, long long nr_points, float* w, void* stream);
int vsa_winding_number_q_stats(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots, int nr_meshes,
                               int max_depth, const float* moments, const long long* moment_roots, float beta,
                               const float* points, long long nr_points, long long* counters, void* stream);
int vsa_signed_distance_w_q(const uint32_t* qnodes, const float* tris, const int32_t* mesh_roots,
                            const float* mesh_frames, int nr_meshes, int max_depth, const float* moments,
                            const long long* moment_roots, float beta, const float* points, long long nr_points,
                            float* dist, int32_t* slot, float* bary, void* stream);
long long vsa_mesh_sdf_grid_w_workspace_bytes(int nx, int ny, int nz);
int vsa_mesh_sdf_grid_w(const uint32_t* qnodes, const float* tris, int root, const float* frame, int max_depth,
                        const float* moments, long long moment_root, float beta, const float* x, const float* y,
                        const float* z, int nx, int ny, int nz, float band, float* grid, void* workspace,
                        long long workspace_bytes, long long* brick_counts, void* stream);
long long vsa_mesh_edge_census_workspace_bytes(long long nr_verts, long long nr_faces);
int vsa_mesh_edge_census(const float* vertices, long long nr_verts, const int32_t* faces, long long nr_faces,
                         void* workspace, long long workspace_bytes, long long* counts, void* stream);

/* ---- Mesh repair (no counterpart in the reference; csrc/mesh_repair.hip) ----
 * Welding the vertices that are one point and winding every edge-connected component consistently, outward.  The rules
 * are this library's own and UNPINNED, restated in tests/mesh_repair_restated.py.
 *   grouping      rep[i] = the lowest index whose row of three 32-bit words equals row i: three stable radix sorts of
 *                 (word, index), last word first, from iota; the head of a run of equal rows is its lowest index.
 * vsa_mesh_weld: verts [V, 3] f32 and faces [F, 3] i32 (device) to out_verts [V, 3] (the first stats[0] rows written),
 *   out_faces [F, 3] (the first stats[1] rows), out_vertex_map [V] i32 (old -> new), out_face_map [F] i32 (old -> new,
 *   -1: dropped) and stats [host, 4] = vertices out, faces out, degenerate faces dropped, duplicate faces dropped.
 *   tol = 0       two vertices are one iff their three coordinates have equal bits after -0.0 -> +0.0; a vertex with a
 *                 NaN coordinate merges with nothing.  Rows = the coordinate bits, grouped.
 *   tol > 0       two vertices are in one cluster iff a chain of vertices links them whose consecutive members are within
 *                 tol: d2 = ((dx dx + dy dy) + dz dz) <= tol tol in fp64 from the fp32 coordinates, no fused
 *                 multiply-add.  The cell of a vertex is floor(p / tol) per axis in fp64, 21 bits each (offset 2^20),
 *                 packed into 63 bits; (cell, vertex) is sorted; a lane per vertex searches its 27 neighbouring cells
 *                 and hooks itself to every lower vertex within tol (the union-find of csrc/mesh_topology.h: the root
 *                 is the lowest vertex whatever the order).  A vertex with a NaN has no cell and stays alone; a cell
 *                 index outside [-2^20, 2^20) gives VSA_ERR_UNSUPPORTED (counted on the device, seen at the read).
 *                 n vertices in one cell cost n^2 distance tests.
 *   output        a representative (the lowest vertex of its cluster) keeps its own bits: nothing is averaged.  New
 *                 indices ascend with the representative's old index.  Faces are remapped; with drop_degenerate a face
 *                 that names a vertex twice goes; with drop_duplicates a face that stays so far and whose sorted
 *                 triple equals a lower face's goes (the grouping over the sorted triples of all faces).  The others
 *                 keep their order and winding.  Vertices no face names stay.
 *   One blocking read.  stage_ms [host, 4] or NULL: group, vertices, duplicates, faces.
 * vsa_mesh_orient: faces [F, 3] to out_faces [F, 3], out_flipped [F] u8, out_component [F] i32 and stats [host, 5] =
 *   components, faces flipped, components that are not orientable, undecided components, their faces.  faces_uvs
 *   [F, 3, 2] f32 or NULL: the per-corner UVs, written to out_faces_uvs with the flipped faces' corners swapped.
 *   constraints   an undirected edge named by exactly two different faces of positive finite area (vsa_mesh_edge_census'
 *                 faces and manifold edges) ties them: par = 1 iff both traverse it in the same direction.  Node
 *                 2 f + s means face f kept (s = 0) or flipped (s = 1); 2 f is joined with 2 g + par and 2 f + 1 with
 *                 2 g + 1 - par in a union-find over 2 F nodes whose roots are minima.  component[f] = root(2 f) >> 1
 *                 (the lowest face of the component), the relative flip = root(2 f) & 1; root(2 f) = root(2 f + 1):
 *                 the component is not orientable and keeps its faces as they are.
 *   outward       per orientable component, fp64 sums of fixed shape over its faces in ascending order (chunks of 2048
 *                 sorted positions, then the chunks of a component; no float atomics), a face without a finite area
 *                 adding nothing: with N = 1/2 (v1 - v0) x (v2 - v0) after the relative flip, A = |N| and c = ((v0 + v1)
 *                 + v2) / 3: cbar = sum A c / sum A (0 without area); S = sum (Nx dx + Ny dy) + Nz dz, d = c - cbar;
 *                 U = sum A (|c|_1 + |cbar|_1).  S is three times the signed volume of a closed component and positive
 *                 for a sheet whose normals point away from its centroid.  Decided iff |S| > 2^-20 U; a decided
 *                 component with S < 0 (outward = 1; S > 0 with outward = 0) is flipped whole, an undecided one keeps
 *                 the relative orientation.  flipped = relative flip xor the component's; a flipped face is
 *                 (v0, v2, v1).
 *   One blocking read.  stage_ms [host, 5] or NULL: edges, hook, roots, sums, flip.
 * workspace = vsa_mesh_weld_workspace_bytes(V, F) / vsa_mesh_orient_workspace_bytes(V, F) bytes, the caller's.
 * VSA_ERR_ARG (before any HIP call): a NULL pointer (faces_uvs, out_faces_uvs without faces_uvs, and stage_ms may be
 *   NULL), V or F < 1, tol negative, NaN or infinite, a workspace smaller than asked for.  VSA_ERR_UNSUPPORTED: V >= 2^31
 *   or 3 F + 3 (orient: 6 F + 3) >= 2^31, a cell index out of range (and from the queries, a failed rocPRIM size query:
 *   no device). */
long long vsa_mesh_weld_workspace_bytes(long long nr_verts, long long nr_faces);
int vsa_mesh_weld(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces, double tol,
                  int drop_degenerate, int drop_duplicates, void* workspace, long long workspace_bytes,
                  float* out_verts, int32_t* out_faces, int32_t* out_vertex_map, int32_t* out_face_map,
                  long long* stats, float* stage_ms, void* stream);
long long vsa_mesh_orient_workspace_bytes(long long nr_verts, long long nr_faces);
int vsa_mesh_orient(const float* verts, long long nr_verts, const int32_t* faces, long long nr_faces, int outward,
                    const float* faces_uvs, void* workspace, long long workspace_bytes, int32_t* out_faces,
                    float* out_faces_uvs, uint8_t* out_flipped, int32_t* out_component, long long* stats,
                    float* stage_ms, void* stream);

/* ---- Image preparation (the reference's loader, mvdatasets, is absent; csrc/image_prepare.hip) ----
 * A split's decoded image bytes to the float stacks `TensorReel`, `render_and_eval` and the bakers read, in one launch:
 * alpha over a background colour, box subsampling by an integer factor s, and the mask.  The rule is this library's own,
 * restated in tests/datasets_restated.py and UNPINNED.
 *   src  [C, H0, W0, ch] u8, ch in {1, 3, 4} (grey, RGB, RGBA; ch = 4 is read a dword per texel: src 4-byte aligned)
 *   mask [C, H0, W0] u8 or NULL;  bg [host, 3] f32;  1 <= s <= 16;  H = H0 / s, W = W0 / s (the remainder rows and
 *   columns at the bottom and the right are dropped)
 *   rgb  [C, H, W, 3] f32;  out_mask [C, H, W] f32, or NULL when there is neither a mask nor an alpha channel
 * Per output pixel, over its n = s s source texels k (a_k the alpha byte, 255 when ch is 1 or 3; c_k the colour bytes,
 * replicated for ch = 1), with integer sums A = sum a_k, P_c = sum c_k a_k, M = sum mask_k (all below 2^24):
 *   alpha = fl(float(A) / float(255 n)),  prem_c = fl(float(P_c) / float(65025 n))     (correctly rounded divisions)
 *   rgb_c = fl(prem_c + fl(fl(1 - alpha) bg_c))                                         (no fused multiply-add)
 *   out_mask = fl(float(M) / float(255 n)) with a mask, else alpha (ch = 4)
 * so that an opaque texel at s = 1 gives fl(c / 255), a transparent one gives bg, and subsampling averages
 * premultiplied colour (a transparent texel's colour bytes never count).
 * VSA_ERR_ARG (before any HIP call): s outside 1..16, ch not 1 / 3 / 4, a negative size, a NULL src / bg / rgb with
 *   something to do, out_mask without a mask or an alpha channel, a mask without out_mask, a misaligned RGBA src.
 *   VSA_ERR_UNSUPPORTED: more than 2^31 - 1 blocks (C H ceil(W / 256)). */
int vsa_images_prepare(const uint8_t* src, const uint8_t* mask, int C, int H0, int W0, int ch, int s, const float* bg,
                       float* rgb, float* out_mask, void* stream);

/* ---- Mesh crossings (no counterpart in the reference; csrc/mesh_cross.hip, csrc/cross_walk.h) ----
 * Which faces of two meshes cross -- pass through one another -- and which faces of one mesh cross each other.  Exact in
 * the sense that every face pair is decided by one restated rule, not sampled.  The reference has no such stage: the
 * rule below is this library's own, restated in tests/mesh_intersect_restated.py and UNPINNED.
 *   inputs        two triangles A = (A0, A1, A2), B = (B0, B1, B2): the fp32 bits of the meshes' VERTEX ARRAYS converted
 *                 to fp64 (not the tree's records v0, e1, e2: their rounded edges would give a vertex two faces share
 *                 different bits in each, and the rule leans on shared vertices being bit-equal).
 *   arithmetic    fp64, in the order written, no contraction.  orient(a, b, c, d) = det[a - d; b - d; c - d] along its
 *                 first row: p = a - d, q = b - d, r = c - d;  m0 = q.y r.z - q.z r.y,  m1 = q.x r.z - q.z r.x,
 *                 m2 = q.x r.y - q.y r.x;  orient = (p.x m0 - p.y m1) + p.z m2.
 *   determinants  sB[i] = orient(B0, B1, B2, A_i) (the side of A's vertex i of B's plane), sA[j] = orient(A0, A1, A2,
 *                 B_j), e[i][j] = orient(A_i, A_{i+1}, B_j, B_{j+1}), indices mod 3: fifteen, each computed once.
 *   crossing      edge i of A pierces B iff sB[i] and sB[i+1] are strictly opposite (one < 0, the other > 0) and
 *                 e[i][0..2] are all >= 0 or all <= 0; edge j of B pierces A iff sA[j], sA[j+1] are strictly opposite
 *                 and e[0..2][j] are all >= 0 or all <= 0.  A and B cross iff one of the six edges pierces and none of
 *                 the six sides is NaN.  Signs only: a determinant whose sign no live condition reads may be skipped.
 *   it follows    a vertex two faces share by equal bits has side exactly 0, so faces that share an edge never cross and
 *                 faces that share one vertex cross only when the opposite edge of one goes through the other; no index
 *                 is compared, so a triangle soup gives what its welded mesh gives; coplanar pairs, touching without
 *                 passing through, duplicate faces and zero-area faces are not crossings; a face with a NaN coordinate
 *                 crosses nothing (without the clause on the sides, the edge between its two other vertices could).
 *   segment       the piercing point of edge p q against the other triangle's plane is p + t (q - p) per component,
 *                 t = s_p / (s_p - s_q).  The pair's segment is the point of the first and of the last piercing edge in
 *                 the order A's edges 0, 1, 2, B's edges 0, 1, 2.  Generically exactly two edges pierce; where a third
 *                 does (an edge through an edge), first and last may be the same point.
 *   walk          one lane per query face, one wave per workgroup, an LDS stack; a child of the tree mesh's q16 node is
 *                 entered iff its u16 box overlaps (closed) the box of the query triangle in the tree's grid, g = (x -
 *                 lo) / step + 1 of the fp32 minimum and maximum of the three vertices.  The boxes' outward margin of at
 *                 least one unit covers the three roundings of g (below 2^-6 of a unit wherever g is compared with a u16
 *                 coordinate, at any distance): no crossing pair is missed, and the result is that of brute force over
 *                 all pairs.  At a leaf: slot -> the record's face id -> tree_faces row -> tree_vertices, then the rule.
 *   self mode     (self_mode = 1: the query arrays are the tree's) face i against itself is skipped; a pair is evaluated
 *                 with the lower face id as A whichever lane finds it; count_query[i] = the number of partners of face
 *                 i; only pairs with j > i are emitted (offsets and total count those).
 * qnodes / tris / max_depth as vsa_trace_q takes them; root, frame [host, 6 floats]: the tree mesh's.  query_order [Fq]
 * i32 or NULL: lane i takes query face query_order[i] (a permutation that puts nearby faces into one wave; the results
 * do not depend on it).  A face with a vertex index outside its vertex array, and a record whose id is outside 0 .. Ft -
 * 1, cross nothing; nothing outside the arrays is read.
 * vsa_mesh_cross_count: count_query [Fq] i32 = the tree faces each query face crosses; count_tree [Ft] i32 = the query
 *   faces that cross each tree face (one integer atomicAdd per crossing; NULL and unused in self mode); offsets [Fq] i32
 *   = the exclusive scan (rocPRIM) of the pairs each query face emits; total [device, 1] i64 = their sum (integer
 *   atomics), the one word a caller reads back.
 * vsa_mesh_cross_emit: the same walk with those offsets and nr_pairs = that total (>= 1): the pairs (query face, tree
 *   face) as 64-bit keys at the query's offset, sorted ascending by a radix sort (csrc/mesh_topology.hip) -> pairs
 *   [nr_pairs, 2] i64, segments [nr_pairs, 2, 3] f64 (or NULL) carried along.  A slot the walk leaves unwritten (offsets
 *   that are not this input's) comes out as (2^32 - 1, 2^32 - 1) at the end; nothing beyond nr_pairs is written.
 * workspace = vsa_mesh_cross_workspace_bytes(nr_query_faces, nr_pairs (0 for the count pass), segments != 0) bytes.
 * VSA_ERR_ARG (before any HIP call): a NULL pointer (query_order, segments, and count_tree in self mode may be NULL),
 *   root < 0, max_depth >= 48, a vertex or face count < 1, self_mode outside 0..1 or with counts that differ, nr_pairs <
 *   1 (emit) or < 0 (query); a workspace smaller than asked for.  VSA_ERR_UNSUPPORTED: 3 F + 3 or V beyond 2^31 - 1,
 *   nr_pairs beyond 2^31 - 1 (and from the query, a failed rocPRIM size query: no device). */
long long vsa_mesh_cross_workspace_bytes(long long nr_query_faces, long long nr_pairs, int segments);
int vsa_mesh_cross_count(const uint32_t* qnodes, const float* tris, int root, const float* frame, int max_depth,
                         const float* tree_vertices, long long nr_tree_verts, const int32_t* tree_faces,
                         long long nr_tree_faces, const float* query_vertices, long long nr_query_verts,
                         const int32_t* query_faces, long long nr_query_faces, const int32_t* query_order,
                         int self_mode, int32_t* count_query, int32_t* count_tree, int32_t* offsets, long long* total,
                         void* workspace, long long workspace_bytes, void* stream);
int vsa_mesh_cross_emit(const uint32_t* qnodes, const float* tris, int root, const float* frame, int max_depth,
                        const float* tree_vertices, long long nr_tree_verts, const int32_t* tree_faces,
                        long long nr_tree_faces, const float* query_vertices, long long nr_query_verts,
                        const int32_t* query_faces, long long nr_query_faces, const int32_t* query_order,
                        int self_mode, const int32_t* offsets, long long nr_pairs, long long* pairs, double* segments,
                        void* workspace, long long workspace_bytes, void* stream);

/* ---- Shell untangling (no counterpart in the reference; csrc/shell_untangle.hip) ----
 * Move the vertices of a shell M until it lies on one side of a fixed shell X and none of its faces crosses X.  Faces,
 * UVs, vertex count and order are untouched.  The reference has no such stage: the rule below is this library's own,
 * restated in tests/shell_untangle_restated.py and UNPINNED.
 *   state         every vertex of M carries an integer level, 0 at round 0.  side s = +1 (M moves outward: it is to
 *                 lie outside X) or -1 (inward).
 *   project       for every vertex p of M, referenced by a face or not: the query of vsa_signed_distance_q against X
 *                 (moments = NULL; the pseudonormal sign) or of vsa_signed_distance_w_q (moments, moment_root, beta: the
 *                 winding sign) gives the signed dist, the residual r = p - closest point and the table's entry n of
 *                 the closest feature.  m = margin * 2^min(level, max_level) (fp32, exact).  The vertex is VIOLATED iff
 *                 it has a closest record and s dist < m (fp32; a NaN never is).  A violated vertex moves to p + t g per
 *                 component, a multiply then an add without contraction: t = s (1.25f m) - dist;  g = r / |dist|,
 *                 negated when dist < 0, if |dist| > 0, else g = n / sqrt(dot3(n, n)).  A g with a non-finite component
 *                 leaves the vertex where it is: it counts as stuck, not as moved.  (1.25: a step that lands exactly on
 *                 the margin flickers on the last ulp.)
 *   count         the crossing face pairs P of M's faces against X: vsa_mesh_cross_count with M as the query mesh,
 *                 after the project step.
 *   stop          moved == 0 and P == 0: the pair has converged.
 *   escalate      otherwise every vertex of every face of M with a non-zero count gets level += 1, once per round
 *                 however many of its faces cross; the next round follows.
 * vsa_shell_untangle_project: one lane per vertex, one wave per workgroup, the closest-point walk of X's q16 tree with an
 *   LDS stack; vertices [nr_verts, 3] f32 are M's, moved IN PLACE; dist, slot and weights never reach memory.  state
 *   [device, 4] i64: word 0 = moved, word 1 = stuck, word 2 = the bits of the largest |t| of a moved vertex (a non-negative
 *   float: integer atomicMax), all three cleared by this call and written with one integer atomic per wave; word 3 is not
 *   touched (hand &state[3] to vsa_mesh_cross_count as its `total`, and one read of 32 bytes ends the round).  round = 0
 *   also clears the workspace: levels 0, stamps -1.  table / table_face_base: X's pseudonormals, needed with either sign
 *   (a vertex on X moves along n).  side: +1 or -1.
 * vsa_shell_untangle_escalate: one lane per face of M; count_query [nr_faces] i32 is the count pass's.  A crossing face
 *   raises the stamp of its three vertices to `round` (integer atomicMax); the lane that raised it adds 1 to the level.
 *   A face with an index outside 0 .. nr_verts - 1 is skipped.  `round` must increase from call to call.
 * workspace = vsa_shell_untangle_workspace_bytes(nr_verts) bytes, kept by the caller across the rounds of one pair: the
 *   levels [nr_verts] i32 at offset 0, then the stamps.
 * No float atomics; the same inputs give the same bytes.
 * VSA_ERR_ARG (before any HIP call): a NULL pointer (moments may be NULL), root < 0, max_depth >= 48, a count < 1, side
 *   not +-1, margin not a positive finite number, max_level outside 0 .. 30, round < 0, moments with moment_root < 0 or
 *   beta <= 1, a workspace smaller than asked for.  VSA_ERR_UNSUPPORTED: nr_verts or 3 nr_faces + 3 beyond 2^31 - 1. */
long long vsa_shell_untangle_workspace_bytes(long long nr_verts);
int vsa_shell_untangle_project(const uint32_t* qnodes, const float* tris, int root, const float* frame, int max_depth,
                               const float* table, long long table_face_base, const float* moments,
                               long long moment_root, float beta, float* vertices, long long nr_verts, int side,
                               float margin, int max_level, int round, void* workspace, long long workspace_bytes,
                               long long* state, void* stream);
int vsa_shell_untangle_escalate(const int32_t* count_query, const int32_t* faces, long long nr_faces,
                                long long nr_verts, int round, void* workspace, long long workspace_bytes, void* stream);

/* ---- Shell rasterization (no counterpart in the reference's tree; csrc/shell_raster.hip) ----
 * The hit records of vsa_trace_q for every sample of one camera, from screen-space bins instead of BVH walks: the same
 * pinhole ray (csrc/pinhole.h) and the same triangle test (csrc/trace_walk.h tri_test: smallest t, ties to the smallest
 * original face id, a hit iff t > t_min) over, per 8 x 8-sample tile, a list that holds every triangle one of the
 * tile's rays can pass.  The closest hit does not depend on the order or the length of such a list, so the records
 * equal the trace's bit for bit.  The bin rule below is this library's own, restated in tests/rasterize_restated.py and
 * UNPINNED.  No nodes are read: any builder, either node format.
 *   tris          the tracer's leaf-ordered records [nr_slots, 12] f32 (v0.xyz, id | e1.xyz, - | e2.xyz, -);
 *                 mesh_tri_offset / mesh_nr_tris [host, nr_meshes] i32: shell k owns slots offset .. offset + nr - 1.
 *   camera        c2w [3, 4] = [R | t], intrinsics K [3, 3] and intrinsics_inv [3, 3], f32 on the device; any pinhole K
 *                 (skew and an off-centre principal point included).  Rays come from intrinsics_inv, boxes from K.
 *   samples       the grid of vsa_face_view_counts: sample (i, j) of pixel (col, row) goes through x = col + (i + 0.5f)
 *                 / s, y = row + (j + 0.5f) / s; s = 1 is the unjittered ray of vsa_camera_rays bit for bit.  Sample
 *                 (X, Y) = (col s + i, row s + j) of the (s H) x (s W) grid belongs to tile (X / 8, Y / 8).
 *   bin rule      fp32, in the order written, no contraction.  Per slot: a = v0, b = v0 + e1, c = v0 + e2; per vertex
 *                 w = v - t, p = ((R0i w0 + R1i w1) + R2i w2) for i = x, y, z (p = R^T w).  z_g = 1e-4f max(1, |t.x|,
 *                 |t.y|, |t.z|).
 *                 dropped      a vertex coordinate is not finite: in no list (tri_test accepts nothing on NaN).
 *                 behind       all three p.z < -z_g: in no list.  (A hit has camera z = t d_z > 0 for t > t_min >= 0.)
 *                 straddling   neither behind nor in front, or a projection that is not finite or has h.w <= 0: the
 *                              face goes to EVERY tile of its shell.  It is kept once, in a list per shell that every
 *                              tile's wave walks after its own, not copied into the tiles' lists.
 *                 in front     all three p.z > z_g.  h = K p (rows as (Ki0 p.x + Ki1 p.y) + Ki2 p.z), u = h.x / h.w,
 *                              v = h.y / h.w in pixels.  The box of the three (u, v), grown by ONE PIXEL on every side,
 *                              in samples: X0 = floor((min u - 1) s), X1 = floor((max u + 1) s), Y likewise; off the
 *                              image (X1 < 0, X0 > s W - 1, ...) it is in no list, else clamped to [0, s W - 1] x
 *                              [0, s H - 1] in float, converted, and the face is in the list of every tile from
 *                              (X0 / 8, Y0 / 8) to (X1 / 8, Y1 / 8).
 *                 The pixel is part of the rule: tri_test is inexact and accepts rays just outside the exact triangle
 *                 (measured: at most 1.9e-6 pixels outside the unexpanded box; DESIGN 35 has the argument).
 *   stats         [host, 4] long long: faces behind, faces straddling, faces binned (in front, in at least one tile's
 *                 list), pairs = the (tile, slot) entries of all tiles' lists (straddling faces not among them).
 * vsa_shell_raster_setup: the setup pass (one lane per slot: class, box, one integer atomic per tile touched), a scan
 *   of the (shell, tile) counters, and one blocking read of `stats`.  t_min is only checked.
 * vsa_shell_raster_draw: the fill pass (one integer atomic per pair; the order inside a list is the schedule's and does
 *   not matter) and the raster pass (one wave per (shell, tile), one lane per sample, lanes past the image edge masked;
 *   no stack, no LDS, no scratch).  Same arguments and workspace as the setup call before it; pairs [device, nr_pairs]
 *   i32 is the caller's, nr_pairs = stats[3] (pairs may be NULL when it is 0).  May be repeated after one setup.
 *   hit_t [K, N] f32 (0 for a miss), hit_slot [K, N] i32 (global slot, -1 = miss), hit_uv [K, N, 2] f32, as vsa_trace_q
 *   writes them; N = H W s^2, pixel-major, a pixel's samples consecutive, j outer, i inner.  rays_d [N, 3] f32 or NULL:
 *   the samples' directions (the origin is t).  stage_ms [host, 2] or NULL: device ms of the fill and the raster pass
 *   (synchronises).
 * workspace = vsa_shell_raster_workspace_bytes(nr_slots, nr_meshes, height, width, supersample) bytes, the caller's:
 *   20 bytes per slot and 12 per (shell, tile) plus the scan's storage.
 * Integer atomics only; the same inputs give the same bytes.
 * VSA_ERR_ARG (before any HIP call): a NULL pointer (rays_d, stage_ms and, with nr_pairs = 0, pairs may be NULL),
 *   nr_slots < 1, nr_meshes outside 1 .. 16, a slot range outside 0 .. nr_slots, height or width < 1, supersample outside
 *   1 .. 8, t_min < 0 or not finite, H W s^2 >= 2^31, nr_pairs < 0, a workspace smaller than asked for.
 *   VSA_ERR_UNSUPPORTED: more than 2^31 - 1 pairs (setup: after the read; faces that each cover the whole image make
 *   F x tiles pairs), or K x tiles + 1 beyond 2^31 - 1. */
long long vsa_shell_raster_workspace_bytes(long long nr_slots, int nr_meshes, int height, int width, int supersample);
int vsa_shell_raster_setup(const float* tris, long long nr_slots, const int32_t* mesh_tri_offset,
                           const int32_t* mesh_nr_tris, int nr_meshes, const float* c2w, const float* intrinsics,
                           const float* intrinsics_inv, int height, int width, int supersample, float t_min,
                           void* workspace, long long workspace_bytes, long long* stats, void* stream);
int vsa_shell_raster_draw(const float* tris, long long nr_slots, const int32_t* mesh_tri_offset,
                          const int32_t* mesh_nr_tris, int nr_meshes, const float* c2w, const float* intrinsics,
                          const float* intrinsics_inv, int height, int width, int supersample, float t_min,
                          const void* workspace, long long workspace_bytes, long long nr_pairs, int32_t* pairs,
                          float* hit_t, int32_t* hit_slot, float* hit_uv, float* rays_d, float* stage_ms, void* stream);

/* ---- Mesh smoothing (no counterpart in the reference; csrc/mesh_smooth.hip) ----
 * Taubin's lambda | mu fairing of one mesh: vertices move, and only vertices, so faces, UVs, vertex count and order are
 * untouched.  With guard meshes the result crosses no guard face that the input did not cross.  The reference never
 * smooths: the rule below is this library's own, restated in tests/mesh_smooth_restated.py and UNPINNED.  fp32 in the
 * order written, no contraction; fp32 division is correctly rounded.  P [V, 3] f32, faces [F, 3] i32 with every index in
 * 0 .. V - 1 (as vsa_simplify requires).
 *   ring          of vertex v: the corner slots 3 f + c with faces[f, c] == v in ascending slot order (the order of the
 *                 stage's (vertex, face) sort); a face that names v twice is in it twice.
 *   boundary      v is a boundary vertex iff it is an endpoint of an undirected edge key (min, max of a corner and the
 *                 next) that occurs exactly once among the 3 F keys.  With fix_boundary != 0 a boundary vertex never
 *                 moves; a vertex with an empty ring never moves.
 *   half-step     with weight w, for every vertex that may move: acc = 0; for each ring slot in order, componentwise,
 *                 acc = (acc + P[a]) + P[b] with a = faces[f, (c + 1) % 3], b = faces[f, (c + 2) % 3]; cen = acc /
 *                 (float)(2 slots); Q[v] = P[v] + w (cen - P[v]) (a subtract, a multiply, an add).  A Q[v] with a
 *                 component that is not finite is dropped: the vertex keeps P[v] and counts as stuck.  Every vertex reads
 *                 P and writes Q (Jacobi): src and dst are two buffers.
 *   iteration     a half-step with lambda in (0, 1] (half = 0), then one with mu <= 0 (half = 1) on its result; mu = 0
 *                 is plain Laplacian smoothing.
 *   guard         once per iteration, P = the positions before it, Q after it; rounds r = 0, 1, ...:
 *                 a face of the mesh is BAD iff one of its vertices differs in bits between Q and P and it crosses, as A,
 *                 a face of a guard, as B, by the rule of "Mesh crossings" (tri_cross of csrc/cross_walk.h; a face with
 *                 an index outside its vertex array is no face).  Every vertex of a bad face that still differs from P
 *                 gets its bits of P back: reverted.  The rounds end with the first that reverts nothing; the reverted
 *                 set only grows, so they end.  Afterwards every face that crosses a guard face has its three vertices
 *                 where they were before the iteration: the crossing pairs with a guard are a subset of the input's.
 *                 The verdict is an OR over (face, guard face) pairs: it does not depend on a guard's tree or builder.
 * vsa_mesh_smooth_prepare: once per mesh: the rings, the sorted edge keys and the boundary flags into the workspace,
 *   stamps -1.  The flags [V] i32 (0 / 1) are at offset 0 of the workspace.
 * vsa_mesh_smooth_step: one half-step src -> dst, one lane per vertex, the ring summed by that lane alone in ring order.
 *   half = 0 takes weight in (0, 1], half = 1 weight <= 0.  *state (device, i64) += the stuck vertices, one integer
 *   atomic per wave; it is the caller's to clear.  No read, no synchronisation.
 * vsa_mesh_smooth_guard: one lane per face, one wave per workgroup; before = P, after = Q.  A face with a vertex that
 *   differs from P walks each guard's q16 tree (LDS stack) until its first crossing and then stamps its three vertices
 *   with `round`.  The guard block is vsa_simplify_guarded's, arrays and errors.  `round` must increase by one from call to call after
 *   one prepare (across iterations too): the stamps are never cleared.  first_round = the `round` of this iteration's
 *   first call: in a later round only a face with a vertex stamped in the round before is judged again (the others
 *   have not changed since they were found clear), which changes no verdict.
 * vsa_mesh_smooth_revert: one lane per vertex: a vertex stamped `round` whose bits in `after` differ from `before` gets
 *   them back.  *state (device, i64) += the vertices restored, one integer atomic per wave; the caller reads it, the
 *   one blocking read of a round.
 * workspace = vsa_mesh_smooth_workspace_bytes(V, F) bytes, kept by the caller from prepare to the last call: 16 bytes
 *   per vertex and 96 per face plus rocPRIM's temporary storage.
 * No float atomics; the same inputs give the same bytes.
 * VSA_ERR_ARG (before any HIP call): a NULL pointer, src == dst, V or F < 1, a workspace smaller than asked for, a
 *   weight that is not finite, half = 0 with a weight outside (0, 1], half = 1 with a weight > 0, half not 0 or 1,
 *   the guard block's cases, round < 0, first_round < 0 or > round.  VSA_ERR_UNSUPPORTED: V >= 2^31 or 3 F + 3 >= 2^31
 *   (of the mesh or of a guard), or a failed size query. */
long long vsa_mesh_smooth_workspace_bytes(long long nr_verts, long long nr_faces);
int vsa_mesh_smooth_prepare(const int32_t* faces, long long nr_verts, long long nr_faces, void* workspace,
                            long long workspace_bytes, void* stream);
int vsa_mesh_smooth_step(const float* src, float* dst, const int32_t* faces, long long nr_verts, long long nr_faces,
                         int half, float weight, int fix_boundary, const void* workspace, long long workspace_bytes,
                         long long* state, void* stream);
int vsa_mesh_smooth_guard(const float* before, const float* after, const int32_t* faces, long long nr_verts,
                          long long nr_faces, int nr_guards, const uint32_t* const* guard_qnodes,
                          const float* const* guard_tris, const int32_t* guard_roots, const float* guard_frames,
                          const int32_t* guard_max_depths, const float* const* guard_vertices,
                          const long long* guard_nr_verts, const int32_t* const* guard_faces,
                          const long long* guard_nr_faces, int first_round, int round, void* workspace,
                          long long workspace_bytes, void* stream);
int vsa_mesh_smooth_revert(const float* before, float* after, long long nr_verts, long long nr_faces, int round,
                           const void* workspace, long long workspace_bytes, long long* state, void* stream);

/* ---- Texture transfer (no counterpart in the reference; csrc/texture_transfer.hip) ----
 * The baked 8-bit SH textures of a stack of K source shells carried onto K destination shells with other faces and
 * other per-corner UVs: the planes of "Texture export / import" in, planes of the same layout at the destination's
 * per-degree resolutions out.  The rule is this library's own, restated in tests/texture_transfer_restated.py and
 * unpinned.  Everything is per shell s and SH degree d; R = the source's tex_res[d], R' = the destination's.  fp32,
 * one rounding per operation, in the order written (the build compiles without contraction).
 *   texel centre  pixel (row r, column c) of a plane is read by the baked shade with both lerp fractions zero at
 *                 uv = ((c + 0.5) / R, (r + 0.5) / R): nt_footprint's lerp branch gives i0 = floor(R - v R - 0.5),
 *                 j0 = floor(u R - 0.5), its corner 0 is texel (iy, ix) = (j0, i0), and the orientation rule above
 *                 stores texel (iy, ix) at pixel (R-1-ix, iy); so R - v R - 0.5 = R-1-r and u R - 0.5 = c.  (Exact
 *                 where R is a power of two; elsewhere the fractions are a rounding of zero.)  In TEXEL UNITS (uv
 *                 times R') the centre is (c + 0.5, r + 0.5): row r runs along v, column c along u, the orientation
 *                 of vsa_atlas_rasterize.
 *   uv record     of a destination face: its corners in texel units, x_k = u_k * (float)R', y_k = v_k * (float)R',
 *                 as a record of "Mesh distance" with z = 0: v0 = (x_0, y_0, 0), e1 = (x_1 - x_0, y_1 - y_0, 0), e2
 *                 alike.
 *   projection    of a texel-unit point (qx, qy) onto a uv record: closest_on_triangle of (qx, qy, 0) gives (d2, u, v);
 *                 where its region is the interior, d2 = 0 (the point is its own nearest point; the residual the
 *                 chain forms there is the rounding of u and v).  A zero-area uv triangle falls through as there.
 *   inside        a texel centre lies INSIDE face f iff f covers texel (i, j) = (c, r) by the rule of "UV atlas", raster
 *                 (corners snapped in fp64 to 1/256 texel, int64 edge functions, top-left rule, snapped area > 0):
 *                 vsa_atlas_rasterize's rule, restated, so that the two stages agree texel for texel.  The projection
 *                 onto the exact triangle alone differs from it within the snapping step.
 *   ownership     face f is a candidate of texel (r, c) iff the centre lies inside it (its d2 is 0 then) or the
 *                 projection of the centre onto it has d2 <= reach * reach (a NaN d2 fails).  A face with a uv or a
 *                 vertex that is not finite is a candidate of nothing.  The owner is the minimum over (centre not
 *                 inside, bits of d2, face id): a texel whose centre lies inside a face belongs to the lowest such
 *                 face, vsa_atlas_rasterize's face_id.  The owned barycentrics are the projection's (u, v) in every
 *                 case.  A texel with d2 = 0 is COVERED.  No candidate: UNOWNED.
 *   samples       samples = S in 1..4; sample n = b S + a (a, b in 0..S-1) of texel (r, c) is the texel-unit point
 *                 qx = ((float)c + 0.5) + (((float)a + 0.5) / (float)S - 0.5), qy alike with r and b, projected onto
 *                 the owner's uv record (S = 1: the centre itself).  Its 3-D point is p = (v0 + u e1) + v e2 per
 *                 component on the destination face's record (v0, e1 = v1 - v0, e2 = v2 - v0), vsa_surface_sample's
 *                 expression.
 *   source lookup the closest point of source shell s to p by the walk of "Mesh distance" (slot, weights and d2 are
 *                 vsa_closest_point_q's bits); uv = nt_interp_uv of that slot's per-corner uvs; nt_footprint(uv, R,
 *                 anchor as the source plan says) gives (i0, j0, fx, fy).  Corner k = 2 ky + kx reads texel (iy, ix) =
 *                 (clamp(j0 + ky, 0, R-1), clamp(i0 + kx, 0, R-1)), i.e. pixel (R-1-ix, iy), with weight
 *                 (kx ? fx : 1 - fx) * (ky ? fy : 1 - fy) -- vsa_nt_import_planes' clamp-to-edge apron; under anchor
 *                 all four corners are texel (j0, i0).  Per channel: acc = 0; acc = acc + lut[byte_k] * w_k for k =
 *                 0..3; the sample's coefficient = fp16(acc).  lut[q] = fp16(sh_lo + fp16(sh_span * fp16(q / 255))).
 *                 A p without a closest record (not finite) contributes nothing and counts as far.
 *   resolve       x = (the sample coefficients added in sample order to 0) * (1 / ((float)S * (float)S)); the stored
 *                 byte is the q in 0..255 with the smallest |lut[q] - x| (one fp32 subtract), the lowest such q.  A
 *                 stored byte therefore survives a fetch with zero fractions.  R, G, B = colour channel 0..2 of
 *                 coefficient i, A = alpha coefficient i; A = 255 on a shell without an alpha model.  Unowned texels:
 *                 R = G = B = 0, A = 0 (255 without an alpha model).
 *   report        per shell, TT words u64 [8]: 0 owned texels, 1 covered texels, 2 samples (owned * S^2), 3 the bits
 *                 of the largest d = sqrt(d2) of a sample's closest point (fp32, zero-extended), 4 the samples with
 *                 d > max_distance or without a closest record, 5 the bits of the fp64 sum of (double)d2: per lane in
 *                 sample order, per 8 x 8 tile (lane = 8 (r % 8) + c % 8) by the butterfly s += s[lane ^ m], m = 32,
 *                 16, .. 1, then the tiles in row-major order in vsa_surface_distance's shape (lane t of 1024 adds
 *                 tiles [t c, (t + 1) c), c = ceil(tiles / 1024); lane 0 adds the 1024 sums in order).
 * reach: every texel the shade can read for a hit inside a uv triangle has its centre closer than 1 texel to the hit on
 *   each axis, hence closer than sqrt(2) to the triangle: with reach >= 1.5 it has an owner.
 * vsa_textransfer_owners: the owner words of every shell at one resolution into the workspace, one wave per face over
 *   the face's uv box grown by reach, one 64-bit atomicMin per candidate pair of the word (bit 63: centre not inside;
 *   bits 32..62: d2; bits 0..31: face).
 *   dst_uvs [F, 3, 2], dst_recs [F, 12] (v0.xyz, - | e1.xyz, - | e2.xyz, -; 16-byte aligned) hold the K shells' faces
 *   one after the other, shell s the rows face_base[s] .. face_base[s + 1] - 1 (face_base: host, [K + 1], from 0).
 * vsa_textransfer_owner_fields: shell `shell`'s words as face [R', R'] i32 (-1: unowned), bary [R', R', 2], d2 [R', R']
 *   (unowned: 0 and +inf).
 * vsa_textransfer_planes: degree `degree` of every shell after vsa_textransfer_owners at dst_tex_res[degree] with the
 *   same workspace: a wave per 8 x 8 tile, the walk's stack in LDS.  src_planes / dst_planes are whole plane buffers
 *   (vsa_nt_planes_bytes of the source plan; the same with dst_tex_res), 16-byte aligned; the tree arguments are
 *   vsa_closest_point_q's, nr_meshes = the plan's nr_shells; src_face_uvs [slots, 6] in the order of tris; stats
 *   [K, 8] u64 is cleared and written.  No float atomics: the same inputs give the same bytes.
 * workspace = vsa_textransfer_workspace_bytes(K, R') bytes, 16-byte aligned: 8 R'^2 per shell and 8 per tile.
 * VSA_ERR_ARG (before any HIP call): a NULL pointer, misalignment, K outside 1..16, a resolution outside 1..16384, a
 *   shell without faces, a short workspace, reach negative, NaN or above 64, samples outside 1..4, a NaN max_distance,
 *   a degree outside the plan's, nr_meshes != nr_shells, wrong planes_bytes, a tree deeper than the stack.
 *   VSA_ERR_UNSUPPORTED: 2^31 faces or more, alpha_degrees != rgb_degrees, row_format != 0. */
long long vsa_textransfer_workspace_bytes(int nr_shells, int dst_res);
int vsa_textransfer_owners(const float* dst_uvs, const float* dst_recs, const long long* face_base, int nr_shells,
                           int dst_res, float reach, void* workspace, long long workspace_bytes, void* stream);
int vsa_textransfer_owner_fields(const void* workspace, long long workspace_bytes, const float* dst_uvs,
                                 const long long* face_base, int nr_shells, int shell, int dst_res, int32_t* face,
                                 float* bary, float* d2, void* stream);
int vsa_textransfer_planes(const vsa_nt_plan* src_plan, int degree, const uint8_t* src_planes,
                           long long src_planes_bytes, const uint32_t* qnodes, const float* tris,
                           const int32_t* mesh_roots, const float* mesh_frames, int nr_meshes, int max_depth,
                           const float* src_face_uvs, const float* dst_uvs, const float* dst_recs,
                           const long long* face_base, const int32_t* dst_tex_res, int samples, float max_distance,
                           void* workspace, long long workspace_bytes, uint8_t* dst_planes,
                           long long dst_planes_bytes, unsigned long long* stats, void* stream);

/* ---- Texture fit (no counterpart in the reference; csrc/texel_fit.hip) ----
 * Adam whose parameters are the 8-bit texel rows of a baked bank: what lets a baked scene (a LOD above all) be fitted
 * to target views through vsa_nt_shade_fwd(act_out) -> vsa_composite_dense_fwd_bwd_l1 -> vsa_nt_shade_bwd.  The rule
 * is this library's own, restated in tests/texture_fit_restated.py, which the step equals BIT FOR BIT in p, m, v,
 * texels, grad_rows and stats; unpinned against the reference, which has no such stage.
 *   state     p, m, v: fp32 arrays indexed like texels / grad_rows (row_base[last] * 4 elements; vsa_texel_fit_state_bytes
 *             is the bytes of ONE of them).  p in [0, 1] is the master of one texel-row element in units of q / 255, the
 *             quantity vsa_nt_shade_bwd differentiates (round = straight-through estimator); m, v are Adam's moments.
 *             Only INTERIOR texels own state: the one-texel apron does not exist on disk (vsa_nt_import_planes clamps
 *             it to the edge), so apron texel (ay, ax) of the (R+2)^2 domain FOLDS INTO interior texel
 *             (clamp(ay, 1, R), clamp(ax, 1, R)): 1 apron texel per plain edge texel, 3 per corner, 8 for R = 1.
 *             Elements the launches never reach (apron rows, segment padding) keep what the caller put there.
 *   rows      found through slot_of / seg_start / row_base as vsa_nt_export_planes finds them; a texel whose slot lies
 *             outside its segment is skipped (nothing read, nothing written), as an interior texel and as an apron texel.
 *   init      per interior texel: p = (float)byte / 255.0f (one division), m = v = 0; then every apron row of `texels`
 *             becomes the row of the interior texel it folds into.  A bank out of bake() holds the network's values in
 *             the apron: this makes it what a write_scene -> load_scene round trip gives.
 *   step      per interior texel and per quad (4 elements):
 *     fold    g = 0; the quad's own f16 gradients converted to fp32 are added, then those of the apron texels that fold
 *             into the texel, in row-major (ay, ax) order: fp32, one rounding per add.  A gradient quad whose 64 bits
 *             are all zero is neither added nor stored to.  Then g = g * inv_grad_scale; an element that is not finite
 *             counts in stats[1] and is taken as 0.
 *     consume every other gradient quad read is reset to zero bits, idle or not: grad_rows is all zero wherever the
 *             step reads it, vsa_nt_mlp_bwd's contract with that buffer.
 *     lazy    a quad whose four g are all zero (either sign) is IDLE: p, m, v and the bytes are neither read nor
 *             written, the moments do not decay (SparseAdam's rule at the granularity of vsa_adam_step's idle skip);
 *             bias correction uses the global `step`.
 *     update  vsa_adam_step's formulas, operation order and host-side coefficients (step_size = (float)(lr / (1 -
 *             beta1^step)), inv_bc2_sqrt = (float)(1 / sqrt(1 - beta2^step)), both formed in double) with grad_scale 1:
 *               m = m + (1 - beta1) * (g - m);  v = v * beta2 + ((1 - beta2) * g) * g;
 *               p = p - step_size * (m / (sqrtf(v) * inv_bc2_sqrt + eps));
 *             an element with !(0 <= p <= 1) counts in stats[3]; p = fminf(fmaxf(p, 0), 1); byte = (int)rintf(255.0f * p).
 *             IEEE division and square root, no contraction.
 *     tie     the four bytes are stored to the texel's own quad and to that quad of every apron row that folds into it:
 *             after any number of steps the apron equals its clamped interior.
 *     stats   u64 [4], cleared by the call: 0 quads updated, 1 gradient elements that were not finite, 2 bytes of
 *             interior texels that changed, 3 elements clamped.  Integer atomics, at most one per workgroup and counter.
 * Given its inputs the step is deterministic.  What feeds it is not: vsa_nt_shade_bwd adds f16 atomically, so two fits
 * of the same scene to the same views need not give the same bytes.
 * Elements of shells without an alpha model and the rows' padding receive no gradient from vsa_nt_shade_bwd and are
 * therefore idle for ever; nothing treats them specially.
 * One lane per (interior texel, quad) in domain (= slot) order: 8-byte gradient, 16-byte p / m / v and 4-byte texel
 * accesses; no scratch, and no LDS but 64 bytes for the counters.  An idle quad costs its 8 gradient bytes; a live one
 * 116 (8 + 8 gradient, 3 x 32 state, 4 + 4 bytes).
 * All pointers 16-byte aligned (stats: 8).  VSA_ERR_ARG (before any HIP call): a NULL pointer, misalignment, step < 1,
 * lr, eps or inv_grad_scale negative or not finite, a beta outside [0, 1), nr_shells, rgb_degrees or a resolution out
 * of range.  VSA_ERR_UNSUPPORTED: row_format != 0, alpha_degrees != rgb_degrees, a row buffer beyond
 * vsa_nt_shade_bwd's 32-bit offset limit (row_base[last] * 8 >= 2^32). */
long long vsa_texel_fit_state_bytes(const vsa_nt_plan* plan);
int vsa_texel_fit_init(const vsa_nt_plan* plan, const int32_t* slot_of, const int32_t* seg_start, uint8_t* texels,
                       float* p, float* m, float* v, void* stream);
int vsa_texel_fit_step(const vsa_nt_plan* plan, const int32_t* slot_of, const int32_t* seg_start, uint16_t* grad_rows,
                       float inv_grad_scale, float* p, float* m, float* v, uint8_t* texels, float lr, float beta1,
                       float beta2, float eps, int step, unsigned long long* stats, void* stream);

/* ---- Texture mips (no counterpart in the reference; csrc/texture_mip.hip) ----
 * Minification filtering for baked scenes: a mip chain of the planes of "Texture export / import", built on the device,
 * and a baked shade that takes each SH degree's coefficients from the level its pixel's footprint on the surface asks
 * for.  The rule is this library's own, restated in tests/texture_mip_restated.py, which the three entry points equal
 * BIT FOR BIT; unpinned against the reference, which has no such stage.  fp32 with one rounding per operation in the
 * order written (the build compiles without contraction); sqrtf and / are IEEE, nothing of the log / exp / pow family
 * is called.
 *   chain       level 0 = the scene's planes at tex_res[d]; level l = 1..L the same layout at tex_res[d] >> l.  L is in
 *               1..VSA_TEXMIP_MAX_LEVELS and every tex_res[d] is divisible by 2^L.  Coefficients are filtered as BYTES,
 *               before the SH sum and the sigmoid ("Texture transfer" accepts the same): lut[q] is affine in q up to
 *               its fp16 roundings, so a mean of bytes is a mean of coefficients.
 *   reduce      pixel (r, c) of a level-l image has the four children (2r + a, 2c + b), a, b in 0..1, of the level
 *               below.  Per channel byte: q = (2 sum + n) / (2 n), an integer division (the mean, halves rounded up),
 *               over the n COVERED children; where no child is covered, over all four (n = 4).  Integers only: the
 *               same bytes on every call.  An alpha of 255 on every child (a shell without an alpha model) stays 255.
 *   coverage    an optional u8 mask per (shell, degree) at level 0, [R_d, R_d] in the planes' pixel orientation, ordered
 *               (shell, degree): mask (s, d) starts at byte s * C + sum_{d' < d} R_d'^2, C = sum_d R_d^2; nonzero =
 *               covered.  A level's mask is the OR of its children (stored as 0 / 1), with the same layout at that
 *               level's resolutions.  NULL = every texel covered.  Without it the zero bytes outside the charts (sh_lo,
 *               the most negative coefficient) bleed into the charts' edges at every level.
 *   density     per face slot of the tracer's triangle array: du1 = u1 - u0, dv1 = v1 - v0, du2 = u2 - u0, dv2 = v2 - v0
 *               of the slot's per-corner uvs; a2 = |du1 * dv2 - dv1 * du2|; c = e1 x e2 as vsa_nt_shade_fwd forms it
 *               (cx = e1.y e2.z - e1.z e2.y, ...); a3 = sqrtf((cx cx + cy cy) + cz cz); density = a2 / a3, and 0 where
 *               a3 is not > 0 or the quotient is not finite: uv area per world area.
 *   footprint   of a hit at distance t along its ray (hit_t; the rays of vsa_camera_rays and of the rasterizer are UNIT
 *               vectors, d / |d| in fp32, so t is a distance; the cosine below does not assume it):
 *               nn = (cx cx + cy cy) + cz cz, dd = (dx dx + dy dy) + dz dz, nd = |(cx dx + cy dy) + cz dz| with c the
 *               face's e1 x e2 and d the ray direction; cos = fmaxf(nd / sqrtf(nn * dd), 1/8) (a NaN quotient takes
 *               1/8); A_uv = (((t * t) * spread2) * density[slot]) / cos.  spread2 is the host's: the solid angle of a
 *               sample, 1 / (fx fy s^2) for a pinhole camera at supersample s, times 4^lod_bias.
 *   level       per degree d: A = A_uv * ((float)R_d * (float)R_d), the footprint in texels of level 0.  !(A >= 1)
 *               (magnification, NaN): l = 0, f = 0.  Else l0 = ((A's exponent field) - 127) >> 1 = floor(log4 A); where
 *               l0 >= L: l = L, f = 0 (the top level alone; +inf too); else l = l0 and f = (A * 4^-l0 - 1) * 0.333333343f
 *               (4^-l0 an exact power of two: f is linear in area between two levels, in [0, 1)).
 *   fetch       level 0 is the scene's own bank through slot_of / seg_start / row_base, exactly as vsa_nt_shade_fwd
 *               reads it (a bank out of bake() holds the network's values in the apron).  A level l >= 1 reads its
 *               planes by the corner rule of "Texture transfer, source lookup": nt_footprint(uv, R_d >> l, anchor)
 *               gives (i0, j0, fx, fy); corner k = 2 ky + kx reads texel (clamp(j0 + ky, 0, R-1), clamp(i0 + kx, 0, R-1))
 *               with weight (kx ? fx : 1 - fx) * (ky ? fy : 1 - fy) (anchor: all four are texel (j0, i0)); per channel
 *               acc = 0; acc = acc + lut[byte_k] * w_k for k = 0..3; the level's coefficient is fp16(acc).
 *   blend       f = 0: the coefficient is level l's.  f > 0 (then l < L; level l + 1 is fetched only here):
 *               c = fp16(c_l + f * (c_{l+1} - c_l)), a subtract, a multiply and an add in fp32 on the two fp16 values.
 *               Everything after the coefficients (SH evaluation, sigmoid, alpha decay, the dense scatter) is
 *               vsa_nt_shade_fwd's code (csrc/nt_shade_common.h).  Where every hit of a call has l = 0 and f = 0 in
 *               every degree, every output byte equals vsa_nt_shade_fwd's.
 * vsa_texmip_planes_bytes: the bytes of level `level`'s plane buffer, 0..L: vsa_nt_planes_bytes >> (2 level).
 * vsa_texmip_reduce: level `level` (1..8) from level `level - 1`, every image in one launch.  src_cover / dst_cover:
 *   the masks of the two levels; src_cover NULL = all covered (dst_cover, if given, is then all 1); dst_cover NULL =
 *   not wanted.  A lane makes two adjacent texels from two 16-byte loads and stores 8 bytes (one texel from four
 *   4-byte loads where the destination's rows are odd).  No LDS, no atomics.
 * vsa_texmip_density: density [nr_slots] f32 from tris [nr_slots, 12] (the tracer's records) and face_uvs [nr_slots, 6].
 * vsa_nt_shade_mip_fwd: vsa_nt_shade_fwd's arguments (forward only: no act_out; coeffs_out as there, the blended fp16
 *   coefficients) plus hit_t [K, N], slot_density, spread2, levels = L, level_planes [host]: L device pointers,
 *   level_planes[l - 1] = the planes of level l, and the optional lod_out [K, N, rgb_degrees] f32 = l + f per degree
 *   (NaN on a miss).
 * All device pointers 16-byte aligned.  VSA_ERR_ARG (before any HIP call): a NULL pointer, misalignment, level / levels
 *   outside 1..8, a tex_res[d] not divisible by 2^level (2^levels), wrong planes_bytes, src_planes == dst_planes,
 *   nr_slots < 1, nr_rays < 0, a spread2 that is negative or not finite, nr_shells, rgb_degrees or a resolution out of
 *   range.  VSA_ERR_UNSUPPORTED: alpha_degrees != rgb_degrees, row_format != 0. */
#define VSA_TEXMIP_MAX_LEVELS 8
long long vsa_texmip_planes_bytes(const vsa_nt_plan* plan, int level);
int vsa_texmip_reduce(const vsa_nt_plan* plan, int level, const uint8_t* src_planes, long long src_planes_bytes,
                      const uint8_t* src_cover, uint8_t* dst_planes, long long dst_planes_bytes, uint8_t* dst_cover,
                      void* stream);
int vsa_texmip_density(const float* tris, const float* face_uvs, long long nr_slots, float* density, void* stream);
int vsa_nt_shade_mip_fwd(const vsa_nt_plan* plan, const int32_t* hit_slot, const float* tex_uv, const float* rays_d,
                         const float* tris, const int32_t* slot_of, const int32_t* seg_start, const uint8_t* texels,
                         int nr_rays, const float* hit_t, const float* slot_density, float spread2, int levels,
                         const uint8_t* const* level_planes, float* surfs_rgb, float* surfs_alpha,
                         float* surfs_normals, float* coeffs_out, float* lod_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VOLSURFS_HIP_H */
