"""Neural-texture bank: parameters, plan and per-frame buffers of the K shells'
SH neural textures, and the host side of the shade stage.

Parameter shapes mirror what the reference instantiates per shell
(/root/reference/volsurfs_py/methods/volsurfs.py:143-206): an rgb
SHNeuralTextures (3 channels) and an alpha one (1 channel), each a ModuleList of
sh_degree+1 NeuralTexture = tcnn HashGrid (16 levels x 2 features, 2^15 entries,
base 16, x1.5; models/neural_texture.py:54-63) + FullyFusedMLP 32->64->64->C
(:65-77).  Here all of them live in two stacked tensors so that one launch
serves every texture:  tables [n_tex, E, 2],  weights [n_tex, 8192]
(W1[64,32] | W2[64,64] | W3[32,64], rows >= C zero), texture index
x = (shell*2 + type)*4 + degree.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib

MAX_SHELLS, MAX_DEG, MAX_LEVELS = 16, 4, 16
DOM_BLOCK = 4096
WEIGHTS_PER_TEX = 8192
# encode + MLP as one launch (csrc/nt_fused.hip; bit-identical to the two kernels).  Measured on
# MI355X (profiles/r03): forward-only evaluation, where the 730 MB of feature planes are neither
# written nor read, 1.30 -> 1.18 ms per 800x800 frame (+10.5 % Mrays/s); the training step, whose
# backward needs the planes, 0.65 vs 0.61-0.64 ms and 1 043 vs 1 061 it/s — the vector cache's
# look-up rate bounds the gathers (profiles/NOTEBOOK.md A9.1a).  Hence "auto": fused exactly when the feature
# planes are not needed.  VSA_NT_FUSED=1 / 0 force it on / off (A/B switch, tools/README).
# work split of the persistent kernels corrected by the previous frame's measured workgroup times
# (vsa_nt_rebalance; same results); "0" = the fitted cost model alone
REBALANCE = os.environ.get("VSA_NT_REBALANCE", "1") != "0"
FUSED_FORWARD = {"0": False, "1": True}.get(os.environ.get("VSA_NT_FUSED", "auto"), "auto")

# Scale of the f16 gradient chain relative to the ray count of a mean-L1 loss (the analogue of tiny-cuda-nn's
# loss scale; divided out before anything is accumulated in fp32).  With 1 x N the chain carried 1/3 per
# ray and channel: fine up to K = 7, but at K = 9 the shells behind eight others underflowed f16 — every
# MLP-weight gradient within 3.6e-3 of its tensor's largest entry instead of 3.1e-4 at 16 x N, table entries over
# 1e-3: 2.7e-5 -> 1.3e-6 of them (profiles/r05/parity_report.json; 16 and 256 measure the same, so 16 it is:
# the headroom to f16's 65 504 stays > 10x even with hundreds of hits on one texel).  A power of two: exact.
GRAD_CHAIN_GAIN = 16.0


def chain_scale(nr_rays=None, loss_scale=None):
    """The default scale of the f16 gradient chain of a mean-L1 step, from whichever the caller has: the number of rays
    the mean runs over (GAIN x nr_rays), or the factor its composite + L1 launch applies per ray and channel
    (GAIN / (3 x loss_scale)).  The same number when loss_scale = 1 / (3 nr_rays); a loss weight in it is divided out."""
    return GRAD_CHAIN_GAIN * float(nr_rays) if loss_scale is None else GRAD_CHAIN_GAIN / (3.0 * loss_scale)


def _stage(run, name, fn, *args, **kw):
    """fn(*args, **kw), through the stage hook `run(stage_name, thunk)` when the caller has one; no closure otherwise."""
    return fn(*args, **kw) if run is None else run(name, lambda: fn(*args, **kw))

class Plan(ctypes.Structure):
    """Mirror of `vsa_nt_plan` (include/volsurfs_hip.h)."""
    _fields_ = [
        ("nr_shells", ctypes.c_int32), ("rgb_degrees", ctypes.c_int32),
        ("alpha_degrees", ctypes.c_int32), ("inner_solid", ctypes.c_int32),
        ("with_alpha_decay", ctypes.c_int32), ("n_levels", ctypes.c_int32),
        ("tex_res", ctypes.c_int32 * MAX_DEG), ("sh_lo", ctypes.c_float * MAX_DEG),
        ("sh_span", ctypes.c_float * MAX_DEG), ("level_scale", ctypes.c_float * MAX_LEVELS),
        ("level_res", ctypes.c_int32 * MAX_LEVELS), ("level_size", ctypes.c_int32 * MAX_LEVELS),
        ("level_offset", ctypes.c_int32 * (MAX_LEVELS + 1)),
        ("dom_off", ctypes.c_int64 * (MAX_SHELLS * MAX_DEG + 1)),
        ("slot_capacity", ctypes.c_int64),
        ("max_rays", ctypes.c_int32), ("anchor", ctypes.c_int32),
        ("row_base", ctypes.c_int64 * (MAX_SHELLS * MAX_DEG + 1)),
        ("balance", ctypes.c_void_p),
        ("row_format", ctypes.c_int32), ("grads_zeroed", ctypes.c_int32),
        ("shared_rgb", ctypes.c_int32), ("shared_alpha", ctypes.c_int32),
    ]


ROW_QUADS = (2, 4, 8, 8)      # VSA_NT_ROW_QUADS(d): quads (4 elements) per texel / gradient row
ALPHA_QUAD = (1, 3, 4, 6)     # VSA_NT_ALPHA_QUAD(d): first alpha quad of a row


def grid_geometry(n_levels=16, log2_hashmap_size=15, base_resolution=16, per_level_scale=1.5):
    """Level geometry of tiny-cuda-nn's multiresolution grid (published formula;
    neural_texture.py:54-61 fixes the arguments)."""
    log2_pls = np.float32(math.log2(per_level_scale))
    scale, res, size, offset = [], [], [], [0]
    for l in range(n_levels):
        s = np.float32(np.exp2(np.float32(l) * log2_pls)) * np.float32(base_resolution) - np.float32(1.0)
        r = int(np.ceil(s)) + 1
        n = min((r * r + 7) // 8 * 8, 1 << log2_hashmap_size)
        scale.append(float(s))
        res.append(r)
        size.append(n)
        offset.append(offset[-1] + n)
    return scale, res, size, offset


class NeuralTextureBank(torch.nn.Module):
    def __init__(self, nr_shells, max_rays, sh_degree=3, alpha_sh_degree=3,
                 sh_range=(15.0, 15.0, 15.0, 15.0), textures_res=(2048, 1024, 512, 256),
                 inner_solid=False, with_alpha_decay=True, device="cuda", seed=42,
                 training=True, anchor=False, lerp=True, quantize_output=True, squeeze_output=True,
                 grid=None, shared_rgb=False, shared_alpha=False, parameters=True):
        """anchor / lerp / quantize_output / squeeze_output: NeuralTexture's switches
        (models/neural_texture.py:19-52; config keys using_neural_textures_anchor / _lerp,
        using_sh_quantization, using_sh_squeezing).  Built: lerp (the shipped configs) and anchor, each with 8-bit
        quantised texel rows (row_format 0), f16 rows of the un-quantised sigmoid (quantize_output=False: 1) or
        f16 rows of the raw network output (squeeze_output=False: 2; neural_texture.py:157-169, 181-187 skipped).
        shared_rgb / shared_alpha: are_volsurfs_colors_indep = 0 / are_volsurfs_alphas_indep = 0
        (methods/volsurfs.py:159-165, 200-206, 524-527, 553-556): ONE model for all shells — every shell reads
        the parameters of shell 0's textures of that type and the K shells' gradients accumulate there (the
        other shells' rows of `tables` / `weights` are unused and stay zero).  With inner_solid, shared_alpha
        means NO alpha model at all: the reference's loop stores models["alpha"] = None at i = 0 and leaves.
        grid: keyword arguments of grid_geometry() for a hash grid other than the reference's
        (16 levels always: the MLP reads 32 features); levels of more than 2^15 entries are refused
        by the library (one level = one LDS plane).
        parameters=False: a bank that only holds texel rows written from outside (texture_export.load_scene):
        no hash tables, MLP weights, feature planes or gradient rows; `tables` / `weights` are None."""
        super().__init__()
        if bool(anchor) == bool(lerp):
            raise ValueError("NeuralTexture is either anchor or lerp (neural_texture.py:47-51, 141-147)")
        if quantize_output and not squeeze_output:
            raise ValueError("quantize_output requires squeeze_output (sh_neural_textures.py:32-36)")
        # 0: 8-bit quantised rows (every shipped config); 1: f16 rows of sigmoid(x), un-quantised; 2: f16 rows of x
        self.row_format = 0 if quantize_output else (1 if squeeze_output else 2)
        self.shared_rgb, self.shared_alpha = bool(shared_rgb), bool(shared_alpha)
        self.anchor = bool(anchor)
        K = nr_shells
        self.K, self.max_rays = K, max_rays
        self.rgb_degrees, self.alpha_degrees = sh_degree + 1, alpha_sh_degree + 1
        self.D = max(self.rgb_degrees, self.alpha_degrees)
        scale, res, size, offset = grid_geometry(**(grid or {}))
        self.n_entries = offset[-1]
        self.n_tex = K * 2 * MAX_DEG
        p = Plan()
        p.nr_shells, p.rgb_degrees, p.alpha_degrees = K, self.rgb_degrees, self.alpha_degrees
        p.inner_solid, p.with_alpha_decay, p.n_levels = int(inner_solid), int(with_alpha_decay), 16
        for d in range(MAX_DEG):
            p.tex_res[d] = int(textures_res[d])
            p.sh_lo[d] = -float(sh_range[d])
            p.sh_span[d] = 2.0 * float(sh_range[d])
        for l in range(16):
            p.level_scale[l], p.level_res[l], p.level_size[l] = scale[l], res[l], size[l]
        for l in range(17):
            p.level_offset[l] = offset[l]
        off, cap, quads = 0, 0, 0
        for s in range(K):
            for d in range(MAX_DEG):
                p.dom_off[s * MAX_DEG + d] = off
                p.row_base[s * MAX_DEG + d] = quads
                if d < self.D:
                    T = (textures_res[d] + 2) ** 2
                    off += (T + DOM_BLOCK - 1) // DOM_BLOCK * DOM_BLOCK
                    cap += min(4 * max_rays, T)
                    quads += (min(4 * max_rays, T) * ROW_QUADS[d] + 7) // 8 * 8
        for i in range(K * MAX_DEG, MAX_SHELLS * MAX_DEG + 1):
            p.dom_off[i] = off
            p.row_base[i] = quads
        self.row_quads_total = quads
        cap = (cap + 255) // 256 * 256 + 256      # feature planes are blocked by 256 slots
        p.slot_capacity = cap
        p.max_rays = max_rays
        p.anchor = int(self.anchor)
        p.row_format = int(self.row_format)
        p.shared_rgb, p.shared_alpha = int(self.shared_rgb), int(self.shared_alpha)
        self.plan, self.dom_total, self.slot_capacity = p, off, cap
        self.tex_res = tuple(int(r) for r in textures_res)

        self.has_parameters = bool(parameters)
        if not parameters:
            self.tables = self.weights = None
            self._alloc(device, training=False)
            return
        # ---- parameters (fp32 masters), tcnn-style init: U(-1e-4, 1e-4) tables,
        # Xavier-uniform weights
        g = torch.Generator().manual_seed(seed)
        tables = (torch.rand(self.n_tex, self.n_entries, 2, generator=g) * 2 - 1) * 1e-4
        weights = torch.zeros(self.n_tex, WEIGHTS_PER_TEX)
        for x in range(self.n_tex):
            C = self.tex_channels(x)
            if C and self.param_tex(x) != x:     # (a shell that reads shell 0's shared model owns no parameters)
                tables[x] = 0
                continue
            if C == 0:
                continue

            def xav(o, i):
                s_ = math.sqrt(6.0 / (i + o))
                return (torch.rand(o, i, generator=g) * 2 - 1) * s_
            w3 = torch.zeros(32, 64)
            pad = (C + 15) // 16 * 16
            w3[:C] = xav(pad, 64)[:C]
            weights[x] = torch.cat([xav(64, 32).flatten(), xav(64, 64).flatten(), w3.flatten()])
        self.tables = torch.nn.Parameter(tables.to(device))
        self.weights = torch.nn.Parameter(weights.to(device))
        self._alloc(device, training)

    # -- bookkeeping -------------------------------------------------------
    def tex_channels(self, x):
        deg, typ, shell = x % MAX_DEG, (x // MAX_DEG) & 1, x // (2 * MAX_DEG)
        if typ == 0:
            return 3 * (2 * deg + 1) if deg < self.rgb_degrees else 0
        if self.plan.inner_solid and (shell == 0 or self.shared_alpha):     # nt_shell_has_alpha (csrc/nt_common.h)
            return 0
        return (2 * deg + 1) if deg < self.alpha_degrees else 0

    def param_tex(self, x):
        """The texture whose rows of `tables` / `weights` (and of their gradients) logical texture x uses:
        itself, or shell 0's of the same type and degree when that type's model is shared (nt_param_tex)."""
        typ = (x // MAX_DEG) & 1
        return x % (2 * MAX_DEG) if (self.shared_alpha if typ else self.shared_rgb) else x

    @staticmethod
    def tex_index(shell, typ, deg):
        return (shell * 2 + typ) * MAX_DEG + deg

    def _alloc(self, dev, training):
        i32, u8 = torch.int32, torch.uint8
        cap, K = self.slot_capacity, self.K
        self.frame_generation = 0        # (all per-frame and gradient state is declared here) bumped by frame()
        self.texels_version = 0          # bumped by whatever rewrites a BAKED bank's bytes (bake_all, the plane import,
                                         # a texel-fit step): a texture_mip.MipChain built before is stale afterwards
        self.baked, self._marks_dirty = False, False     # the rows hold EVERY texel (bake_all); a mark not yet compacted
        self._grad_flat = None           # zero_grads(): tables.grad | weights.grad | _dfsum as one allocation, built lazily
        self._dfsum, self._dfsum_clean = None, False     # per-texture sum |dF| of the MLP backward; "is all zero"
        self._tables_grad_sig = None     # zero_grads() -> _take_grads_zeroed(): (id, version) of the all-zero tables.grad
        if REBALANCE:
            self.balance = torch.zeros(_lib.workspace_bytes("vsa_nt_balance_bytes"), dtype=u8, device=dev)
            self.plan.balance = self.balance.data_ptr()
        self.marks = torch.zeros(self.dom_total, dtype=u8, device=dev)
        self.slot_of = torch.full((self.dom_total,), -1, dtype=i32, device=dev)
        self.texel_of_slot = torch.zeros(cap, dtype=i32, device=dev)
        self.slot_xy = torch.zeros(cap, 2, device=dev)
        self.seg_start = torch.zeros(K * MAX_DEG + 1, dtype=i32, device=dev)
        self.block_scratch = torch.zeros(self.dom_total // DOM_BLOCK + 1, dtype=i32, device=dev)
        texel_dtype = u8 if self.row_format == 0 else torch.float16
        if not self.has_parameters:
            self.features = self.tables_h = self.weights_h = self.grad_rows = None
            self.texels = torch.zeros(self.row_quads_total * 4, dtype=texel_dtype, device=dev)
            return
        # blocked layout [type][slot/256][level][slot%256][2]  (nt_common.h: nt_feat_index)
        self.features = torch.empty(2, cap // 256, 16, 256, 2, dtype=torch.float16, device=dev)
        self.tables_h = torch.empty(self.n_tex, self.n_entries, 2, dtype=torch.float16, device=dev)
        self.weights_h = torch.empty(self.n_tex, WEIGHTS_PER_TEX, dtype=torch.float16, device=dev)
        # per-degree row widths (include/volsurfs_hip.h: VSA_NT_ROW_QUADS), 4 elements per quad
        # texel rows: 4 elements per quad — bytes (8-bit quantised) or halves (row_format 1)
        self.texels = torch.zeros(self.row_quads_total * 4, dtype=texel_dtype, device=dev)
        self.grad_rows = torch.zeros(self.row_quads_total * 4, dtype=torch.float16, device=dev) if training else None
        self._dfsum, self._dfsum_clean = torch.zeros(self.n_tex, 32, device=dev), True
        self.refresh_half_params()

    @torch.no_grad()
    def refresh_half_params(self):
        """fp16 compute copies of the fp32 masters (tcnn keeps the same pair)."""
        self.wait_params()
        self.tables_h.copy_(self.tables)
        self.weights_h.copy_(self.weights)

    # -- stages --------------------------------------------------------------
    def frame(self, hit_slot, hit_uv, face_uvs):
        """The step for these hits as a ShadedFrame: the texels they touch get their slots (a baked bank has them and
        only resolves the hits' uv).  An earlier frame's per-frame state is gone from here on: its backward refuses."""
        tex_uv = (self.tex_uv_only if self.baked else self.mark_and_compact)(hit_slot, hit_uv, face_uvs)
        self.frame_generation += 1
        return ShadedFrame(self, hit_slot, tex_uv)

    def mark_and_compact(self, hit_slot, hit_uv, face_uvs, want_texel_of_slot=False):
        """hit_slot [K,N] i32, hit_uv [K,N,2], face_uvs [nr_tris,6] (leaf order).
        Returns tex_uv [K,N,2].  slot_of is valid for the touched texels only (vsa_nt_compact_frame);
        texel_of_slot (the inverse map: nothing on the path reads it) is written on request."""
        K, N = hit_slot.shape
        assert K == self.K and N <= self.max_rays
        if self.baked:
            raise _lib.VolsurfsHipError("this bank holds baked textures: use tex_uv_only + shade")
        # Invariant: the marks are zero between frames — allocated so, and vsa_nt_compact_frame clears
        # what it reads.  `_marks_dirty` is set while a mark has not been followed by a compaction that
        # returned OK (an exception between the two, a failed launch): stale marks would silently
        # inflate every later frame's slot counts.
        if self._marks_dirty:
            self.marks.zero_()
        self._marks_dirty = True
        tex_uv = self.tex_uv_only(hit_slot, hit_uv, face_uvs, self.marks)
        _lib.call("vsa_nt_compact_frame", ctypes.byref(self.plan), self.marks, self.slot_of,
                  self.texel_of_slot if want_texel_of_slot else None, self.slot_xy, self.seg_start,
                  self.block_scratch, _lib.stream_ptr())
        self._marks_dirty = False
        return tex_uv

    # -- baking (the deploy format, sh_neural_textures.py:99-114 /
    # neural_texture.py:200-251 evaluate every texel once and store it as an 8-bit texture)
    @staticmethod
    def full_capacity_rays(textures_res):
        """max_rays for which every (shell, degree) segment can hold ALL its texels."""
        return ((max(int(r) for r in textures_res) + 2) ** 2 + 3) // 4

    @torch.no_grad()
    def bake_all(self):
        """Evaluate EVERY texel of every texture (instead of the texels a frame touches): after
        this, `shade` works for any ray without mark/compact/encode/mlp.  Needs a bank built
        with max_rays >= full_capacity_rays(textures_res)."""
        if self.row_format != 0:
            raise _lib.VolsurfsHipError("baked textures are the 8-bit deploy format: using_sh_quantization=1 only")
        self.compact_all()
        self.evaluate(need_features=False)
        self.baked = True
        self.texels_version += 1
        return self

    @torch.no_grad()
    def compact_all(self, want_texel_of_slot=True):
        """Give EVERY texel of every (shell, degree) domain, interior and one-texel apron, a slot: all marks set,
        then vsa_nt_compact_frame (the slot layout of a baked bank)."""
        self.marks.zero_()
        for s in range(self.K):
            for d in range(self.D):
                R = self.tex_res[d]
                W = R + 2
                if min(4 * self.max_rays, W * W) < W * W:
                    raise _lib.VolsurfsHipError("bake_all needs a full-capacity bank "
                                                "(max_rays >= NeuralTextureBank.full_capacity_rays)")
                off = int(self.plan.dom_off[s * MAX_DEG + d])
                self.marks[off:off + W * W].view(W, W).fill_(1)   # interior + the one-texel apron
        _lib.call("vsa_nt_compact_frame", ctypes.byref(self.plan), self.marks, self.slot_of,
                  self.texel_of_slot if want_texel_of_slot else None, self.slot_xy, self.seg_start,
                  self.block_scratch, _lib.stream_ptr())

    @torch.no_grad()
    def baked_textures(self):
        """{(shell, type, degree): uint8 [R, R, C]} indexed [iy, ix] in the network's texel
        coordinates (texel centre = ((ix + 0.5) / R, (iy + 0.5) / R), see nt_footprint: the
        reference's 90-degree-rotated uv, neural_texture.py:114-121); C = channels x (2d+1)."""
        dense = self.rows_dense(self.texels)
        out = {}
        for s in range(self.K):
            for d in range(self.D):
                R = self.tex_res[d]
                W, n = R + 2, 2 * d + 1
                off = int(self.plan.dom_off[s * MAX_DEG + d])
                slots = self.slot_of[off:off + W * W].view(W, W)[1:R + 1, 1:R + 1].long()
                rows = dense[slots]                                  # [R, R, 32]
                if self.tex_channels(self.tex_index(s, 0, d)):
                    out[(s, 0, d)] = rows[..., :3 * n].contiguous()
                if self.tex_channels(self.tex_index(s, 1, d)):
                    out[(s, 1, d)] = rows[..., 24:24 + n].contiguous()
        return out

    def tex_uv_only(self, hit_slot, hit_uv, face_uvs, marks=None):
        """Per-hit texture uv without touching the compaction (inference from a baked bank); marks: mark_and_compact's."""
        K, N = hit_slot.shape
        tex_uv = torch.empty(K, N, 2, device=hit_slot.device)
        _lib.call("vsa_nt_mark", ctypes.byref(self.plan), hit_slot, hit_uv, face_uvs, N, tex_uv, marks, _lib.stream_ptr())
        return tex_uv

    def wait_params(self):
        """An optimiser step may still be running on a side stream (VolSurfs.optim_step(overlap=True)):
        the first reader of the parameters on the current stream waits for it here."""
        ev = getattr(self, "_params_event", None)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)
            self._params_event = None

    @staticmethod
    def encode_config(sibling_groups, grid_override=0):
        """Process-wide setting of the hash-grid encode launches (vsa_nt_encode_config): the hashed levels walked by the
        plain walk (0) or in sibling groups (1: forward and backward, 2: backward only — the default, 3: forward only),
        and a forced number of workgroups (0: one per compute unit)."""
        _lib.call("vsa_nt_encode_config", int(sibling_groups), int(grid_override))

    @staticmethod
    def encode_row_terms(forward, backward):
        """Process-wide switch of the encode kernels' row terms (vsa_nt_encode_row_terms), 0 / 1 per direction: what
        the cell arithmetic derives from a texel row's y once per lane run instead of once per slot.  Same bits.
        Only the backward has such a walk (default on); `forward` is accepted and ignored."""
        _lib.call("vsa_nt_encode_row_terms", int(forward), int(backward))

    def encode(self):
        self.wait_params()
        _lib.call("vsa_nt_encode_fwd", ctypes.byref(self.plan), self.tables_h, self.slot_xy,
                  self.seg_start, self.features, _lib.stream_ptr())
        return self.features

    def features_level_major(self):
        """[type, level, slot, 2] view-copy of the blocked feature planes (tests)."""
        f = self.features.permute(0, 2, 1, 3, 4)            # [type, level, block, 256, 2]
        return f.reshape(2, 16, self.slot_capacity, 2)

    def mlp(self, want_pre=False):
        self.wait_params()
        pre = torch.zeros(self.slot_capacity, 32, dtype=torch.float16, device=self.texels.device) if want_pre else None
        _lib.call("vsa_nt_mlp_fwd", ctypes.byref(self.plan), self.weights_h, self.features,
                  self.seg_start, self.texels, pre, _lib.stream_ptr())
        return (self.rows_dense(self.texels), pre) if want_pre else self.texels

    def encode_mlp(self, write_features=True, want_pre=False):
        """encode() + mlp() as ONE launch (csrc/nt_fused.hip; bit-identical results).
        write_features=False: inference — the feature planes are neither written nor read."""
        self.wait_params()
        pre = torch.zeros(self.slot_capacity, 32, dtype=torch.float16, device=self.texels.device) if want_pre else None
        _lib.call("vsa_nt_encode_mlp_fwd", ctypes.byref(self.plan), self.tables_h, self.weights_h,
                  self.slot_xy, self.seg_start, self.features if write_features else None,
                  self.texels, pre, _lib.stream_ptr())
        return (self.rows_dense(self.texels), pre) if want_pre else self.texels

    def evaluate(self, need_features=True, run=None):
        """Texel rows of the compacted slots.  need_features=False (inference, baking): the fused
        launch; True (a backward pass follows): the level-major encode kernel, then the MLP kernel.
        run: the stage hook of ShadedFrame."""
        if self.row_format == 0 and (FUSED_FORWARD is True or (FUSED_FORWARD == "auto" and not need_features)):
            return _stage(run, "nt_encode_mlp_fwd", self.encode_mlp, write_features=need_features)
        _stage(run, "nt_encode_fwd", self.encode)
        return _stage(run, "nt_mlp_fwd", self.mlp)

    def rows_dense(self, buf):
        """Tests / export: the per-degree rows of `texels` or `grad_rows` re-laid as
        [slot_capacity, 32] with rgb coefficient c at column c and alpha coefficient c at 24+c."""
        seg = self.seg_start.cpu().tolist()
        dense = torch.zeros(self.slot_capacity, 32, dtype=buf.dtype, device=buf.device)
        for s in range(self.K):
            for d in range(self.D):
                sd, n, q = s * MAX_DEG + d, 2 * d + 1, ROW_QUADS[d]
                a, b = seg[sd], seg[sd + 1]
                r0 = int(self.plan.row_base[sd]) * 4
                rows = buf[r0:r0 + (b - a) * q * 4].view(b - a, q * 4)
                dense[a:b, :3 * n] = rows[:, :3 * n]
                dense[a:b, 24:24 + n] = rows[:, 4 * ALPHA_QUAD[d]:4 * ALPHA_QUAD[d] + n]
        return dense

    def shade(self, hit_slot, tex_uv, rays_d, tris, want_coeffs=False, want_normals=False,
              act_out=None):
        """act_out: optional [K,N,4] f32 buffer that receives the per-hit output sigmoids;
        pass it to backward_shade(act=...) of the same frame to skip the re-gather."""
        K, N = hit_slot.shape
        dev = hit_slot.device
        rgb = torch.empty(N, K, 3, device=dev)
        alpha = torch.empty(N, K, device=dev)
        normals = torch.empty(N, K, 3, device=dev) if want_normals else None
        coeffs = torch.empty(K, N, 64, device=dev) if want_coeffs else None
        _lib.call("vsa_nt_shade_fwd", ctypes.byref(self.plan), hit_slot, tex_uv, rays_d, tris,
                  self.slot_of, self.seg_start, self.texels, N, rgb, alpha, normals, coeffs,
                  act_out, _lib.stream_ptr())
        return rgb, alpha, normals, coeffs

    def backward(self, hit_slot, tex_uv, rays_d, tris, g_surfs_rgb, g_surfs_alpha, grad_scale,
                 act=None, grads_zeroed=None):
        """Back-propagates d loss / d surfs_rgb [N,K,3], d surfs_alpha [N,K] to
        self.tables.grad / self.weights.grad (accumulating, like autograd).
        grad_scale keeps the fp16 intermediate gradients in range (the analogue of
        tiny-cuda-nn's loss scale); it is divided out before accumulation.
        grads_zeroed: see backward_encode."""
        self.backward_shade(hit_slot, tex_uv, rays_d, tris, g_surfs_rgb, g_surfs_alpha, grad_scale, act)
        self.backward_mlp(grad_scale)
        self.backward_encode(grad_scale, grads_zeroed=grads_zeroed)

    def _ensure_grads(self):
        if self.tables.grad is None:
            self.tables.grad = torch.zeros_like(self.tables)
        if self.weights.grad is None:
            self.weights.grad = torch.zeros_like(self.weights)

    def zero_grads(self):
        """tables.grad, weights.grad and the per-texture sum |dF| of the MLP backward live in ONE
        allocation so that a training step clears them with one fill (three small launches
        otherwise).  Returns False if the gradient tensors are not (any more) those views —
        e.g. an optimiser's zero_grad(set_to_none=True) dropped them — and clears what exists."""
        flat = self._grad_flat
        nt, nw = self.tables.numel(), self.weights.numel()
        if flat is None:
            flat = torch.zeros(nt + nw + self.n_tex * 32, device=self.tables.device)
            self._grad_flat = flat
            self._flat_t, self._flat_w = flat[:nt].view_as(self.tables), flat[nt:nt + nw].view_as(self.weights)
            self._dfsum = flat[nt + nw:].view(self.n_tex, 32)
        if self.tables.grad is None and self.weights.grad is None:
            self.tables.grad, self.weights.grad = self._flat_t, self._flat_w
        whole = self.tables.grad is self._flat_t and self.weights.grad is self._flat_w
        if whole:
            flat.zero_()
            self._dfsum_clean = True
        else:
            self.tables.grad.zero_()
            self.weights.grad.zero_()
        # (backward_encode: a sole writer's table plane is stored, not added, while tables.grad is this all-zero buffer)
        self._tables_grad_sig = (id(self.tables.grad), self.tables.grad._version)
        return whole

    def _take_grads_zeroed(self, grads_zeroed):
        """plan.grads_zeroed of the next hash-grid backward launch: the caller's word (it knows its optimiser
        has just cleared the gradients), else what zero_grads() left; either way the buffer holds something
        after the launch."""
        if grads_zeroed is None:       # zero_grads() said so: still the same buffer, untouched by torch since?
            g = self.tables.grad
            grads_zeroed = g is not None and self._tables_grad_sig == (id(g), g._version)
        # (shared models: the kernel itself keeps a shared plane's flushes atomic — K shells write it)
        self._tables_grad_sig = None
        self.plan.grads_zeroed = int(bool(grads_zeroed))

    def backward_shade(self, hit_slot, tex_uv, rays_d, tris, g_surfs_rgb, g_surfs_alpha, grad_scale,
                       act=None, grad_rows=None):
        """grad_rows: the caller's f16 rows instead of the bank's own (the texel fit, on a bank without parameters)."""
        if grad_rows is None:
            self._ensure_grads()
            grad_rows = self.grad_rows
        if act is not None:
            _lib.check_f32(act, hit_slot.shape[0], hit_slot.shape[1], 4)
        _lib.call("vsa_nt_shade_bwd", ctypes.byref(self.plan), hit_slot, tex_uv, rays_d, tris, self.slot_of,
                  self.seg_start, self.texels, hit_slot.shape[1], g_surfs_rgb.contiguous(), g_surfs_alpha.contiguous(),
                  float(grad_scale), grad_rows, act, _lib.stream_ptr())

    def backward_mlp(self, grad_scale):
        if not self._dfsum_clean:
            self._dfsum.zero_()
        self._dfsum_clean = False            # (zero_grads() has just cleared it together with the gradients)
        _lib.call("vsa_nt_mlp_bwd", ctypes.byref(self.plan), self.weights_h, self.features,
                  self.seg_start, self.grad_rows, self.weights.grad, self._dfsum,
                  1.0 / float(grad_scale), _lib.stream_ptr())

    def backward_encode(self, grad_scale, shells=None, grads_zeroed=None):
        """shells=(begin, end) restricts the launch to those shells' textures (their table
        gradients are the contiguous slice tables.grad[begin*8:end*8]).  grads_zeroed=True: the caller
        vouches that tables.grad is all zero (vsa_nt_plan.grads_zeroed); None: true right after zero_grads()."""
        self._take_grads_zeroed(grads_zeroed)
        if shells is None:
            _lib.call("vsa_nt_encode_bwd", ctypes.byref(self.plan), self.features, self._dfsum,
                      float(grad_scale), self.slot_xy, self.seg_start, self.tables.grad,
                      _lib.stream_ptr())
        else:
            _lib.call("vsa_nt_encode_bwd_range", ctypes.byref(self.plan), self.features,
                      self._dfsum, float(grad_scale), self.slot_xy, self.seg_start,
                      self.tables.grad, int(shells[0]), int(shells[1]), _lib.stream_ptr())

    def backward_encode_phased(self, grad_scale, signals, grads_zeroed=None):
        """The hash-grid backward as ONE launch that finishes the shells phase by phase and publishes
        each phase's completion in signals.flags (parallel.StepSignals; vsa_nt_encode_bwd_phased)."""
        self._take_grads_zeroed(grads_zeroed)
        _lib.call("vsa_nt_encode_bwd_phased", ctypes.byref(self.plan), self.features, self._dfsum,
                  float(grad_scale), self.slot_xy, self.seg_start, self.tables.grad, signals.n,
                  signals.phase_end_c, signals._flags, signals.counters, signals.epoch, int(signals.reserve_cus),
                  _lib.stream_ptr())


class ShadedFrame:
    """The neural-texture step of one batch of hits, written once: `bank.frame(hits)` (mark / compact) ->
    `forward` (encode + MLP -> shade) -> the caller's own composite and loss -> `backward` (shade backward -> MLP
    backward -> hash-grid backward).  Plain launches on the current stream, no autograd inside.  Holds what its backward
    reads beside the bank's per-frame buffers, and the bank's generation it was made at.
    run: an optional stage hook, run(stage_name, thunk) -> thunk(), once per launch (KShellPipeline's stage timer)."""
    __slots__ = ("bank", "generation", "hit_slot", "tex_uv", "rays_d", "tris", "act")

    def __init__(self, bank, hit_slot, tex_uv):
        self.bank, self.generation, self.hit_slot, self.tex_uv = bank, bank.frame_generation, hit_slot, tex_uv
        self.rays_d = self.tris = self.act = None

    def forward(self, rays_d, tris, differentiable, want_normals=False, run=None):
        """(surfs_rgb [N,K,3], surfs_alpha [N,K], normals | None).  differentiable: the feature planes and the hits'
        output sigmoids are kept for a backward."""
        bank, (K, N) = self.bank, self.hit_slot.shape
        if not bank.baked:
            bank.evaluate(need_features=differentiable, run=run)
        self.rays_d, self.tris = rays_d, tris
        self.act = torch.empty(K, N, 4, device=rays_d.device) if differentiable else None
        return _stage(run, "nt_shade_fwd", bank.shade, self.hit_slot, self.tex_uv, rays_d, tris,
                      want_normals=want_normals, act_out=self.act)[:3]

    def _check(self):
        if self.bank.frame_generation != self.generation:
            raise _lib.VolsurfsHipError("backward of a frame whose per-frame texel state was overwritten by a later frame "
                                        "(a render, a training step): call backward before rendering again")

    def backward_rows(self, g_rgb, g_alpha, scale, grad_rows=None, run=None):
        """Shade backward into the gradient rows, MLP backward into weights.grad and the feature gradients.
        grad_rows: the caller's rows instead, and the shade backward alone (the texel fit, on a baked bank)."""
        self._check()
        bank = self.bank
        _stage(run, "nt_shade_bwd", bank.backward_shade, self.hit_slot, self.tex_uv, self.rays_d, self.tris, g_rgb,
               g_alpha, scale, self.act, grad_rows=grad_rows)
        if grad_rows is None:
            _stage(run, "nt_mlp_bwd", bank.backward_mlp, scale)

    def backward_tables(self, scale, shells=None, signals=None, grads_zeroed=None, run=None):
        """The hash-grid backward: whole, for shells=(begin, end), or phased with signals (parallel.StepSignals)."""
        self._check()
        if signals is not None:
            _stage(run, "nt_encode_bwd", self.bank.backward_encode_phased, scale, signals, grads_zeroed=grads_zeroed)
        else:
            _stage(run, "nt_encode_bwd", self.bank.backward_encode, scale, shells=shells, grads_zeroed=grads_zeroed)

    def backward(self, g_rgb, g_alpha, scale, grads_zeroed=None, grad_rows=None, run=None):
        """backward_rows, then (unless grad_rows takes the gradient) backward_tables.  scale: chain_scale's."""
        self.backward_rows(g_rgb, g_alpha, scale, grad_rows=grad_rows, run=run)
        if grad_rows is None:
            self.backward_tables(scale, grads_zeroed=grads_zeroed, run=run)


def stage_accounting(bank, nr_rays, nr_hits, tracer_bytes=0):
    """ALGORITHMIC bytes / FLOPs of every neural-texture stage for the frame the bank last compacted
    (DESIGN.md §5): each operand counted once per stage at its stored width, gathers per hit.  Host-side
    read-back of the slot counts: outside any timed region.  Returns (bytes per stage, unpadded forward FLOPs
    of the MLP over the unique texels, slots)."""
    N, K, M = nr_rays, bank.K, nr_hits
    P = int(bank.seg_start[K * 4].item())
    seg = bank.seg_start.cpu().tolist()
    fl, row_quads, slot_models = 0, 0, 0
    for s_ in range(K):
        for d in range(4):
            P_sd = seg[s_ * 4 + d + 1] - seg[s_ * 4 + d]
            row_quads += P_sd * ROW_QUADS[d]
            for typ in range(2):
                C = bank.tex_channels(bank.tex_index(s_, typ, d))
                if C:
                    fl += P_sd * 2 * (32 * 64 + 64 * 64 + 64 * C)
                    slot_models += P_sd
    ntex = sum(1 for x in range(bank.n_tex) if bank.tex_channels(x))
    rows_u8, rows_f16 = row_quads * 4, row_quads * 8      # texel rows u8, gradient rows f16
    feats = slot_models * 64                      # 16 levels x f16x2 per (slot, model)
    gathers = M * (16 * 4 + 4 * sum(ROW_QUADS) * 4 + 8) + N * 12   # slot ids + 16 texel rows + uv, dirs
    acct = {
        "trace": N * (24 + 16 * K) + tracer_bytes,
        # marks read twice (count, assign); per slot: mark set + cleared, slot_of, slot_xy
        # (vsa_nt_compact_frame: nothing is written for untouched texels)
        "nt_mark_compact": N * K * 20 + bank.dom_total * (1 + 1) + P * (1 + 1 + 4 + 8),
        "nt_encode_fwd": P * 8 + feats + ntex * bank.n_entries * 4,
        "nt_mlp_fwd": feats + rows_u8 + ntex * 8192 * 2,
        # fused: texel centre in (per texture), feature planes + texel rows out, parameters once
        "nt_encode_mlp_fwd": slot_models * 8 + feats + rows_u8 + ntex * (bank.n_entries * 4 + 8192 * 2),
        "nt_shade_fwd": gathers + N * K * 16,
        "nt_shade_bwd": gathers + N * K * 16 + rows_f16,
        "nt_mlp_bwd": 2 * feats + 2 * rows_f16 + ntex * 8192 * (2 + 4),
        "nt_encode_bwd": feats + P * 8 + ntex * bank.n_entries * 8,
    }
    return acct, fl, P
