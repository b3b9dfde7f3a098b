"""RayTracer — raytracelib-shaped ray / K-shell intersector (SURVEY §8a A2, §8b
"Secondary boundaries").

Mirrors `raytracelib.RayTracer(list[TensorMesh])` / `.trace(rays_o, rays_d,
mesh_id=int) -> dict` as called at the reference's
volsurfs_py/methods/volsurfs.py:128 and :476-501, and adds
`trace_all` (all K shells in one launch, no host sync) used by the fused path.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib


def _rays(rays_o, rays_d):
    """(N, rays_o, rays_d): the rays as checked contiguous f32 [N, 3] tensors."""
    N = rays_o.shape[0]
    return N, _lib.check_f32(rays_o.contiguous(), N, 3), _lib.check_f32(rays_d.contiguous(), N, 3)


def _sizes(fn, h):
    """(status, (nr_nodes, nr_tris, depth)) of one tree handle, from vsa_bvh_sizes / vsa_bvh_dev_sizes."""
    nn, nt, md = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = fn(h, ctypes.byref(nn), ctypes.byref(nt), ctypes.byref(md))
    return rc, (nn.value, nt.value, md.value)


class _HostTrees:
    """The shells' binned-SAH trees, built on the CPU from host copies of the meshes (csrc/bvh_build.cpp)."""

    def __init__(self):
        self.handles = []

    def build(self, meshes, leaf_size, radius):
        """Builds every shell's tree; returns their (nr_nodes, nr_tris, depth) in mesh order."""
        L = _lib.lib()
        arrays = [(np.ascontiguousarray(m.vertices.detach().cpu().numpy(), np.float32),
                   np.ascontiguousarray(m.faces.detach().cpu().numpy(), np.int32)) for m in meshes]
        made = self.handles = []        # every tree as it is made: what destroy frees if the build fails part-way

        def build_one(vf):
            v, f = vf
            h = ctypes.c_void_p()
            rc = L.vsa_bvh_build(v.ctypes.data_as(ctypes.c_void_p), f.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.c_int(v.shape[0]), ctypes.c_int(f.shape[0]),
                                 ctypes.c_int(leaf_size), ctypes.byref(h))
            if h.value:
                made.append(h)
            return rc, h
        # The shells' trees are independent builds, one thread each: built side by side on a thread pool (ctypes drops
        # the GIL inside the call), 7 x 1.31 M triangles (configs[4]) take the time of one shell (2.1 s) instead of
        # 15 s.  Handles are collected in mesh order: the layout is the sequential build's.
        if len(arrays) > 1 and sum(f.shape[0] for _, f in arrays) >= 100000 and os.environ.get("VSA_BVH_THREADS", "1") != "0":
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(len(arrays), os.cpu_count() or 1)) as pool:
                built = list(pool.map(build_one, arrays))
        else:
            built = [build_one(vf) for vf in arrays]
        for rc, _ in built:
            if rc != 0:
                raise _lib.VolsurfsHipError(f"vsa_bvh_build failed with status {rc}")
        self.handles = [h for _, h in built]                        # (in mesh order)
        return [_sizes(L.vsa_bvh_sizes, h)[1] for h in self.handles]

    def export(self, layout, nodes, qnodes, tris, frames):
        """Both node formats and the triangles into the concatenated arrays (staged through numpy: they may live on
        the GPU), the K quantisation frames into the host array `frames`."""
        L = _lib.lib()
        h_nodes = np.empty(tuple(nodes.shape), np.float32)
        h_qnodes = np.empty(tuple(qnodes.shape), np.uint32)
        h_tris = np.empty(tuple(tris.shape), np.float32)
        for i, (h, (nb, nn, tb, nt)) in enumerate(zip(self.handles, layout)):
            rc = L.vsa_bvh_export(h, h_nodes[nb:nb + nn].ctypes.data_as(ctypes.c_void_p),
                                  h_tris[tb:tb + nt].ctypes.data_as(ctypes.c_void_p), ctypes.c_int(nb),
                                  ctypes.c_int(tb))
            rc2 = L.vsa_bvh_export_q(h, h_qnodes[nb:nb + nn].ctypes.data_as(ctypes.c_void_p),
                                     h_tris[tb:tb + nt].ctypes.data_as(ctypes.c_void_p), ctypes.c_int(nb),
                                     ctypes.c_int(tb), ctypes.c_void_p(ctypes.addressof(frames) + 24 * i))
            if rc != 0 or rc2 != 0:
                raise _lib.VolsurfsHipError(f"vsa_bvh_export failed with status {rc} / {rc2}")
        nodes.copy_(torch.from_numpy(h_nodes))
        qnodes.copy_(torch.from_numpy(h_qnodes.view(np.int32)))
        tris.copy_(torch.from_numpy(h_tris))

    def refit(self, meshes):
        L = _lib.lib()
        for h, m in zip(self.handles, meshes):
            v = np.ascontiguousarray(m.vertices.detach().cpu().numpy(), np.float32)
            rc = L.vsa_bvh_refit(h, v.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(v.shape[0]))
            if rc != 0:
                raise _lib.VolsurfsHipError(f"vsa_bvh_refit failed with status {rc} (vertex count changed?)")

    def destroy(self):
        for h in self.handles:
            _lib.lib().vsa_bvh_destroy(h)
        self.handles = []


class _DeviceTrees:
    """The shells' trees built on the GPU from the meshes' device tensors, no host copy: the Karras LBVH
    (builder="device", csrc/bvh_device.hip) or PLOC clustering (builder="ploc", csrc/bvh_ploc.hip)."""

    def __init__(self, builder):
        self.builder = builder
        self.handles = []

    def build(self, meshes, leaf_size, radius):
        """Issues every shell's build (vsa_bvh_dev_build, or vsa_bvh_dev_build_ploc at `radius`) on the current stream,
        then reads the sizes: one synchronisation per shell.  Returns their (nr_nodes, nr_tris, depth) in mesh order."""
        L = _lib.lib()
        dev = self.device = meshes[0].vertices.device
        if dev.type != "cuda":
            raise _lib.VolsurfsHipError(f'builder="{self.builder}" needs the meshes on the GPU')
        st = _lib.stream_ptr()
        name, rule = ("vsa_bvh_dev_build_ploc", (radius,)) if self.builder == "ploc" else ("vsa_bvh_dev_build", ())
        inputs = []             # (alive until the sizes calls have synchronised the builds that read them)
        for m in meshes:
            v = m.vertices.detach().to(dev, torch.float32).contiguous()
            f = m.faces.detach().to(dev, torch.int32).contiguous()
            inputs.append((v, f))
            h = ctypes.c_void_p()
            rc = getattr(L, name)(v.data_ptr(), f.data_ptr(), v.shape[0], f.shape[0], leaf_size, *rule, st,
                                  ctypes.byref(h))
            if rc != 0:
                raise _lib.VolsurfsHipError(f"{name} failed with status {rc}")
            self.handles.append(h)
        sizes = []
        for h in self.handles:
            rc, size = _sizes(L.vsa_bvh_dev_sizes, h)
            if rc == -2 and size[2] >= 48:
                raise _lib.VolsurfsHipError(
                    f'builder="{self.builder}": tree depth {size[2]} >= 48, deeper than the traversal stack; '
                    'build this mesh with builder="host"')
            if rc != 0:
                raise _lib.VolsurfsHipError(f"vsa_bvh_dev_sizes failed with status {rc}")
            sizes.append(size)
        return sizes

    def export(self, layout, nodes, qnodes, tris, frames):
        """Both node formats and the triangles written in place into the concatenated device arrays, the K
        quantisation frames into the host array `frames`."""
        L = _lib.lib()
        st = _lib.stream_ptr()
        for i, (h, (nb, nn, tb, nt)) in enumerate(zip(self.handles, layout)):
            rc = L.vsa_bvh_dev_export(h, nodes[nb].data_ptr(), qnodes[nb].data_ptr(), tris[tb].data_ptr(), nb, tb,
                                      ctypes.addressof(frames) + 24 * i, st)
            if rc != 0:
                raise _lib.VolsurfsHipError(f"vsa_bvh_dev_export failed with status {rc}")

    def refit(self, meshes):
        L = _lib.lib()
        st = _lib.stream_ptr()
        for h, m in zip(self.handles, meshes):
            v = m.vertices.detach().to(self.device, torch.float32).contiguous()
            rc = L.vsa_bvh_dev_refit(h, v.data_ptr(), v.shape[0], st)
            if rc != 0:
                raise _lib.VolsurfsHipError(f"vsa_bvh_dev_refit failed with status {rc} (vertex count changed?)")

    def destroy(self):
        for h in self.handles:
            _lib.lib().vsa_bvh_dev_destroy(h)
        self.handles = []


def _trees(builder):
    """The one place that knows which builder is which."""
    if builder == "host":
        return _HostTrees()
    if builder in RayTracer.DEVICE_BUILDERS:
        return _DeviceTrees(builder)
    raise _lib.VolsurfsHipError(f"unknown builder {builder!r} (expected one of {RayTracer.BUILDERS})")


class RayTracer:
    BUILDERS = ("host", "device", "ploc")
    DEVICE_BUILDERS = ("device", "ploc")
    PLOC_RADIUS = 8                                 # builder="ploc"'s default search radius

    def __init__(self, tensor_meshes, leaf_size=4, node_format=None, builder="host", ploc_radius=None):
        """builder: "host" (default; binned-SAH trees built on the CPU from host copies of the meshes,
        csrc/bvh_build.cpp), "device" (Karras LBVH built on the GPU from the meshes' device tensors,
        csrc/bvh_device.hip: no host copy, milliseconds instead of seconds, a higher SAH cost) or "ploc" (PLOC
        clustering on the GPU from the device tensors, csrc/bvh_ploc.hip: no host copy, milliseconds, close to
        the host tree's SAH cost; ploc_radius = its search radius 1..32, default PLOC_RADIUS).  All three give
        bit-identical hits.
        node_format: "q16" (default; binary 32-byte quantised nodes, vsa_trace_q / vsa_trace_q_fb) or
        "f32" (binary 64-byte fp32 nodes, vsa_trace); also selected by VSA_TRACE_NODES.  Both give
        identical hits; the quantised format assumes ray origins within ~60 mesh extents of the mesh
        (include/volsurfs_hip.h)."""
        self._trees = _trees(builder)               # (the builder's handles, kept for refit)
        self.builder = builder
        self.node_format = node_format or os.environ.get("VSA_TRACE_NODES", "q16")
        if self.node_format not in ("q16", "f32"):
            raise _lib.VolsurfsHipError(f"unknown node_format {self.node_format}")
        # q16 only: launch order from the previous call's measured cost (vsa_trace_q_fb; identical hits)
        self.cost_feedback = os.environ.get("VSA_TRACE_FEEDBACK", "1") != "0"
        self._meshes = list(tensor_meshes)
        self._drop_geometry_state()
        K = self.nr_meshes = len(tensor_meshes)
        if not 1 <= K <= 16:
            raise _lib.VolsurfsHipError("RayTracer supports 1..16 meshes")
        try:
            sizes = self._trees.build(self._meshes, leaf_size, self.PLOC_RADIUS if ploc_radius is None else ploc_radius)
        except Exception:
            self._trees.destroy()
            raise
        nr_nodes, nr_tris = self._record_shells(sizes)
        dev = self.device = tensor_meshes[0].vertices.device
        self.nodes = torch.empty(nr_nodes, 16, dtype=torch.float32, device=dev)
        self.qnodes = torch.empty(nr_nodes, 8, dtype=torch.int32, device=dev)
        self.tris = torch.empty(nr_tris, 12, dtype=torch.float32, device=dev)
        self._frames = (ctypes.c_float * (6 * K))()         # the K quantisation frames (host)
        self._trees.export(self._layout, self.nodes, self.qnodes, self.tris, self._frames)
        # original face id of every leaf-ordered triangle slot (for uv tables etc.)
        self.slot_face_id = self.tris[:, 3].contiguous().view(torch.int32)

    def slot_face_uvs(self, meshes):
        """[slots, 6]: the per-corner UVs of `meshes` (this tracer's shells, in its order) gathered into the tracer's
        leaf (slot) order, the table `tex_uv_only` and the texture stages index by hit slot."""
        fu = []
        for m, off, n in zip(meshes, self.mesh_tri_offset, self.mesh_nr_tris):
            fu.append(m.get_faces_uvs().reshape(-1, 6)[self.slot_face_id[off:off + n].long()])
        return torch.cat(fu, 0).contiguous()

    def _record_shells(self, sizes):
        """The shells' (nr_nodes, nr_tris, depth), in mesh order, into the layout of the concatenated arrays: `_layout`
        ((node_base, nr_nodes, tri_base, nr_tris) per shell), `mesh_tri_offset`, `mesh_nr_tris`, `max_depth` and the
        roots.  Returns the totals (nr_nodes, nr_tris)."""
        self._layout, self.max_depth = [], 0
        node_base = tri_base = 0
        for nn, nt, md in sizes:
            self._layout.append((node_base, nn, tri_base, nt))
            self.max_depth = max(self.max_depth, md)
            node_base += nn
            tri_base += nt
        self.mesh_tri_offset = [lay[2] for lay in self._layout]
        self.mesh_nr_tris = [lay[3] for lay in self._layout]
        self.roots = [lay[0] for lay in self._layout]
        self._roots = (ctypes.c_int32 * self.nr_meshes)(*self.roots)
        return node_base, tri_base

    def _drop_geometry_state(self):
        """Forget what belongs to the meshes' geometry, each rebuilt on first use: the cost feedback's measured launch
        order (`_fb`), the pseudonormal tables (`_pn`), the winding moments (`_wm`) and the edge census (`_census`)."""
        self._fb = self._pn = self._wm = self._census = None

    def refit(self, tensor_meshes):
        """The shells' vertices moved (same faces): recompute triangle records and boxes bottom-up in the
        existing trees (vsa_bvh_refit / vsa_bvh_dev_refit) and overwrite the arrays in place — no rebuild, triangle
        slots (and with them `slot_face_id` and any per-slot uv table) unchanged.  Hits through the
        refitted trees are bit-identical to a rebuild's (tests/test_raytrace.py::test_refit_*,
        tests/test_bvh_device.py::test_device_refit_*, tests/test_bvh_ploc.py::test_ploc_refit_*).
        SURVEY §8f row 1; replaces re-running RayTracer(tensor_meshes) (volsurfs.py:82-128)."""
        if len(tensor_meshes) != self.nr_meshes:
            raise _lib.VolsurfsHipError("refit needs the meshes the tracer was built on")
        self._meshes = list(tensor_meshes)
        self._drop_geometry_state()
        self._trees.refit(self._meshes)
        self._trees.export(self._layout, self.nodes, self.qnodes, self.tris, self._frames)
        return self

    def __del__(self):
        try:
            self._trees.destroy()
        except Exception:
            pass

    @classmethod
    def over(cls, meshes, nr_shells=None, builder="device"):
        """`meshes` itself when it is a RayTracer, else a tracer built over this list of meshes with `builder`.
        nr_shells: the number of shells it must have (ValueError)."""
        tracer = meshes if isinstance(meshes, cls) else cls(list(meshes), builder=builder)
        if nr_shells is not None and tracer.nr_meshes != nr_shells:
            raise ValueError(f"a tracer of {tracer.nr_meshes} shells for {nr_shells} meshes")
        return tracer

    def trace_all(self, rays_o, rays_d, t_min=0.0, out=None):
        """All K shells, one launch.  Returns hit_t [K,N] f32, hit_slot [K,N]
        i32 (global index into self.tris, -1 = miss), hit_uv [K,N,2] f32 (written into `out` = that triple when given)."""
        N, rays_o, rays_d = _rays(rays_o, rays_d)
        K = self.nr_meshes
        if out is not None:
            hit_t, hit_slot, hit_uv = out
            _lib.check_f32(hit_t, K, N)
            _lib.check_f32(hit_uv, K, N, 2)
            if hit_slot.dtype != torch.int32 or tuple(hit_slot.shape) != (K, N) or not hit_slot.is_contiguous():
                raise _lib.VolsurfsHipError("trace_all: out[1] must be a contiguous int32 [K, N] tensor")
        else:
            hit_t = torch.empty(K, N, device=rays_o.device)
            hit_slot = torch.empty(K, N, dtype=torch.int32, device=rays_o.device)
            hit_uv = torch.empty(K, N, 2, device=rays_o.device)
        # small batches (a training batch's few ten thousand random rays: ~2 waves per SIMD, each the maximum of 64
        # unrelated walks): narrow waves — fewer rays per wave, more waves (vsa_trace_q_narrow; same hits).  The launch-order
        # feedback has nothing to learn from random rays (profiles/NOTEBOOK.md round 5)
        rpw = self.narrow_rays_per_wave(N, K) if self.node_format == "q16" else 64
        if rpw < 64:
            _lib.call("vsa_trace_q_narrow", *self.q16_tree_args(), rays_o, rays_d, N, float(t_min), hit_t, hit_slot,
                      hit_uv, int(rpw), _lib.stream_ptr())
        elif self.node_format == "q16" and self.cost_feedback and self.max_depth < 48:
            if self._fb is None or self._fb[1] < N or self._fb[0].device != rays_o.device:   # grows only
                nbytes = _lib.workspace_bytes("vsa_trace_feedback_bytes", N, K)
                self._fb = [torch.zeros(nbytes, dtype=torch.uint8, device=rays_o.device), N, nbytes]
            # phase 2: the read / written halves alternate through a word in the buffer, flipped on the
            # device in front of every launch, so a captured graph alternates them on every replay too
            _lib.call("vsa_trace_q_fb", *self.q16_tree_args(), rays_o, rays_d, N, float(t_min), hit_t, hit_slot, hit_uv,
                      self._fb[0], ctypes.c_longlong(self._fb[2]), 2, _lib.stream_ptr())
        elif self.node_format == "q16":
            _lib.call("vsa_trace_q", *self.q16_tree_args(), rays_o, rays_d, N, float(t_min), hit_t, hit_slot, hit_uv,
                      _lib.stream_ptr())
        else:
            _lib.call("vsa_trace", self.nodes, self.tris, self._roots, K, self.max_depth, rays_o,
                      rays_d, N, float(t_min), hit_t, hit_slot, hit_uv, _lib.stream_ptr())
        return hit_t, hit_slot, hit_uv

    # narrow waves (vsa_trace_q_narrow: NARROW_RPW rays per 64-lane wave) below this many (ray, shell) walks; 0 = never.
    # Measured on MI355X (tools/trace_narrow_ab.py, profiles/r06/trace_narrow_ab.txt): 34 000 random rays x 5 shells
    # 0.108 ms -> 0.132 (worse), 8 000 rays 0.080 -> 0.069 at 8 per wave: off by default, the hits do not depend on it
    NARROW_BELOW = int(os.environ.get("VSA_TRACE_NARROW_BELOW", "0"))
    NARROW_RPW = 16

    @staticmethod
    def coop_config(chunk=16, lanes=24, max_waves=4096):
        """Process-wide setting of the traversal's cooperative finish (vsa_trace_coop_config: in launches of at most
        `max_waves` waves a wave whose last `lanes` rays are still walking finishes them together; lanes = 0: never).
        The hits do not depend on it."""
        _lib.call("vsa_trace_coop_config", int(chunk), int(lanes), ctypes.c_longlong(int(max_waves)))

    def narrow_rays_per_wave(self, N, K):
        return self.NARROW_RPW if N * K < self.NARROW_BELOW else 64

    @staticmethod
    def _counted(name, counters, device, *args):
        """{counter: value} of one `name(*args, counters, stream)`: a walk with int64 counters.  Synchronises."""
        st = torch.zeros(len(counters), dtype=torch.int64, device=device)
        _lib.call(name, *args, st, _lib.stream_ptr())
        return dict(zip(counters, st.cpu().tolist()))

    def walk_stats(self, rays_o, rays_d, t_min=0.0):
        """{lane_visits, tri_tests, wave_trips, waves, max_wave_trips} of one traversal of these rays
        (vsa_trace_q_stats: the same walk with counters; q16 nodes).  Synchronises; measurement only."""
        N, rays_o, rays_d = _rays(rays_o, rays_d)
        return self._counted("vsa_trace_q_stats", ("lane_visits", "tri_tests", "wave_trips", "waves", "max_wave_trips"),
                             rays_o.device, *self.q16_tree_args(), rays_o, rays_d, N, float(t_min))

    def face_view_counts(self, cameras, supersample=1, t_min=0.0):
        """Per shell, how many samples of how many views had each face as the shell's closest hit: a list of K int64
        [F_k] tensors (vsa_face_view_counts: rays made in registers, the walk of `trace_all`, hits counted per face in
        one launch; q16 nodes).  `visibility.face_view_counts` is the same call from a list of meshes."""
        from .visibility import tracer_face_view_counts
        return tracer_face_view_counts(self, cameras, supersample, t_min)

    raster_stats = None         # the `rasterize.RasterStats` of the last `rasterize` call

    def rasterize(self, camera, supersample=1, t_min=0.0, out=None, want_dirs=False):
        """`trace_all`'s (hit_t, hit_slot, hit_uv), bit for bit, for every sample of one camera, by screen-space bins
        instead of BVH walks (vsa_shell_raster_setup / _draw; include/volsurfs_hip.h "Shell rasterization", DESIGN
        §35): N = H W s^2 samples, pixel-major, a pixel's s x s samples consecutive (j outer, i inner), sample (i, j)
        through (col + (i + 0.5) / s, row + (j + 0.5) / s) as in `face_view_counts`; s = 1 is the unjittered rays of
        `get_camera_rays`.  No ray is written or read and no node is walked: any builder, either node format.
        `out` as `trace_all` takes it; want_dirs adds rays_d [N, 3] to the result (the origin is the camera centre).
        t_min must be >= 0.  One blocking read (the pair list is sized from it); `raster_stats` has the call's
        (behind, straddling, binned, pairs)."""
        from .rasterize import tracer_rasterize
        return tracer_rasterize(self, camera, supersample, t_min, out, want_dirs)

    def _shells(self, mesh_id=None):
        """(mesh_roots, mesh_frames, nr_meshes) of all K shells, or of shell `mesh_id` alone as a tracer of one shell."""
        if mesh_id is None:
            return self._roots, self._frames, self.nr_meshes
        frame = ctypes.c_void_p(ctypes.addressof(self._frames) + 24 * int(mesh_id))   # (six floats per shell, host)
        return (ctypes.c_int32 * 1)(self.roots[mesh_id]), frame, 1

    def q16_tree_args(self, mesh_id=None):
        """The leading arguments of the q16 entry points (qnodes, tris, mesh_roots, mesh_frames, nr_meshes, max_depth):
        of all K shells, or of shell `mesh_id` alone as a tracer of one shell."""
        return (self.qnodes, self.tris, *self._shells(mesh_id), self.max_depth)

    def require_q16(self, what, walk=True):
        """Raises unless `what` can use this tracer's quantised nodes and (walk) walk them with the traversal stack."""
        if self.node_format != "q16":
            raise _lib.VolsurfsHipError(
                f'{what} walks the quantised nodes: the tracer was built with node_format="{self.node_format}", '
                'build it with node_format="q16"')
        if walk and self.max_depth >= 48:
            raise _lib.VolsurfsHipError(f"tree depth {self.max_depth} >= 48, deeper than the traversal stack")

    def _points(self, points, what):
        """The query points of `what` as a checked contiguous f32 [N, 3] tensor; raises without q16 nodes."""
        self.require_q16(what)
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
            raise _lib.VolsurfsHipError(f"{what}: expected points [N, 3] with N >= 1, got "
                                        f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points)}")
        return _lib.check_f32(points.contiguous(), points.shape[0], 3)

    def _check_mesh_id(self, mesh_id, what):
        if mesh_id is not None and not 0 <= mesh_id < self.nr_meshes:
            raise _lib.VolsurfsHipError(f"{what}: mesh_id {mesh_id} outside 0..{self.nr_meshes - 1}")

    def _table_args(self, rule, mesh_id):
        """(table, first row per shell) of the sign rule's table, the pseudonormals or the winding moments: of all K
        shells, or of shell `mesh_id` alone."""
        table, base = self.winding_moments() if rule == "winding" else self.pseudonormal_tables()
        return table, base if mesh_id is None else (ctypes.c_longlong * 1)(base[mesh_id])

    def _closest(self, name, points, mesh_id, *table_args):
        """{dist, face, slot, bary} of one closest-point entry point (vsa_closest_point_q, vsa_signed_distance_q or
        vsa_signed_distance_w_q with its table arguments) for all K shells ([K, N] results; mesh_id None) or one ([N])."""
        N = points.shape[0]
        shape = (self.nr_meshes, N) if mesh_id is None else (N,)
        dist = torch.empty(shape, device=points.device)
        slot = torch.empty(shape, dtype=torch.int32, device=points.device)
        bary = torch.empty(*shape, 2, device=points.device)
        _lib.call(name, *self.q16_tree_args(mesh_id), *table_args, points, N, dist, slot, bary, _lib.stream_ptr())
        return {"dist": dist, "face": self._slot_faces(slot), "slot": slot, "bary": bary}

    def closest_all(self, points):
        """The closest point of every shell to every query point, one launch (vsa_closest_point_q: the closest-point walk
        of the q16 nodes, the result of brute force over all triangles bit for bit; queries within ~60 mesh extents).
        points [N, 3] f32 -> {dist [K, N] f32, face [K, N] i64 (original face ids), slot [K, N] i32 (global index into
        self.tris), bary [K, N, 2] f32 (the weights of the face's second and third vertex)}.  No host sync."""
        return self._closest("vsa_closest_point_q", self._points(points, "closest_all"), None)

    def closest(self, points, mesh_id=0):
        """`closest_all` for one shell: dist [N], face [N], slot [N], bary [N, 2]."""
        points, mesh_id = self._points(points, "closest"), int(mesh_id)
        self._check_mesh_id(mesh_id, "closest")
        return self._closest("vsa_closest_point_q", points, mesh_id)

    def pseudonormal_tables(self):
        """(table [sum F_k, 7, 3] f32, face_base [K] host long long): the pseudonormals of every face of every shell
        (vsa_mesh_pseudonormals; `mesh_sdf.pseudonormals` per mesh, one after the other) and each shell's first row.
        Built on first use from the tracer's meshes and kept; `refit` drops them."""
        if self._pn is None:
            from .mesh_sdf import pseudonormals
            tables = [pseudonormals(m, device=self.device) for m in self._meshes]
            base = np.cumsum([0] + [t.shape[0] for t in tables[:-1]])
            self._pn = (torch.cat(tables) if len(tables) > 1 else tables[0],
                        (ctypes.c_longlong * self.nr_meshes)(*[int(b) for b in base]))
        return self._pn

    SIGNS = ("pseudonormal", "winding", "auto")

    def winding_moments(self):
        """(table [2 nr_nodes + K, 8] f32, root_entry [K] host long long): per subtree of every shell's q16 tree the
        area vector N = sum 1/2 e1 x e2, the area-weighted centroid and a radius about it (vsa_mesh_winding_moments;
        include/volsurfs_hip.h "Mesh winding number"): entry 2 n + c for child c of node n, then one per
        shell root; an entry is N.xyz, r, p.xyz, 0.  Built on first use and kept; `refit` drops it.  The same tracer
        gives the same bytes."""
        if self._wm is None:
            self.require_q16("winding_moments")
            nn, nt, K = self.qnodes.shape[0], self.tris.shape[0], self.nr_meshes
            nbytes = _lib.workspace_bytes("vsa_mesh_winding_moments_workspace_bytes", nn, K)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            table = torch.empty(2 * nn + K, 8, device=self.device)
            _lib.call("vsa_mesh_winding_moments", self.qnodes, self.tris, self._roots, K, nn, nt, ws, nbytes, table,
                      _lib.stream_ptr())
            self._wm = (table, (ctypes.c_longlong * K)(*[2 * nn + k for k in range(K)]))
        return self._wm

    def edge_census(self, mesh_id=0):
        """{boundary, non_manifold, inconsistent} of shell `mesh_id` (`mesh_winding.edge_census`), kept until `refit`."""
        if self._census is None:
            self._census = [None] * self.nr_meshes
        if self._census[mesh_id] is None:
            from .mesh_winding import edge_census
            self._census[mesh_id] = edge_census(self._meshes[mesh_id], device=self.device)
        return self._census[mesh_id]

    @classmethod
    def _check_sign(cls, sign):
        if sign not in cls.SIGNS:
            raise ValueError(f"sign must be one of {cls.SIGNS}, got {sign!r}")

    def sign_rule(self, sign, mesh_ids=None):
        """"pseudonormal" or "winding": what `sign` means for these shells (all of them by default).  "auto" is the
        winding number iff the edge census of one of them finds a boundary, a non-manifold or an inconsistently wound
        edge.  Anything else raises ValueError."""
        self._check_sign(sign)
        if sign != "auto":
            return sign
        ids = range(self.nr_meshes) if mesh_ids is None else mesh_ids
        return "winding" if any(any(self.edge_census(k).values()) for k in ids) else "pseudonormal"

    @staticmethod
    def _check_beta(beta):
        beta = float(beta)
        if not beta > 1.0:
            raise ValueError(f"beta must be > 1 (math.inf: every leaf is summed exactly), got {beta}")
        return beta

    def _winding_args(self, what, points, mesh_id, beta):
        """(checked points, the arguments of vsa_winding_number_q / _stats in front of them: qnodes, tris, mesh_roots,
        nr_meshes, max_depth, moments, moment_roots, beta), for all K shells or for shell `mesh_id`."""
        points, beta = self._points(points, what), self._check_beta(beta)
        self._check_mesh_id(mesh_id, what)
        roots, _, K = self._shells(mesh_id)
        return points, (self.qnodes, self.tris, roots, K, self.max_depth, *self._table_args("winding", mesh_id), beta)

    def _winding(self, what, points, mesh_id, beta):
        """w [K, N] of all K shells, or w [N] of shell `mesh_id`."""
        points, args = self._winding_args(what, points, mesh_id, beta)
        N = points.shape[0]
        w = torch.empty((self.nr_meshes, N) if mesh_id is None else (N,), device=points.device)
        _lib.call("vsa_winding_number_q", *args, points, N, w, _lib.stream_ptr())
        return w

    def winding_number_all(self, points, beta=2.0):
        """w [K, N] f32: the generalised winding number of every shell at points [N, 3] f32, one launch
        (vsa_winding_number_q): about 1 inside and about 0 outside for outward-wound faces, in between
        across a hole, the multiplicity where parts overlap.  Returned raw: threshold it as you see fit (the signed
        queries use w > 1/2).  Subtrees farther than beta times their radius are taken by their area vector (Barill
        et al. 2018, order 0); beta must be > 1, math.inf sums every triangle exactly.  A NaN query gives NaN.  No
        host sync once the moments exist."""
        return self._winding("winding_number_all", points, None, beta)

    def winding_number(self, points, mesh_id=0, beta=2.0):
        """`winding_number_all` for one shell: w [N]."""
        return self._winding("winding_number", points, int(mesh_id), beta)

    def winding_stats(self, points, beta=2.0):
        """{node_visits, tri_terms, queries} of one `winding_number_all` of these points, summed over the K shells
        (vsa_winding_number_q_stats: the same walk with counters).  Synchronises; measurement only."""
        points, args = self._winding_args("winding_stats", points, None, beta)
        return self._counted("vsa_winding_number_q_stats", ("node_visits", "tri_terms", "queries"), points.device, *args,
                             points, points.shape[0])

    def _signed(self, what, points, mesh_id, sign, beta):
        """`_closest` signed by what `sign` means for these shells; beta is checked where the winding number uses it."""
        points = self._points(points, what)
        self._check_sign(sign)
        self._check_mesh_id(mesh_id, what)
        if self.sign_rule(sign, None if mesh_id is None else [mesh_id]) == "winding":
            beta = self._check_beta(beta)
            return self._closest("vsa_signed_distance_w_q", points, mesh_id, *self._table_args("winding", mesh_id), beta)
        return self._closest("vsa_signed_distance_q", points, mesh_id, *self._table_args("pseudonormal", mesh_id))

    def signed_distance_all(self, points, sign="pseudonormal", beta=2.0):
        """`closest_all` with `dist` signed; |dist|, face, slot and bary are `closest_all`'s bits.
        sign="pseudonormal" (default; vsa_signed_distance_q; include/volsurfs_hip.h "Mesh signed distance", DESIGN
        §29): negative inside a closed shell whose faces wind outward, by the angle-weighted pseudonormal of the
        closest feature; a point on the surface gets +0.  It means inside / outside for closed, consistently oriented
        shells only; for any other mesh it is whatever the rule gives.
        sign="winding" (vsa_signed_distance_w_q; "Mesh winding number"): negative iff the winding number
        `winding_number_all(points, beta)` exceeds 1/2, for outward-wound faces.  It also holds for open,
        self-intersecting and inconsistently wound meshes: across a hole the level sets close with the w = 1/2
        membrane, where the field jumps from -d to +d.
        sign="auto": the winding number iff `edge_census` finds anything on a shell, else the pseudonormal.
        No host sync once the tables exist."""
        return self._signed("signed_distance_all", points, None, sign, beta)

    def signed_distance(self, points, mesh_id=0, sign="pseudonormal", beta=2.0):
        """`signed_distance_all` for one shell: dist [N] (signed), face [N], slot [N], bary [N, 2]."""
        return self._signed("signed_distance", points, int(mesh_id), sign, beta)

    def _slot_faces(self, slot):
        """Original face ids of triangle slots (-1 stays -1: a query with a NaN coordinate has no closest face)."""
        face = self.slot_face_id[slot.clamp_min(0).long()].long()
        return torch.where(slot >= 0, face, torch.full_like(face, -1))

    def closest_stats(self, points):
        """{node_visits, tri_tests, queries} of one `closest_all` of these points, summed over the K shells
        (vsa_closest_point_q_stats: the same walk with counters).  Synchronises; measurement only."""
        points = self._points(points, "closest_stats")
        return self._counted("vsa_closest_point_q_stats", ("node_visits", "tri_tests", "queries"), points.device,
                             *self.q16_tree_args(), points, points.shape[0])

    def crossings(self, mesh, mesh_id=0, segments=False):
        """Which faces of `mesh` (a cuda TensorMesh, or (RayTracer, mesh_id)) cross which faces of shell `mesh_id`:
        `mesh_intersect.mesh_crossings(mesh, (self, mesh_id), segments)` -- a `Crossings` of (face of mesh, face of the
        shell) pairs decided by the fp64 rule of DESIGN §33 over a box-overlap walk of the shell's q16 tree
        (vsa_mesh_cross_count / vsa_mesh_cross_emit).  One blocking read."""
        from .mesh_intersect import mesh_crossings
        return mesh_crossings(mesh, (self, int(mesh_id)), segments)

    def untangle(self, mesh_id, against, side, margin=1e-3, max_rounds=16, max_level=6, sign="pseudonormal", beta=2.0,
                 log=None):
        """Move the vertices of shell `mesh_id` until it clears shell `against` on `side` (+1: outside it, -1: inside
        it): one pair of `shell_untangle.untangle_shells` (vsa_shell_untangle_project / _escalate around the crossing
        count pass; include/volsurfs_hip.h "Shell untangling").  The shell's mesh is replaced by a new
        TensorMesh with the same faces and UVs and the tracer is `refit`.  Returns an `UntangleReport`; one blocking
        read per round."""
        from .shell_untangle import untangle_pair
        return untangle_pair(self, mesh_id, against, side, margin, max_rounds, max_level, sign, beta, log)

    def sah_cost(self):
        """Per-mesh SAH cost of the trees, from the fp32 nodes (measurement; copies them to the host):
        1 (the root's visit) + sum over every child box of area / root area x (1 for an inner node, its triangle
        count for a leaf).  Lower is a better tree for the same geometry."""
        nodes = self.nodes.cpu().numpy()
        out = []
        for nb, nn, _, _ in self._layout:
            nd = nodes[nb:nb + nn, :12].astype(np.float64)                             # (12:16 are int bits)
            ref = nodes[nb:nb + nn, 12:14].copy().view(np.int32)
            cnt = nodes[nb:nb + nn, 14:16].copy().view(np.int32)
            w = np.where(ref >= 0, 1.0, cnt.astype(np.float64))                     # empty child: cnt 0
            area = np.zeros((nn, 2))
            for c in range(2):
                ext = np.clip(nd[:, 6 * c + 3:6 * c + 6] - nd[:, 6 * c:6 * c + 3], 0.0, None)
                area[:, c] = 2.0 * (ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 2] * ext[:, 0])
            live = w[0] > 0
            lo = nd[0, [0, 6]][live].min(), nd[0, [1, 7]][live].min(), nd[0, [2, 8]][live].min()
            hi = nd[0, [3, 9]][live].max(), nd[0, [4, 10]][live].max(), nd[0, [5, 11]][live].max()
            e = np.subtract(hi, lo)
            root_area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
            out.append(1.0 + float((area * w).sum()) / root_area)
        return out

    def feedback_header(self):
        """{tag, n0, n1, n2} of the half the LAST cost-feedback launch wrote (tests, diagnostics)."""
        half = ((self._fb[2] - 256) // 2) & ~255
        ph = int(self._fb[0][2 * half:2 * half + 4].view(torch.int32).item()) & 1
        return self._fb[0][(ph ^ 1) * half:][:16].view(torch.int32).cpu().tolist()

    def trace(self, rays_o, rays_d, mesh_id=0, t_min=0.0):
        """raytracelib-shaped single-mesh trace (volsurfs.py:480-501)."""
        N, rays_o, rays_d = _rays(rays_o, rays_d)
        dev = rays_o.device
        hit_t = torch.empty(1, N, device=dev)
        hit_slot = torch.empty(1, N, dtype=torch.int32, device=dev)
        hit_uv = torch.empty(1, N, 2, device=dev)
        root = (ctypes.c_int32 * 1)(self.roots[mesh_id])
        st = _lib.stream_ptr()
        _lib.call("vsa_trace", self.nodes, self.tris, root, 1, self.max_depth, rays_o, rays_d, N,
                  float(t_min), hit_t, hit_slot, hit_uv, st)
        is_hit = torch.empty(N, dtype=torch.uint8, device=dev)
        tri_id = torch.empty(N, dtype=torch.int32, device=dev)
        pos = torch.empty(N, 3, device=dev)
        nrm = torch.empty(N, 3, device=dev)
        bary = torch.empty(N, 3, device=dev)
        _lib.call("vsa_hit_attributes", self.tris, rays_o, rays_d, hit_t, hit_slot, hit_uv, N,
                  is_hit, tri_id, pos, nrm, bary, st)
        is_hit = is_hit.bool()
        return {
            "any_hit": bool(is_hit.any().item()),  # host sync, as in the reference (volsurfs.py:481)
            "is_hit": is_hit,
            "triangles_id": tri_id.long(),
            "depth": hit_t[0],
            "positions": pos,
            "normals": nrm,
            "barycentric": bary,
        }
