"""The cases that hold for any device builder of RayTracer, builder="device" (the Karras LBVH, csrc/bvh_device.hip)
or builder="ploc" (PLOC clustering, csrc/bvh_ploc.hip), each taking the builder as its first argument, and their
helpers.  tests/test_bvh_device.py and tests/test_bvh_ploc.py run them; not a test module itself.

The traversal's closest hit is the minimum over (t, original face id) and the boxes only prune, so every tree with
conservative boxes gives bit-identical hits: the trees are pinned against the brute-force oracle and against the
host tree with no tolerances."""
import numpy as np
import pytest
import torch

from oracle import raytrace as oracle_rt
from tests.test_raytrace import _chain_mesh, _rays
from volsurfs_amd.mesh import icosphere


def face_ids(rt, hit_slot):
    return torch.where(hit_slot >= 0, rt.slot_face_id[hit_slot.clamp(min=0).long()],
                       torch.full_like(hit_slot, -1))


def perturbed_spheres(subdiv, k=3, seed=None, scale=0.05):
    g = np.random.default_rng(subdiv if seed is None else seed)
    out = []
    for i in range(k):
        v, f = icosphere(subdiv, 0.3 + 0.02 * i)
        out.append(((v * (1 + scale * g.standard_normal((v.shape[0], 1)))).astype(np.float32), f))
    return out


def assert_same_hits(a, b, rt_a, rt_b):
    assert torch.equal(face_ids(rt_a, a[1]), face_ids(rt_b, b[1]))
    assert torch.equal(a[0], b[0])
    hit = (a[1] >= 0).unsqueeze(-1).expand_as(a[2])
    assert torch.equal(a[2][hit], b[2][hit])


def builder_needs_the_meshes_on_the_gpu(builder):
    from volsurfs_amd import _lib
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.raytrace import RayTracer
    assert builder in RayTracer.BUILDERS
    v, f = icosphere(1, 0.3)
    with pytest.raises(_lib.VolsurfsHipError, match=f'builder="{builder}" needs the meshes on the GPU'):
        RayTracer([TensorMesh(v, f, device="cpu")], builder=builder)


def tree_bit_exact_vs_bruteforce(builder, subdiv, n, fmt):
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.raytrace import RayTracer
    meshes_np = perturbed_spheres(subdiv)
    rt = RayTracer([TensorMesh(v, f) for v, f in meshes_np], node_format=fmt, builder=builder)
    assert rt.builder == builder
    o, d = _rays(n, subdiv)
    oc, dc = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    hit_t, hit_slot, hit_uv = rt.trace_all(oc, dc)
    face_id = face_ids(rt, hit_slot).cpu().numpy()
    for k, (v, f) in enumerate(meshes_np):
        ref = oracle_rt.trace_bruteforce(v, f, o, d)
        assert (ref["tri"] >= 0).sum() > n // 20
        assert np.array_equal(face_id[k], ref["tri"])
        assert np.array_equal(hit_t[k].cpu().numpy(), ref["t"])
        m = ref["tri"] >= 0
        assert np.array_equal(hit_uv[k].cpu().numpy()[m], ref["uv"][m])
        res = rt.trace(oc, dc, mesh_id=k)
        att = oracle_rt.hit_attributes(v, f, o, d, ref)
        assert res["any_hit"] == att["any_hit"]
        assert np.array_equal(res["is_hit"].cpu().numpy(), att["is_hit"])
        assert np.array_equal(res["triangles_id"].cpu().numpy(), att["triangles_id"])
        np.testing.assert_allclose(res["positions"].cpu().numpy(), att["positions"], atol=1e-6)
        np.testing.assert_allclose(res["normals"].cpu().numpy(), att["normals"], atol=1e-6)
        np.testing.assert_allclose(res["barycentric"].cpu().numpy(), att["barycentric"], atol=1e-6)


def tree_equals_host_tree_on_every_traversal_form(builder):
    from volsurfs_amd.camera import pinhole_rays
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.raytrace import RayTracer
    meshes = nested_shells(K=5, subdiv=6)
    host, dev = RayTracer(meshes), RayTracer(meshes, builder=builder)
    assert dev.builder == builder and dev.mesh_nr_tris == host.mesh_nr_tris and dev.mesh_tri_offset == host.mesh_tri_offset
    o, d = pinhole_rays(800, 800, focal=1111.1, cam_pos=(0, 0, -1.5))
    ref = [x.clone() for x in host.trace_all(o, d)]
    assert (ref[1] >= 0).sum().item() > 500000
    for _ in range(2):                                   # cost feedback: no order yet / measured on the same rays
        assert_same_hits(dev.trace_all(o, d), ref, dev, host)
    dev.cost_feedback = False
    assert_same_hits(dev.trace_all(o, d), ref, dev, host)
    dev.cost_feedback = True
    # narrow waves, and the cooperative finish of a small launch (a slice of the frame through its centre)
    n = 9000
    os_, ds_ = o[320000:320000 + n].contiguous(), d[320000:320000 + n].contiguous()
    ref_s = [x.clone() for x in host.trace_all(os_, ds_)]
    dev.NARROW_BELOW, dev.NARROW_RPW = 1 << 30, 16
    assert dev.narrow_rays_per_wave(n, 5) == 16
    assert_same_hits(dev.trace_all(os_, ds_), ref_s, dev, host)
    dev.NARROW_BELOW = 0
    try:
        RayTracer.coop_config(1, 64, 8192)             # every small launch finishes cooperatively at once
        for _ in range(2):
            assert_same_hits(dev.trace_all(os_, ds_), ref_s, dev, host)
    finally:
        RayTracer.coop_config()
    assert (ref_s[1] >= 0).sum().item() > n


def check_structure(rt, meshes_np, leaf_size):
    nodes = rt.nodes.cpu().numpy()
    qnodes = rt.qnodes.cpu().numpy().view(np.uint32)
    tris = rt.tris.cpu().numpy()
    frames = np.array(rt._frames[:], np.float32).reshape(-1, 6)
    for k, ((v, f), (nb, nn, tb, nt)) in enumerate(zip(meshes_np, rt._layout)):
        assert rt.roots[k] == nb and nt == f.shape[0]
        T = tris[tb:tb + nt]
        ids = T[:, 3].copy().view(np.int32)
        assert np.array_equal(np.sort(ids), np.arange(f.shape[0]))                 # every face exactly once
        a, b, c = v[f[ids, 0]], v[f[ids, 1]], v[f[ids, 2]]
        want = np.zeros_like(T)
        want[:, 0:3], want[:, 4:7], want[:, 8:11] = a, b - a, c - a
        want[:, 3] = T[:, 3]
        assert np.array_equal(T.view(np.int32), want.view(np.int32))              # the host formula, bit for bit
        N = nodes[nb:nb + nn]
        ref = N[:, 12:14].copy().view(np.int32)
        cnt = N[:, 14:16].copy().view(np.int32)
        inner = ref >= 0
        empty = (ref < 0) & (cnt == 0)
        leaf = (ref < 0) & (cnt > 0)
        # every node except the root referenced exactly once, children after their parent (pre-order)
        kids = ref[inner] - nb
        assert np.array_equal(np.sort(kids), np.arange(1, nn))
        parent_of = np.full(nn, -1)
        for i in range(nn):
            for ch in range(2):
                if inner[i, ch]:
                    assert ref[i, ch] - nb > i
                    parent_of[ref[i, ch] - nb] = i
        assert np.all((cnt[leaf] >= 1) & (cnt[leaf] <= leaf_size)) and np.all(cnt[inner] == 0)
        assert empty.sum() == (1 if nn == 1 and f.shape[0] <= leaf_size else 0)
        first = ~ref[leaf] - tb
        order = np.argsort(first)
        assert np.array_equal(np.cumsum(cnt[leaf][order])[:-1], first[order][1:])   # leaves partition the slots
        assert first.min() == 0 and first.max() + cnt[leaf][np.argmax(first)] == nt
        # subtree slot ranges bottom-up (children have larger indices), tri boxes inside every fp32 child box
        tlo = np.minimum(np.minimum(a, b), c)
        thi = np.maximum(np.maximum(a, b), c)
        span = np.zeros((nn, 2), np.int64)
        for i in range(nn - 1, -1, -1):
            lo_s, hi_s = [], []
            for ch in range(2):
                if inner[i, ch]:
                    s0, s1 = span[ref[i, ch] - nb]
                elif leaf[i, ch]:
                    s0, s1 = ~ref[i, ch] - tb, ~ref[i, ch] - tb + cnt[i, ch]
                else:
                    continue
                assert np.all(tlo[s0:s1] >= N[i, 6 * ch:6 * ch + 3]) and np.all(thi[s0:s1] <= N[i, 6 * ch + 3:6 * ch + 6])
                lo_s.append(s0)
                hi_s.append(s1)
            span[i] = min(lo_s), max(hi_s)
        assert tuple(span[0]) == (0, nt)
        # de-quantised q16 boxes contain the fp32 boxes
        Q = qnodes[nb:nb + nn]
        fr = frames[k].astype(np.float64)
        q = np.stack([Q[:, 0] & 0xffff, Q[:, 0] >> 16, Q[:, 1] & 0xffff, Q[:, 1] >> 16, Q[:, 2] & 0xffff, Q[:, 2] >> 16,
                      Q[:, 3] & 0xffff, Q[:, 3] >> 16, Q[:, 4] & 0xffff, Q[:, 4] >> 16, Q[:, 5] & 0xffff, Q[:, 5] >> 16], 1)
        qref = Q[:, 6:8].view(np.int32)
        for ch in range(2):
            live = ~empty[:, ch]
            qlo = fr[:3] + (q[:, 6 * ch:6 * ch + 3].astype(np.float64) - 1.0) * fr[3:]
            qhi = fr[:3] + (q[:, 6 * ch + 3:6 * ch + 6].astype(np.float64) - 1.0) * fr[3:]
            assert np.all(qlo[live] <= N[live, 6 * ch:6 * ch + 3]) and np.all(qhi[live] >= N[live, 6 * ch + 3:6 * ch + 6])
            assert np.array_equal(qref[inner[:, ch], ch], ref[inner[:, ch], ch])
            lf = leaf[:, ch]
            assert np.array_equal(qref[lf, ch], ~(((~ref[lf, ch]) << 4) | cnt[lf, ch]))
            assert np.all(qref[empty[:, ch], ch] == 0x7fffffff)
        # max_depth = the deepest leaf's number of inner ancestors
        depth = np.zeros(nn, np.int64)
        for i in range(1, nn):
            depth[i] = depth[parent_of[i]] + 1
        want_depth = 0 if nn == 1 and empty.any() else int((depth[:, None] + 1)[leaf.any(1)].max())
        assert rt._dev_depth[k] == want_depth


def shell_depth(mesh, leaf_size, builder):
    from volsurfs_amd.raytrace import RayTracer
    return RayTracer([mesh], leaf_size=leaf_size, builder=builder).max_depth


def tree_structure(builder, leaf_size):
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.raytrace import RayTracer
    meshes_np = perturbed_spheres(4, k=2, seed=7) + [icosphere(2, 0.5)]
    rt = RayTracer([TensorMesh(v, f) for v, f in meshes_np], leaf_size=leaf_size, builder=builder)
    # (the tracer keeps the deepest shell's depth: each shell's own comes from a build of that shell alone)
    rt._dev_depth = [shell_depth(TensorMesh(v, f), leaf_size, builder) for v, f in meshes_np]
    assert rt.max_depth == max(rt._dev_depth)
    check_structure(rt, meshes_np, leaf_size)


def assert_deterministic(meshes, **kw):
    from volsurfs_amd.raytrace import RayTracer
    a, b = RayTracer(meshes, **kw), RayTracer(meshes, **kw)
    assert a._layout == b._layout and a.max_depth == b.max_depth
    assert torch.equal(a.nodes.view(torch.int32), b.nodes.view(torch.int32))
    assert torch.equal(a.qnodes, b.qnodes) and torch.equal(a.tris.view(torch.int32), b.tris.view(torch.int32))
    assert list(a._frames) == list(b._frames)
    return a


def tree_edge_cases(builder, fmt):
    from volsurfs_amd import _lib
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.raytrace import RayTracer
    # one face (the wrapped root), two faces
    one = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    two = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], np.float32), np.array([[0, 1, 2], [1, 3, 2]], np.int32))
    for leaf_size in (1, 4):
        meshes_np = [one, two]
        rt = RayTracer([TensorMesh(v, f) for v, f in meshes_np], leaf_size=leaf_size, node_format=fmt, builder=builder)
        rt._dev_depth = [0, 0 if leaf_size >= 2 else 1]
        check_structure(rt, meshes_np, leaf_size)
        g = np.random.default_rng(3)
        o = np.concatenate([g.random((500, 2)) * 1.4 - 0.2, -np.ones((500, 1))], 1).astype(np.float32)
        d = np.tile(np.array([[0, 0, 1]], np.float32), (500, 1))
        t, s, uv = rt.trace_all(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
        fid = face_ids(rt, s).cpu().numpy()
        for k, (v, f) in enumerate(meshes_np):
            ref = oracle_rt.trace_bruteforce(v, f, o, d)
            assert (ref["tri"] >= 0).sum() > 100
            assert np.array_equal(fid[k], ref["tri"]) and np.array_equal(t[k].cpu().numpy(), ref["t"])
    # every triangle with the same centroid: all Morton codes equal, the LBVH's split goes by index, PLOC's clustering
    # by area alone
    g = np.random.default_rng(4)
    nt = 3000
    a = g.standard_normal((nt, 3)).astype(np.float32) * 0.3
    q = a * g.uniform(-1, 1, (nt, 3)).astype(np.float32)          # |q| <= |a| per axis: box centre 0 for every face
    v = np.concatenate([a, -a, q]).astype(np.float32)
    f = np.stack([np.arange(nt), np.arange(nt) + nt, np.arange(nt) + 2 * nt], 1).astype(np.int32)
    rt = RayTracer([TensorMesh(v, f)], node_format=fmt, builder=builder)
    rt._dev_depth = [rt.max_depth]
    check_structure(rt, [(v, f)], 4)
    if builder == "device":
        assert rt.max_depth <= 12                               # a balanced split of 3000 by index
    o, d = _rays(2000, 5)
    t, s, uv = rt.trace_all(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    ref = oracle_rt.trace_bruteforce(v, f, o, d)
    assert (ref["tri"] >= 0).sum() > 200
    assert np.array_equal(face_ids(rt, s)[0].cpu().numpy(), ref["tri"]) and np.array_equal(t[0].cpu().numpy(), ref["t"])
    if builder == "ploc":
        # identical boxes: every area ties, and the tie order pairs neighbours (a balanced tree, not a chain)
        v = np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (1000, 1))
        f = np.arange(3000, dtype=np.int32).reshape(1000, 3)
        rt = RayTracer([TensorMesh(v, f)], node_format=fmt, builder="ploc")
        rt._dev_depth = [rt.max_depth]
        check_structure(rt, [(v, f)], 4)
        assert rt.max_depth <= 10                               # 1000 triangles paired level by level
    # the chain mesh, deep for the host's SAH: bounded in the LBVH by the Morton codes, which must build it; PLOC
    # builds it below the traversal stack, or refuses it naming "host"
    v, f = _chain_mesh()
    v2, f2 = icosphere(3, 0.4)
    try:
        rt = RayTracer([TensorMesh(v, f), TensorMesh(v2, f2)], node_format=fmt, builder=builder)
    except _lib.VolsurfsHipError as e:
        assert builder == "ploc" and 'builder="host"' in str(e) and ">= 48" in str(e)
        print("chain mesh:", e)
        return
    print("chain mesh: depth", rt.max_depth)
    assert rt.max_depth < 48
    g = np.random.default_rng(1)
    n = 6000
    i = g.integers(0, 20, n)
    tgt = np.stack([3.0 ** -i, np.zeros(n), np.zeros(n)], 1) + (0.2 * 3.0 ** -i)[:, None] * g.standard_normal((n, 3))
    o = np.tile(np.array([[0.2, 0.05, -2.0]]), (n, 1)) + 0.01 * g.standard_normal((n, 3))
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = o.astype(np.float32), d.astype(np.float32)
    hit_t, hit_slot, hit_uv = rt.trace_all(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    face_id = face_ids(rt, hit_slot).cpu().numpy()
    for k, (vv, ff) in enumerate([(v, f), (v2, f2)]):
        ref = oracle_rt.trace_bruteforce(vv, ff, o, d)
        # the well-conditioned hits of tests/test_raytrace.py::test_trace_deep_bvh_takes_the_48_entry_stack_bit_exact
        ok = np.ones(n, bool) if k else ((ref["tri"] // 64 < 12) & (face_id[k] // 64 < 12))
        assert ok.mean() > 0.5
        assert np.array_equal(face_id[k][ok], ref["tri"][ok])
        assert np.array_equal(hit_t[k].cpu().numpy()[ok], ref["t"][ok])
        m = (ref["tri"] >= 0) & ok
        assert np.array_equal(hit_uv[k].cpu().numpy()[m], ref["uv"][m])


def refit_after_the_vertices_moved_is_bit_exact_and_keeps_the_slots(builder, fmt):
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.raytrace import RayTracer
    g = np.random.default_rng(5)
    base = [icosphere(4, 0.3 + 0.03 * k) for k in range(3)]
    rt = RayTracer([TensorMesh(v, f) for v, f in base], node_format=fmt, builder=builder)
    slots_before = rt.slot_face_id.clone()
    o, d = _rays(5000, 9)
    oc, dc = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    rt.trace_all(oc, dc)                                    # leaves a cost-feedback state behind
    shear = np.array([[1.0, 0.15, 0.0], [0.0, 1.0, 0.1], [0.05, 0.0, 1.0]], np.float32)
    moved = [(((v * (1 + 0.06 * g.standard_normal((v.shape[0], 1)))) @ shear).astype(np.float32), f) for v, f in base]
    rt.refit([TensorMesh(v, f) for v, f in moved])
    assert rt._fb is None
    assert torch.equal(rt.slot_face_id, slots_before)
    fresh = RayTracer([TensorMesh(v, f) for v, f in moved], node_format=fmt, builder=builder)
    for _ in range(2):
        hit_t, hit_slot, hit_uv = rt.trace_all(oc, dc)
    ft, fs, fu = fresh.trace_all(oc, dc)
    face_id = face_ids(rt, hit_slot).cpu().numpy()
    assert np.array_equal(face_id, face_ids(fresh, fs).cpu().numpy()) and torch.equal(hit_t, ft)
    assert torch.equal(hit_uv, fu)
    for k, (v, f) in enumerate(moved):
        ref = oracle_rt.trace_bruteforce(v, f, o, d)
        assert (ref["tri"] >= 0).sum() > 250
        assert np.array_equal(face_id[k], ref["tri"])
        assert np.array_equal(hit_t[k].cpu().numpy(), ref["t"])
        m = ref["tri"] >= 0
        assert np.array_equal(hit_uv[k].cpu().numpy()[m], ref["uv"][m])
    rt._dev_depth = [shell_depth(TensorMesh(v, f), 4, builder) for v, f in base]
    check_structure(rt, moved, 4)
    with pytest.raises(Exception):
        rt.refit([TensorMesh(v[:-1], f) for v, f in moved])          # another vertex count: refused


def volsurfs_with_the_tree_renders_the_host_trees_pixels(builder):
    from volsurfs_amd.camera import pinhole_rays
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.methods import VolSurfs
    o, d = pinhole_rays(64, 64, focal=110.0)
    gt = torch.rand(o.shape[0], 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    out = []
    for bvh_builder in ("host", builder):
        m = VolSurfs(nested_shells(K=2, subdiv=3), max_rays=4096, textures_res=(256, 128, 64, 32), bvh_builder=bvh_builder)
        assert m.raytracer.builder == bvh_builder
        g = torch.Generator().manual_seed(0)
        with torch.no_grad():
            m.bank.tables.copy_((torch.rand(m.bank.tables.shape, generator=g) * 2 - 1).cuda())
        m.bank.refresh_half_params()
        m.grad_scale = float(o.shape[0])
        rgb = m.render_rays(o, d)["renders"]["ray_traced"]["rgb"]
        (rgb.float() - gt).abs().mean().backward()
        out.append((rgb.detach().clone(), m.bank.tables.grad.clone(), m.bank.weights.grad.clone()))
    (rgb_h, gt_h, gw_h), (rgb_d, gt_d, gw_d) = out
    assert torch.equal(rgb_h, rgb_d)
    # The gradients run through the f16 chain and float atomics whose order follows the triangle slots, which differ
    # between the trees: measured on MI355X for the LBVH, 1.1e-3 of the tables' largest entry (the smoke test's bound
    # against the oracle is 1e-3); the bound, for both builders, is 5x that.
    for name, a, b in (("tables", gt_d, gt_h), ("weights", gw_d, gw_h)):
        assert b.abs().max() > 0
        rel = float((a - b).abs().max() / b.abs().max())
        cos = float(torch.nn.functional.cosine_similarity(a.flatten(), b.flatten(), dim=0))
        print(f"{name}: max error {rel:.2e} of the largest entry, cos {cos:.7f}")
        assert rel <= 5e-3 and cos > 0.99999, (name, rel, cos)


def pipeline_step_with_the_tree_equals_the_host_trees(builder):
    from volsurfs_amd.pipeline import KShellPipeline
    res = []
    for bvh_builder in ("host", builder):
        p = KShellPipeline.synthetic(K=2, subdiv=2, res=64, bvh_builder=bvh_builder)
        assert p.tracer.builder == bvh_builder
        res.append(p.step().detach().clone())
    assert torch.equal(res[0], res[1])
