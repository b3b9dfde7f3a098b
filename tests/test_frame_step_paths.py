"""The neural-texture step's launch order, path by path (DESIGN "The neural-texture step, written once").

Every caller of the step — autograd, the fused eager step, the graph loop's iteration, the three cuts of
`KShellPipeline.step`, the texel fit and the baked render — is driven once on a tiny scene with `_lib.call` wrapped: each
C-ABI call is recorded as (entry point, its int / float / bool arguments in order); a hash-grid backward launch also
records `vsa_nt_plan.grads_zeroed` as it stands at the call.  The recorded traces must equal EXPECTED below.

EXPECTED was printed by this file's own recorder (`python tests/test_frame_step_paths.py`) on commit 384d79a, the last
one that wrote the step out by hand in five places: the traces pin that commit's launch order and scalar arguments.
"""
import contextlib
import ctypes

import pytest
import torch

K, SUBDIV, RAYS, SIDE = 2, 2, 256, 16
TEX_RES = (64, 32, 16, 8)         # the smallest textures the suite builds a method with


# ---------------------------------------------------------------------------------------------------------------------
# the recorder

def _scalar(a):
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, (int, float)):
        return a
    if isinstance(a, ctypes._SimpleCData) and not isinstance(a, (ctypes.c_void_p, ctypes.c_char_p, ctypes.c_wchar_p)):
        return a.value
    return None


@contextlib.contextmanager
def _recording(monkeypatch_or_none=None):
    """Every `_lib.call` inside the block, as a list of tuples."""
    from volsurfs_amd import _lib
    real, trace = _lib.call, []

    def call(name, *args):
        rec = [name] + [s for s in map(_scalar, args) if s is not None]
        if name.startswith("vsa_nt_encode_bwd"):
            rec.append(("grads_zeroed", int(args[0]._obj.grads_zeroed)))
        trace.append(tuple(rec))
        return real(name, *args)
    if monkeypatch_or_none is not None:
        monkeypatch_or_none.setattr(_lib, "call", call)
        yield trace
        monkeypatch_or_none.setattr(_lib, "call", real)
    else:
        _lib.call = call
        try:
            yield trace
        finally:
            _lib.call = real


# ---------------------------------------------------------------------------------------------------------------------
# the paths

def _method(seed=3):
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.methods import VolSurfs
    m = VolSurfs(nested_shells(K=K, subdiv=SUBDIV), max_rays=RAYS, textures_res=TEX_RES, seed=seed)
    m.init_optim()
    return m


def _batch():
    from volsurfs_amd.camera import pinhole_rays
    o, d = pinhole_rays(SIDE, SIDE, focal=20.0, cam_pos=(0.0, 0.0, -1.5))
    gt = torch.rand(RAYS, 3, generator=torch.Generator().manual_seed(1)).cuda()
    return o.contiguous(), d.contiguous(), gt


def _pipeline():
    from volsurfs_amd.pipeline import KShellPipeline
    return KShellPipeline.synthetic(K=K, subdiv=SUBDIV, res=SIDE, seed=3)


def record_all(mp=None):
    """{path name: trace} of every caller of the step."""
    import bench
    from volsurfs_amd.parallel import StepSignals
    from volsurfs_amd.texture_fit import TextureFit
    from volsurfs_amd.trainer import GraphTrainLoop
    out = {}
    o, d, gt = _batch()

    m = _method()
    with _recording(mp) as t:
        rgb = m.render_rays(o, d, return_samples=False)["renders"]["ray_traced"]["rgb"]
        (gt - rgb).abs().mean().backward()
    out["autograd"] = t

    m = _method()
    m.optimizer.step()
    with _recording(mp) as t:
        m.fused_forward_backward(o, d, gt)
    out["fused_after_step"] = t
    with _recording(mp) as t:
        m.fused_forward_backward(o, d, gt)
    out["fused_again"] = t

    m = _method()
    loop = GraphTrainLoop(m, bench.synthetic_reel(2, SIDE, "cuda", seed=3), RAYS, 300, capacity=RAYS)
    with _recording(mp) as t:
        loop._iteration()
    out["graph_iteration"] = t

    pipe = _pipeline()
    with _recording(mp) as t:
        pipe.step()
    out["pipeline_step"] = t
    with _recording(mp) as t:
        for part in ("prefix", "mid", "tail"):
            pipe.step(part=part)
    out["pipeline_parts"] = t
    with _recording(mp) as t:
        pipe.step(grad_ready=lambda g: None)
    out["pipeline_grad_ready"] = t
    sg = StepSignals(K, "cuda")
    with _recording(mp) as t:
        pipe.step(dp=sg)
    out["pipeline_dp"] = t

    m = _method()
    m.bake()
    fit = TextureFit(m)
    with _recording(mp) as t:
        fit.accumulate(o, d, gt)
        fit.step()
    out["texture_fit"] = t
    with _recording(mp) as t:
        m.render_baked(o, d)
    out["render_baked"] = t
    torch.cuda.synchronize()
    return out


EXPECTED = {
 'autograd': [('vsa_trace_q_fb', 2, 8, 256, 0.0, 2304, 2), ('vsa_nt_mark', 256), ('vsa_nt_compact_frame',),
              ('vsa_nt_encode_fwd',), ('vsa_nt_mlp_fwd',), ('vsa_nt_shade_fwd', 256),
              ('vsa_composite_dense_fwd', 1, 256, 2, 0), ('vsa_composite_dense_bwd', 1, 256, 2, 0),
              ('vsa_nt_shade_bwd', 256, 1024.0), ('vsa_nt_mlp_bwd', 0.0009765625),
              ('vsa_nt_encode_bwd', 1024.0, ('grads_zeroed', 0))],
 'fused_after_step': [('vsa_trace_q_fb', 2, 8, 256, 0.0, 2304, 2), ('vsa_count_hits', 512), ('vsa_nt_mark', 256),
                      ('vsa_nt_compact_frame',), ('vsa_nt_encode_fwd',), ('vsa_nt_mlp_fwd',),
                      ('vsa_nt_shade_fwd', 256),
                      ('vsa_composite_dense_fwd_bwd_l1', 1, 0.0013020833333333333, 256, 2, 0),
                      ('vsa_nt_shade_bwd', 256, 4096.0), ('vsa_nt_mlp_bwd', 0.000244140625),
                      ('vsa_nt_encode_bwd', 4096.0, ('grads_zeroed', 1)), ('vsa_l1_mean', 768)],
 'fused_again': [('vsa_trace_q_fb', 2, 8, 256, 0.0, 2304, 2), ('vsa_count_hits', 512), ('vsa_nt_mark', 256),
                 ('vsa_nt_compact_frame',), ('vsa_nt_encode_fwd',), ('vsa_nt_mlp_fwd',), ('vsa_nt_shade_fwd', 256),
                 ('vsa_composite_dense_fwd_bwd_l1', 1, 0.0013020833333333333, 256, 2, 0),
                 ('vsa_nt_shade_bwd', 256, 4096.0), ('vsa_nt_mlp_bwd', 0.000244140625),
                 ('vsa_nt_encode_bwd', 4096.0, ('grads_zeroed', 0)), ('vsa_l1_mean', 768)],
 'graph_iteration': [('vsa_adam_step_ctl', 2800, 0.9, 0.99, 1e-15, 1.0, 1, 512),
                     ('vsa_reel_next_rays_batch_ctl', 2, 16, 16, 256, 1, 1),
                     ('vsa_trace_q_fb', 2, 8, 256, 0.0, 2304, 2), ('vsa_count_hits', 512), ('vsa_nt_mark', 256),
                     ('vsa_nt_compact_frame',), ('vsa_nt_encode_fwd',), ('vsa_nt_mlp_fwd',),
                     ('vsa_nt_shade_fwd', 256), ('vsa_composite_dense_fwd_bwd_l1_ctl', 1, 256, 2, 0),
                     ('vsa_nt_shade_bwd', 256, 4096.0), ('vsa_nt_mlp_bwd', 0.000244140625),
                     ('vsa_nt_encode_bwd', 4096.0, ('grads_zeroed', 1)), ('vsa_l1_mean_ctl', 256),
                     ('vsa_train_ctl_tick',)],
 'pipeline_dp': [('vsa_tile_order_rays', 16, 16), ('vsa_trace_q_fb', 2, 8, 256, 0.0, 2304, 2), ('vsa_nt_mark', 256),
                 ('vsa_nt_compact_frame',), ('vsa_nt_encode_fwd',), ('vsa_nt_mlp_fwd',), ('vsa_nt_shade_fwd', 256),
                 ('vsa_composite_dense_fwd_bwd_l1', 1, 0.0013020833333333333, 256, 2, 0),
                 ('vsa_tile_order', 16, 16, 3, 1), ('vsa_nt_shade_bwd', 256, 4096.0),
                 ('vsa_nt_mlp_bwd', 0.000244140625), ('vsa_dp_signal', 2, 1),
                 ('vsa_nt_encode_bwd_phased', 4096.0, 2, 0, ('grads_zeroed', 1))],
 'pipeline_grad_ready': [('vsa_tile_order_rays', 16, 16), ('vsa_trace_q_fb', 2, 8, 256, 0.0, 2304, 2),
                         ('vsa_nt_mark', 256), ('vsa_nt_compact_frame',), ('vsa_nt_encode_fwd',), ('vsa_nt_mlp_fwd',),
                         ('vsa_nt_shade_fwd', 256),
                         ('vsa_composite_dense_fwd_bwd_l1', 1, 0.0013020833333333333, 256, 2, 0),
                         ('vsa_tile_order', 16, 16, 3, 1), ('vsa_nt_shade_bwd', 256, 4096.0),
                         ('vsa_nt_mlp_bwd', 0.000244140625),
                         ('vsa_nt_encode_bwd_range', 4096.0, 0, 1, ('grads_zeroed', 1)),
                         ('vsa_nt_encode_bwd_range', 4096.0, 1, 2, ('grads_zeroed', 0))],
 'pipeline_parts': [('vsa_tile_order_rays', 16, 16), ('vsa_trace_q_fb', 2, 8, 256, 0.0, 2304, 2),
                    ('vsa_nt_mark', 256), ('vsa_nt_compact_frame',), ('vsa_nt_encode_fwd',), ('vsa_nt_mlp_fwd',),
                    ('vsa_nt_shade_fwd', 256),
                    ('vsa_composite_dense_fwd_bwd_l1', 1, 0.0013020833333333333, 256, 2, 0),
                    ('vsa_tile_order', 16, 16, 3, 1), ('vsa_nt_shade_bwd', 256, 4096.0),
                    ('vsa_nt_mlp_bwd', 0.000244140625), ('vsa_nt_encode_bwd', 4096.0, ('grads_zeroed', 1))],
 'pipeline_step': [('vsa_tile_order_rays', 16, 16), ('vsa_trace_q_fb', 2, 8, 256, 0.0, 2304, 2), ('vsa_nt_mark', 256),
                   ('vsa_nt_compact_frame',), ('vsa_nt_encode_fwd',), ('vsa_nt_mlp_fwd',), ('vsa_nt_shade_fwd', 256),
                   ('vsa_composite_dense_fwd_bwd_l1', 1, 0.0013020833333333333, 256, 2, 0),
                   ('vsa_tile_order', 16, 16, 3, 1), ('vsa_nt_shade_bwd', 256, 4096.0),
                   ('vsa_nt_mlp_bwd', 0.000244140625), ('vsa_nt_encode_bwd', 4096.0, ('grads_zeroed', 1))],
 'render_baked': [('vsa_trace_q_fb', 2, 8, 256, 0.0, 2304, 2), ('vsa_nt_mark', 256), ('vsa_nt_shade_fwd', 256),
                  ('vsa_composite_dense_fwd', 1, 256, 2, 0)],
 'texture_fit': [('vsa_trace_q_fb', 2, 8, 256, 0.0, 2304, 2), ('vsa_nt_mark', 256), ('vsa_nt_shade_fwd', 256),
                 ('vsa_composite_dense_fwd_bwd_l1', 1, 0.0013020833333333333, 256, 2, 0),
                 ('vsa_nt_shade_bwd', 256, 4096.0), ('vsa_l1_mean', 768),
                 ('vsa_texel_fit_step', 0.000244140625, 0.001, 0.9, 0.99, 1e-15, 1)]}


@pytest.fixture(scope="module")
def traces():
    mp = pytest.MonkeyPatch()
    try:
        return record_all(mp)
    finally:
        mp.undo()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["autograd", "fused_after_step", "fused_again", "graph_iteration", "pipeline_step",
                                  "pipeline_parts", "pipeline_grad_ready", "pipeline_dp", "texture_fit", "render_baked"])
def test_launch_order_is_the_recorded_one(traces, path):
    assert traces[path] == EXPECTED[path]


def _grads_zeroed(trace):
    return [r[-1][1] for r in trace if r[0].startswith("vsa_nt_encode_bwd")]


@pytest.mark.gpu
def test_only_the_step_right_after_the_optimiser_stores(traces):
    """`grads_zeroed = 1` makes the hash-grid backward STORE a table plane: right after a FusedAdam step that is true,
    a second backward without a step in between must add."""
    assert _grads_zeroed(traces["fused_after_step"]) == [1]
    assert _grads_zeroed(traces["fused_again"]) == [0]


@pytest.mark.gpu
def test_backward_of_an_overwritten_frame_raises(monkeypatch):
    """A frame's backward reads the bank's per-frame state (slot_of, seg_start, texels, features): after a later
    `bank.frame(...)` it must refuse, on the fused path as on the autograd one."""
    from volsurfs_amd import _lib, composite
    m = _method()
    o, d, gt = _batch()
    bank, tris = m.bank, m.raytracer.tris
    _, hit_slot, hit_uv = m.raytracer.trace_all(o, d)
    first = bank.frame(hit_slot, hit_uv, m.face_uvs)
    rgb_k, alpha_k = first.forward(d, tris, differentiable=True)[:2]
    later = bank.frame(hit_slot, hit_uv, m.face_uvs)
    later.forward(d, tris, differentiable=True)
    g_c, g_a = torch.zeros_like(rgb_k), torch.zeros_like(alpha_k)
    with pytest.raises(_lib.VolsurfsHipError, match="per-frame texel state was overwritten"):
        first.backward(g_c, g_a, 16.0 * RAYS)
    later.backward(g_c, g_a, 16.0 * RAYS)
    # the fused eager step: another frame taken between its forward and its backward
    real = composite.composite_fwd_bwd_l1_raw

    def composite_then_another_frame(*a, **kw):
        res = real(*a, **kw)
        bank.frame(hit_slot, hit_uv, m.face_uvs)
        return res
    monkeypatch.setattr(composite, "composite_fwd_bwd_l1_raw", composite_then_another_frame)
    with pytest.raises(_lib.VolsurfsHipError, match="per-frame texel state was overwritten"):
        m.fused_forward_backward(o, d, gt)
    # autograd: render, render again, then the first loss's backward
    loss = (gt - m.render_rays(o, d, return_samples=False)["renders"]["ray_traced"]["rgb"]).abs().mean()
    m.render_rays(o, d, return_samples=False)
    with pytest.raises(_lib.VolsurfsHipError, match="per-frame texel state was overwritten"):
        loss.backward()


if __name__ == "__main__":         # the recorder: prints EXPECTED
    import os
    import pprint
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("EXPECTED = " + pprint.pformat(record_all(), width=118, compact=True))
