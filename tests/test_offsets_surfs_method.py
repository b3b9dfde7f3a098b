"""The OffsetsSurfs method (volsurfs_amd/offsets_surfs.py, models.OffsetsSDF): hyper-parameters, the offsets and
K-column field derivatives against the reference's own functions (fixture), the checkpoint layout, the render dict,
the row-batched appearance, the occupancy rule and cadence, frozen parameters through the init phases, and training
on a synthetic scene from a Surf checkpoint through meshing into the K-shell stages."""
import math
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "offsets_surfs.npz")

# ---- CPU


def test_hyper_parameter_defaults_are_the_reference_base_5_config():
    """params/hyper_params.py (HyperParamsOffsetsSuRFs) + config/offsets_surfs/base_5.cfg."""
    from volsurfs_amd.offsets_surfs import OffsetsSurfsHyperParams
    hp = OffsetsSurfsHyperParams()
    want = {"init_phase_end_iter": 2000, "color_init_phase_end_iter": 3000, "nr_warmup_iters": 1000,
            "lr_milestones": [40000, 45000, 47500], "nr_inner_surfs": 4, "nr_outer_surfs": 0,
            "delta_surfs_multiplier": 1.0, "training_end_iter": 50000, "first_phase_end_iter": 45000,
            "first_phase_variance_start_value": 0.7, "first_phase_variance_end_value": 1.0,
            "training_rays_batch_size": 512, "is_nr_training_rays_dynamic": True, "test_rays_batch_size": 16384,
            "is_training_masked": False, "is_testing_masked": False, "mask_weight": 0.0, "geom_feat_size": 32,
            "sdf_encoding_type": "permutohash", "sdf_mlp_layers_dims": [32, 32, 32],
            "rgb_pos_encoder_type": "permutohash", "rgb_dir_encoder_type": "spherical_harmonics",
            "rgb_mlp_layers_dims": [128, 128, 64], "sh_degree": 3, "appearance_predict_sh_coeffs": False,
            "are_surfs_colors_indep": False, "are_surfs_transparency_indep": False, "is_inner_surf_solid": False,
            "rgb_view_dep": True, "rgb_normal_dep": True, "rgb_geom_feat_dep": True, "transp_view_dep": True,
            "transp_normal_dep": True, "transp_geom_feat_dep": True, "with_alpha_decay": True,
            "use_occupancy_grid": True, "do_importance_sampling": True, "max_nr_samples_per_ray": 64,
            "max_nr_imp_samples_per_ray": 32, "sdf_nr_iters_for_c2f": 0, "rgb_nr_iters_for_c2f": 0,
            "eikonal_weight": 0.04, "support_surfs_eikonal_weight": 0.04, "curvature_weight": 0.65,
            "lipshitz_weight": 0.0, "offsurface_weight": 1e-4, "offsets_weight": 0.0,
            "nr_training_rays_per_pixel": 1, "nr_test_rays_per_pixel": 1, "min_nr_samples_per_ray": 3}
    for k, v in want.items():
        assert getattr(hp, k) == v, k
    b1 = OffsetsSurfsHyperParams(nr_inner_surfs=0, are_surfs_colors_indep=True, are_surfs_transparency_indep=True,
                                 is_inner_surf_solid=True, with_alpha_decay=False)
    assert b1.nr_inner_surfs == 0 and b1.is_inner_surf_solid and not b1.with_alpha_decay
    with pytest.raises(KeyError):
        OffsetsSurfsHyperParams(not_a_key=1)
    for bad in ({"rgb_use_lipshitz_mlp": True}, {"lipshitz_weight": 0.1}, {"use_grad_scaler": True},
                {"use_color_calibration": True}):
        with pytest.raises(NotImplementedError):
            OffsetsSurfsHyperParams(**bad)


def _fixture_sdfs(K):
    def fn(p):
        r = p.norm(dim=-1, keepdim=True)
        base = r - 0.3 + 0.05 * torch.sin(5.0 * p[:, 0:1]) * torch.cos(3.0 * p[:, 1:2])
        shifts = (0.02, 0.0, -0.015, 0.03, -0.04, 0.01, 0.05, -0.025, 0.0)
        cols = [base + shifts[i] * torch.cos(4.0 * p[:, 2:3] + i) for i in range(K)]
        return torch.cat(cols, 1).unsqueeze(-1), None, None
    return fn


@pytest.mark.parametrize("K", [1, 3, 5, 9])
def test_offsets_and_field_derivatives_match_the_reference_fixture(K):
    """tools/make_golden.py gen_offsets ran the reference's get_offsets_gt, logistic_distribution_stdev,
    OffsetsSDF.get_offsets and the K-column get_field_gradients / get_sdf_curvature on CPU; the restatements give
    the same bits."""
    from volsurfs_amd.models import MLP, OffsetsSDF
    from volsurfs_amd.offsets_surfs import get_offsets_gt, get_sdfs_curvature
    from volsurfs_amd.surf import get_field_gradients, get_logistic_beta_from_variance, logistic_distribution_stdev
    d = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(d[k])
    for mult in (1.0, 0.25):
        delta = logistic_distribution_stdev(get_logistic_beta_from_variance(0.7)) * mult
        assert delta == float(d[f"delta_{K}_{mult}"])
        gt = get_offsets_gt(0, K - 1, delta)
        want = t(f"offsets_gt_{K}_{mult}")
        assert gt.dtype == want.dtype and torch.equal(gt, want)
    pts = t("field_points")
    fn = _fixture_sdfs(K)
    fg = get_field_gradients(fn, pts)
    assert torch.equal(fg, t(f"field_grad_{K}"))
    curv = get_sdfs_curvature(fn, pts, fg, t(f"curv_rand_dirs_{K}"), eps=1e-2)
    assert torch.equal(curv, t(f"curvature_eps1e2_{K}"))
    if K == 1:
        return
    heads = []
    for i in range(K - 1):
        h = MLP(32, [32, 1], last_layer_linear=True)
        h.load_state_dict({k[len(f"eps_{K}_{i}."):]: t(k) for k in d.files if k.startswith(f"eps_{K}_{i}.")},
                          strict=True)
        heads.append(h)
    host = SimpleNamespace(mlps_eps=heads, nr_outer_surfs=0, min_offset=1e-4)
    host._heads = lambda x: OffsetsSDF._heads(host, x)
    with torch.no_grad():
        got = OffsetsSDF.get_offsets(host, t("geom_feats"))
    for name, v in zip(("cum_inner", "cum_outer", "inner", "outer"), got):
        assert torch.equal(v, t(f"{name}_{K}")), name


# ---- GPU: the method's contract

def _surf_ckpt(tmp_path, radius=0.3, iters=0):
    """A Surf sphere init of `radius` (trained for `iters` sphere-init iterations), saved; -> its models folder.
    Without the coarse-to-fine schedule: OffsetsSDF runs every encoder level, as after a full surf run."""
    from test_surf_method import _method as surf_method
    from volsurfs_amd.camera import TensorReel
    from volsurfs_amd.trainer import train
    m = surf_method(bg_color=(0.0, 0.0, 0.0), init_sphere_radius=radius, save=str(tmp_path / "surf"),
                    hp={"lr": 3e-3, "init_phase_end_iter": max(iters, 1) + 1, "sdf_nr_iters_for_c2f": 0})
    if iters:
        from test_surf_method import _cameras, _gt_images
        cams = _cameras(4)
        train(TensorReel(cams, _gt_images(cams)), m, 0, iters, nr_training_rays=512)
    return m.save(iters)


def _method(models_path, **kw):
    from volsurfs_amd.background import BoundingSphere
    from volsurfs_amd.offsets_surfs import OffsetsSurfs, OffsetsSurfsHyperParams
    hp = OffsetsSurfsHyperParams(**{"nr_warmup_iters": 10, "init_phase_end_iter": 100,
                                    "color_init_phase_end_iter": 200, "first_phase_end_iter": 1000,
                                    "nr_inner_surfs": 2, **kw.pop("hp", {})})
    return OffsetsSurfs(True, hp, kw.pop("load", None), kw.pop("save", None), BoundingSphere(0.5), models_path,
                        bg_color=kw.pop("bg_color", (0.0, 0.0, 0.0)), start_iter_nr=kw.pop("start_iter_nr", 0))


def _rays(n, seed=0):
    from test_surf_method import _rays as surf_rays
    return surf_rays(n, seed)


@pytest.mark.gpu
def test_checkpoint_layout_is_the_reference_one(tmp_path):
    from volsurfs_amd.models import MLP, SDF, OffsetsSDF
    path = _surf_ckpt(tmp_path)
    m = _method(path, save=str(tmp_path / "off"))
    sdfs = m.models["sdfs"]
    keys = set(sdfs.state_dict())
    assert keys and all(k.startswith(("pos_encoder.", "mlp_sdf.")) for k in keys)
    # the reference's sdfs.pt <-> this model, both directions, strict
    ref_sdf = SDF(3, [32, 32, 32], "permutohash", geom_feat_size=32, bb_sides=1.0)
    sdfs.load_state_dict(ref_sdf.state_dict(), strict=True)
    ref_sdf.load_state_dict(sdfs.state_dict(), strict=True)
    head = MLP(32, [32, 1], last_layer_linear=True).cuda()
    for sd in sdfs.heads_state_dicts():
        head.load_state_dict(sd, strict=True)
    sdfs.load_heads_state_dicts([head.state_dict()] * len(sdfs.mlps_eps))
    # the main surface came from Surf.save's sdf.pt
    surf_sd = torch.load(os.path.join(path, "sdf.pt"))
    fresh = OffsetsSDF(nr_inner_surfs=2, nr_outer_surfs=0, bb_sides=1.0)
    fresh.load_main_sdf_ckpt(os.path.join(path, "sdf.pt"))
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, surf_sd[k]), k
    with pytest.raises(FileNotFoundError):
        _method(str(tmp_path / "nowhere"))
    # save / load round trip: sdfs.pt holds the main surface only, one sdfs_eps_<i>.pt per head
    out = m.save(7)
    assert sorted(f for f in os.listdir(out) if f.startswith("sdfs")) == ["sdfs.pt", "sdfs_eps_0.pt", "sdfs_eps_1.pt"]
    m2 = _method(None, load=str(tmp_path / "off"), start_iter_nr=7)
    pts = torch.rand(1000, 3, device="cuda") - 0.5
    with torch.no_grad():
        assert torch.equal(m.models["sdfs"](pts)[0], m2.models["sdfs"](pts)[0])
    # a checkpoint without one of its heads does not resume with random heads
    os.remove(os.path.join(out, "sdfs_eps_1.pt"))
    with pytest.raises(FileNotFoundError):
        _method(None, load=str(tmp_path / "off"), start_iter_nr=7)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 3, 5, 9, 12])
def test_grouped_offset_heads_equal_the_per_head_calls(K):
    """On the GPU the K - 1 heads run as one grouped fused-MLP launch over the replicated features (more than 8
    heads: two runs of groups); column i of [M, K - 1] is head i, forward and backward, as the reference's
    torch.stack of the per-head calls."""
    from volsurfs_amd.models import OffsetsSDF
    s = OffsetsSDF(nr_inner_surfs=K - 1, nr_outer_surfs=0, bb_sides=1.0)
    g = torch.Generator("cuda").manual_seed(K)
    feats = torch.randn(3000, 32, device="cuda", generator=g)
    gy = torch.randn(3000, K - 1, device="cuda", generator=g)
    outs = []
    for grouped in (True, False):
        x = feats.clone().requires_grad_(True)
        for p_ in s.heads_parameters():
            p_.grad = None
        y = s._heads(x) if grouped else torch.stack([h(x) for h in s.mlps_eps], dim=1).squeeze(dim=-1)
        (y * gy).sum().backward()
        outs.append((y.detach(), x.grad, [p_.grad.clone() for p_ in s.heads_parameters()]))
    (yg, xg, pg), (yr, xr, pr) = outs
    assert yg.shape == (3000, K - 1)
    torch.testing.assert_close(yg, yr, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(xg, xr, rtol=1e-5, atol=1e-6)     # the replicated features' gradients are summed
    for a, b in zip(pg, pr):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_render_dict_row_batched_appearance_and_occupancy(tmp_path):
    from volsurfs_amd.offsets_surfs import appearance_rows
    m = _method(_surf_ckpt(tmp_path, 0.3, iters=100), hp={"nr_inner_surfs": 2})
    # occupancy cadence: every 50 iterations and at each phase start, but not inside the colour init
    calls = []
    orig = m.update_occupancy_grid
    m.update_occupancy_grid = lambda iter_nr=None, decay=0.0: calls.append(iter_nr)
    for it in (50, 60, 120, 150, 160):
        m.update_method_state(it)
    assert calls == [50, 120]
    m.update_occupancy_grid = orig
    m.update_method_state(1000)
    o, d = _rays(256)
    res = m.render_rays(o, d, iter_nr=1000)
    vol = res["renders"]["volumetric"]
    N, K = 256, 3
    shapes = {"surfs_rgb": (N, K, 3), "surfs_normals": (N, K, 3), "surfs_depths": (N, K, 1),
              "surfs_weight_sum": (N, K, 1), "surfs_alpha": (N, K, 1), "surfs_transmittance": (N, K, 1),
              "surfs_blending_weights": (N, K, 1), "rgb_fg": (N, 3), "bg_transmittance": (N, 1), "rgb": (N, 3),
              "rgb_bg": (N, 3), "nr_samples": (N, 1)}
    for k, s in shapes.items():
        assert tuple(vol[k].shape) == s, k
    S = res["samples_3d"].shape[0]
    assert tuple(res["samples_grad"].shape) == (S, K, 3)
    # inner to outer: the outermost shell sees the ray first (transmittance 1), the inner ones behind it
    assert torch.equal(vol["surfs_transmittance"][:, K - 1], torch.ones(N, 1, device="cuda"))
    assert bool((vol["surfs_transmittance"][:, 0] <= vol["surfs_transmittance"][:, K - 1]).all())
    # the shared models over K S rows give the per-surface calls' values row for row
    pts = res["samples_3d"].detach()
    dirs = torch.nn.functional.normalize(torch.randn_like(pts), dim=-1)
    nrm = torch.nn.functional.normalize(torch.randn(S, K, 3, device="cuda"), dim=-1)
    feat = torch.randn(S, 32, device="cuda")
    with torch.no_grad():
        for key in ("rgb", "alpha"):
            rows = appearance_rows(m.models[key], pts, dirs, nrm, feat, 1000)
            for k in range(K):
                one = m.models[key](points=pts, samples_dirs=dirs, normals=nrm[:, k], iter_nr=1000, geom_feat=feat)
                assert torch.equal(rows[:, k], one), (key, k)
    # occupancy: min_k |sdf_k| over the grid
    m.variance = 1.0
    m.update_occupancy_grid(iter_nr=1000)
    g = m.occupancy_grid
    pts_g, idx = g.get_grid_samples(False)
    with torch.no_grad():
        sd = torch.abs(m.models["sdfs"](pts_g[:4096])[0].squeeze(-1)).min(dim=-1, keepdim=True)[0]
    assert torch.equal(g.get_grid_values()[idx[:4096].long()].view(-1, 1), sd)


@pytest.mark.gpu
def test_frozen_parameters_and_moments_stay_put_through_the_init_phases(tmp_path):
    from test_surf_method import _cameras, _gt_images
    from volsurfs_amd.camera import TensorReel
    from volsurfs_amd.trainer import train
    m = _method(_surf_ckpt(tmp_path, 0.3, iters=100), hp={"init_phase_end_iter": 20, "color_init_phase_end_iter": 40})
    s = m.models["sdfs"]
    main = list(s.pos_encoder.parameters()) + list(s.mlp_sdf.parameters())
    heads = s.heads_parameters()
    snap = lambda ps: [p_.detach().clone() for p_ in ps]
    moments = lambda ps: [(m.optimizer.state.get(p_, {}).get("exp_avg"), m.optimizer.state.get(p_, {}).get("exp_avg_sq"))
                          for p_ in ps]
    main0, heads_init = snap(main), snap(heads)
    cams = _cameras(4)
    reel = TensorReel(cams, _gt_images(cams))
    train(reel, m, 0, 20, nr_training_rays=256)          # offsets init: main frozen, heads move
    assert all(torch.equal(a, b) for a, b in zip(main0, main))
    assert not all(torch.equal(a, b) for a, b in zip(heads_init, heads))
    heads0, hm0 = snap(heads), [tuple(None if x is None else x.clone() for x in mm) for mm in moments(heads)]
    rgb0 = snap(m.models["rgb"].parameters())
    train(reel, m, 20, 40, nr_training_rays=256)         # colour init: main and heads frozen, appearance moves
    assert all(torch.equal(a, b) for a, b in zip(main0, main))
    assert all(torch.equal(a, b) for a, b in zip(heads0, heads))
    for (a0, b0), (a1, b1) in zip(hm0, moments(heads)):
        assert (a0 is None and a1 is None) or (torch.equal(a0, a1) and torch.equal(b0, b1))
    assert not all(torch.equal(a, b) for a, b in zip(rgb0, m.models["rgb"].parameters()))
    m.is_training = True
    m.update_method_state(40)                             # first phase: both train again
    assert s.is_training_main_surf and s.is_training_offsets and m.lr_scheduler is not None


# ---- GPU: end to end on the synthetic ball of tests/test_surf_method.py

# measured on MI355X: mean |offsets - gt| after the 1 000-iteration offsets init 1.44e-4, gaps after the
# colour init 1.00 and 1.00 delta (this schedule, one run; the offsets init drew the same bits in every run of the
# shorter one); held-out PSNR 27.4 / 32.4 / 31.7 dB over three runs of the same 1 200 data iterations after a shorter
# offsets init, 31.9 dB with this one; the outer shell within 0.0067 of the ball in all four.  Once the data phases
# train the offsets from images of an opaque ball, nothing in the images holds the hidden inner shells, so the
# shells are checked, meshed and handed on after the colour init, where the offsets still hold their init values.
# The error bound is twice the measured one, the gap band +-0.1 delta (about a tenth of a grid cell), the floor
# 2.4 dB below the lowest PSNR.
E2E = {"init": 1000, "color": 1200, "first": 2000, "end": 2200}
OFFSETS_ERR_MAX = 3e-4
PSNR_FLOOR = 25.0
GAP_BAND = (0.9, 1.1)          # the gaps between shells after the colour init, as multiples of delta


@pytest.mark.gpu
def test_train_synthetic_ball_from_a_surf_checkpoint_then_mesh_and_volsurfs(tmp_path):
    from test_surf_method import BALL_R, BG, _cameras, _closed_volume_radius, _gt_images
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.atlas import compute_atlas
    from volsurfs_amd.camera import TensorReel
    from volsurfs_amd.evaluation import render_and_eval
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.simplify import simplify_mesh
    from volsurfs_amd.surf import get_logistic_beta_from_variance, logistic_distribution_stdev
    from volsurfs_amd.trainer import train, train_step
    torch.manual_seed(0)
    t0 = time.time()
    path = _surf_ckpt(tmp_path, BALL_R, iters=300)
    train_cams, test_cams = _cameras(24), _cameras(4, seed=0.5)
    gt_train, gt_test = _gt_images(train_cams), _gt_images(test_cams)
    reel = TensorReel(train_cams, gt_train)
    # delta = stdev(beta(0.7)) multiplier ~ 0.01
    mult = 0.01 / logistic_distribution_stdev(get_logistic_beta_from_variance(0.7))
    m = _method(path, bg_color=BG, hp={"lr": 1e-3, "nr_warmup_iters": 100, "nr_inner_surfs": 2,
                                       "first_phase_variance_end_value": 0.8,
                                       "delta_surfs_multiplier": mult, "init_phase_end_iter": E2E["init"],
                                       "color_init_phase_end_iter": E2E["color"],
                                       "first_phase_end_iter": E2E["first"], "training_end_iter": E2E["end"]})
    kw = {"nr_training_rays": 512, "target_nr_of_training_samples": m.hyper_params.target_nr_of_training_samples}
    assert train(reel, m, 0, E2E["init"], **kw) == E2E["init"]
    with torch.no_grad():
        pts = m.bounding_primitive.get_random_points_inside(20000)
        _, feats = m.models["sdfs"].main_sdf(pts)
        off = torch.cat(m.models["sdfs"].get_offsets(feats)[:2], 1)
        err = float((off - m.offsets_gt.cuda().float()).abs().mean())
    t_train = time.time()
    assert train(reel, m, E2E["init"], E2E["color"], **kw) == E2E["color"]
    shells, levels = iso.extract_offsets_surfs_meshes(m, 128, iter_nr=E2E["color"])
    stats = [_closed_volume_radius(x) for x in shells]
    radii = [r for _, _, r in stats]
    gaps = [(radii[i + 1] - radii[i]) / m.delta_surfs for i in range(len(radii) - 1)]
    paths = iso.save_offsets_surfs_meshes(shells, str(tmp_path / "meshes"))
    assert train(reel, m, E2E["color"], E2E["end"], **kw) == E2E["end"]
    torch.cuda.synchronize()
    t_train = time.time() - t_train
    psnr = render_and_eval(m, {"test": (test_cams, gt_test)}, save_pngs=False)["test"]["psnr"]
    # the main (outermost) surface after the data phases; the hidden inner shells are not constrained by the images
    outer = iso.extract_offsets_surfs_meshes(m, 128, iter_nr=E2E["end"])[0][-1]
    o_closed, o_vol, o_r = _closed_volume_radius(outer)
    print(f"offsets_surfs e2e: delta {m.delta_surfs:.4f}, mean |offsets - gt| after init {err:.2e}, "
          f"{E2E['end'] - E2E['init']} iterations in {t_train:.1f} s, held-out PSNR {psnr:.2f} dB, shells after the "
          f"colour init: radii {[round(r, 4) for r in radii]}, gaps / delta {[round(g, 2) for g in gaps]}, "
          + ", ".join(f"closed={c} vol={v:.4f}" for c, v, _ in stats)
          + f"; outer shell at the end: radius {o_r:.4f} closed={o_closed} vol={o_vol:.4f}")
    assert levels == [0.0] * 3 and [os.path.basename(p_) for p_ in paths] == ["0.ply", "1.ply", "2.ply"]
    assert err < OFFSETS_ERR_MAX
    assert all(c and v > 0 for c, v, _ in stats)
    assert radii[0] < radii[1] < radii[2]
    assert all(GAP_BAND[0] < g < GAP_BAND[1] for g in gaps)
    assert o_closed and o_vol > 0 and abs(o_r - BALL_R) < 0.01
    assert psnr > PSNR_FLOOR
    # level-set mode of the main surface
    ls, lv = iso.extract_offsets_surfs_meshes(m, 96, nr_meshes_to_extract=3, delta_surfs=0.01, iter_nr=E2E["end"])
    assert len(ls) == 3 and all(x.faces.shape[0] > 100 for x in ls)
    # the K-shell stages take the shells as they are
    uvs = [compute_atlas(simplify_mesh(x, 0.1), 512, 4) for x in shells]
    vs = VolSurfs(uvs, using_neural_textures=True, max_rays=4096, textures_res=(256, 128, 64, 32),
                  nr_warmup_iters=2, lr=2e-3, bg_color=BG)
    vs.init_optim()
    vs.grad_scale = 1024.0
    idx, o, d, vals, _ = reel.get_next_rays_batch(1024)
    losses, _ = train_step(vs, o, d, vals["rgb"], None, iter_nr=0, is_first_iter=True, nr_rays=1024)
    assert np.isfinite(losses["loss"])
    print(f"offsets_surfs e2e total {time.time() - t0:.1f} s")
