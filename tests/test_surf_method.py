"""The Surf method (volsurfs_amd/surf.py): hyper-parameters, the schedule helpers, the NeuS / field-derivative
restatements against the reference's own functions (fixture), the render dict and losses, the occupancy cadence,
the phase switch, checkpoints, and training on a synthetic scene through meshing into the K-shell stages."""
import math
import os
import time

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "surf_neus.npz")

# ---- CPU


def test_hyper_parameter_defaults_are_the_reference_surf_config():
    """params/hyper_params.py (HyperParams, HyperParamsSuRF) + config/surf/base.cfg (importance sampling raises
    min_nr_samples_per_ray to 3)."""
    from volsurfs_amd.surf import SurfHyperParams
    hp = SurfHyperParams()
    want = {"lr": 1e-3, "nr_warmup_iters": 3000, "lr_milestones": [80000, 90000], "training_end_iter": 100000,
            "init_phase_end_iter": 5000, "first_phase_end_iter": 100000, "first_phase_variance_start_value": 0.3,
            "first_phase_variance_end_value": 0.7, "reduce_curv_start_iter": None, "reduce_curv_end_iter": None,
            "training_rays_batch_size": 512, "is_nr_training_rays_dynamic": True,
            "target_nr_of_training_samples": 512 * 96, "test_rays_batch_size": 16384, "is_training_masked": False,
            "is_testing_masked": False, "mask_weight": 0.0, "geom_feat_size": 32, "sdf_encoding_type": "permutohash",
            "sdf_mlp_layers_dims": [32, 32, 32], "sdf_nr_iters_for_c2f": 5000, "rgb_pos_encoder_type": "permutohash",
            "rgb_dir_encoder_type": "spherical_harmonics", "rgb_mlp_layers_dims": [128, 128, 64], "sh_degree": 3,
            "appearance_predict_sh_coeffs": True, "rgb_view_dep": True, "rgb_normal_dep": True,
            "rgb_geom_feat_dep": True, "rgb_use_lipshitz_mlp": False, "rgb_nr_iters_for_c2f": 0,
            "use_occupancy_grid": True, "do_importance_sampling": True, "max_nr_samples_per_ray": 64,
            "max_nr_imp_samples_per_ray": 32, "nr_samples_bg": 64, "min_dist_between_samples": 1e-4,
            "min_nr_samples_per_ray": 3, "eikonal_weight": 0.04, "curvature_weight": 0.65, "lipshitz_weight": 0.0,
            "offsurface_weight": 1e-4, "nr_training_rays_per_pixel": 1, "nr_test_rays_per_pixel": 1,
            "bg_pos_encoder_type": "permutohash", "bg_dir_encoder_type": "spherical_harmonics",
            "bg_nr_iters_for_c2f": 0, "jitter_training_rays": True, "jitter_test_rays": False,
            "use_color_calibration": False}
    for k, v in want.items():
        assert getattr(hp, k) == v, k
    assert SurfHyperParams(do_importance_sampling=False).min_nr_samples_per_ray == 1
    with pytest.raises(KeyError):
        SurfHyperParams(not_a_key=1)
    for bad in ({"rgb_use_lipshitz_mlp": True}, {"lipshitz_weight": 0.1}):
        with pytest.raises(NotImplementedError):
            SurfHyperParams(**bad)


def test_schedule_helpers():
    from volsurfs_amd.surf import curvature_weight_schedule, get_logistic_beta_from_variance, map_range_val
    assert get_logistic_beta_from_variance(0.3) == float(np.exp(3.0))
    assert get_logistic_beta_from_variance(0.7) == float(np.exp(7.0))
    assert get_logistic_beta_from_variance(5.0) == 1e6 and get_logistic_beta_from_variance(-5.0) == 1e-6
    # surf.py:815-828 with base.cfg: cos_anneal_ratio 0 -> 1 and variance 0.3 -> 0.7 over [5000, 100000]
    assert map_range_val(5000, 5000, 100000, 0.0, 1.0) == 0.0
    assert map_range_val(52500, 5000, 100000, 0.3, 0.7) == pytest.approx(0.5)
    assert map_range_val(200000, 5000, 100000, 0.3, 0.7) == 0.7
    assert map_range_val(10, 5000, 5000, 0.3, 0.7) == 0.7     # an empty window gives the end value
    assert curvature_weight_schedule(123, None, None) == 1.0
    assert curvature_weight_schedule(150, 100, 200) == pytest.approx(0.5)
    assert curvature_weight_schedule(50, 100, 200) == 1.0 and curvature_weight_schedule(200, 100, 200) == 0.0


def _fixture_sdf(p):
    r = p.norm(dim=-1, keepdim=True)
    return r - 0.3 + 0.05 * torch.sin(5.0 * p[:, 0:1]) * torch.cos(3.0 * p[:, 1:2]), None


def test_neus_alpha_and_field_derivatives_match_the_reference_fixture():
    """tools/make_golden.py gen_surf ran the reference's compute_alphas_from_logistic_beta, eikonal_loss,
    get_field_gradients and get_sdf_curvature on CPU; the restatements in surf.py give the same bits."""
    from volsurfs_amd.surf import eikonal_loss, get_field_gradients, get_sdf_curvature, neus_alphas_torch
    d = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(d[k])
    for i in range(4):
        car, beta = (float(x) for x in d[f"neus_cfg_{i}"])
        a = neus_alphas_torch(t("neus_dirs"), t("neus_dt"), t("neus_sdf"), t("neus_grad"), car, beta)
        assert torch.equal(a, t(f"neus_alpha_{i}")), i
    pts = t("field_points")
    fg = get_field_gradients(_fixture_sdf, pts)
    assert torch.equal(fg, t("field_grad"))
    assert torch.equal(eikonal_loss(fg), t("eikonal"))
    curv = get_sdf_curvature(_fixture_sdf, pts, fg, t("curv_rand_dirs"))
    assert torch.equal(curv, t("curvature"))
    curv = get_sdf_curvature(_fixture_sdf, pts, fg, t("curv_rand_dirs"), eps=1e-2)
    assert torch.equal(curv, t("curvature_eps1e2"))
    assert float(curv.max()) > 10 * float(curv.min())       # the wide step measures a varying angle


# ---- GPU: the method's contract

def _method(**kw):
    from volsurfs_amd.background import BoundingSphere
    from volsurfs_amd.surf import Surf, SurfHyperParams
    hp = SurfHyperParams(**{"nr_warmup_iters": 10, "init_phase_end_iter": 100, "first_phase_end_iter": 1000,
                            **kw.pop("hp", {})})
    return Surf(True, hp, kw.pop("load", None), kw.pop("save", None), BoundingSphere(0.5),
                bg_color=kw.pop("bg_color", None), start_iter_nr=kw.pop("start_iter_nr", 0),
                init_sphere_radius=kw.pop("init_sphere_radius", 0.25))


def _rays(n, seed=0):
    g = torch.Generator("cuda").manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(n, 3, device="cuda", generator=g), dim=1) * 1.5
    tgt = (torch.rand(n, 3, device="cuda", generator=g) - 0.5) * 0.4
    return o.contiguous(), torch.nn.functional.normalize(tgt - o, dim=1).contiguous()


@pytest.mark.gpu
def test_sdf_state_dict_keys_are_the_reference_names():
    from volsurfs_amd.models import SDF
    m = SDF(in_channels=3, mlp_layers_dims=[32, 32, 32], encoding_type="permutohash", geom_feat_size=32)
    sd = m.state_dict()
    assert list(sd.keys()) == ["pos_encoder.encoder.lattice_values", "pos_encoder.encoder.random_shift_per_level",
                               "mlp_sdf.layers.0.weight", "mlp_sdf.layers.0.bias", "mlp_sdf.layers.2.weight",
                               "mlp_sdf.layers.2.bias", "mlp_sdf.layers.4.weight", "mlp_sdf.layers.4.bias",
                               "mlp_sdf.layers.6.weight", "mlp_sdf.layers.6.bias"]
    assert tuple(sd["mlp_sdf.layers.0.weight"].shape) == (32, 50)
    assert tuple(sd["mlp_sdf.layers.6.weight"].shape) == (33, 32)
    p = torch.rand(100, 3, device="cuda") - 0.5
    s, f = m(p)
    assert s.shape == (100, 1) and f.shape == (100, 32) and bool((s < 0).any() or (s > 0).any())
    s2, f2 = m.main_sdf(p)
    assert torch.equal(s, s2) and torch.equal(f, f2)


@pytest.mark.gpu
def test_render_rays_dict_matches_the_reference():
    for bg_color in (None, (0.2, 0.4, 0.6)):
        # (no occupancy grid: the untrained field occupies no voxel of it)
        m = _method(bg_color=bg_color, hp={"use_occupancy_grid": False})
        N = 300
        o, d = _rays(N)
        res = m.render_rays(o, d, iter_nr=200, override={"variance": 0.5, "cos_anneal_ratio": 0.3})
        assert set(res) == {"renders", "samples_3d", "samples_grad"}
        v = res["renders"]["volumetric"]
        assert set(v) == {"rgb_fg", "depth_fg", "weights_sum", "bg_transmittance", "normals", "nr_samples", "rgb_bg",
                          "rgb", "depth_bg", "depth"}
        for k, c in (("rgb", 3), ("rgb_fg", 3), ("rgb_bg", 3), ("depth", 1), ("depth_fg", 1), ("depth_bg", 1),
                     ("weights_sum", 1), ("bg_transmittance", 1), ("normals", 3), ("nr_samples", 1)):
            assert tuple(v[k].shape) == (N, c), k
        assert v["nr_samples"].dtype == torch.int32
        S = int(v["nr_samples"].sum())
        assert S > 0 and res["samples_3d"].shape == (S, 3) and res["samples_grad"].shape == (S, 3)
        assert torch.allclose(v["rgb"], v["rgb_fg"] + v["bg_transmittance"] * v["rgb_bg"], atol=1e-6)
        assert torch.allclose(v["bg_transmittance"], 1 - v["weights_sum"])
        assert torch.allclose(v["depth"], v["depth_fg"] * v["weights_sum"] + v["depth_bg"] * v["bg_transmittance"])
        # the override reaches the composite: a different variance gives a different render
        v2 = m.render_rays(o, d, iter_nr=200, override={"variance": 0.9, "cos_anneal_ratio": 0.3})
        assert not torch.equal(v2["renders"]["volumetric"]["weights_sum"], v["weights_sum"])


@pytest.mark.gpu
def test_occupancy_update_cadence_and_sdf_rule():
    """surf.py:175-176, 246-302, 802-831: at construction the update of iteration 0 and a second one; then every
    50th training iteration and once more when the first phase starts; always the full grid, |sdf|, decay 0 and the
    beta of min(0.8, variance)."""
    from volsurfs_amd import surf as surf_mod
    calls = []
    orig = surf_mod.Surf.update_occupancy_grid

    def spy(self, iter_nr=None, decay=0.0):
        calls.append((iter_nr, decay))
        return orig(self, iter_nr, decay)
    surf_mod.Surf.update_occupancy_grid = spy
    try:
        m = _method(bg_color=(0.0, 0.0, 0.0))
        assert calls == [(0, 0.0), (0, 0.0)]
        calls.clear()
        for it in range(151):
            m.update_method_state(it)
        assert calls == [(0, 0.0), (50, 0.0), (100, 0.0), (100, 0.0), (150, 0.0)]
    finally:
        surf_mod.Surf.update_occupancy_grid = orig
    g = m.occupancy_grid
    assert g.get_nr_voxels_per_dim() == 256
    pts, idx = g.get_grid_samples(False)
    sdf = m.models["sdf"].main_sdf(pts[:4096], iter_nr=150)[0].abs().detach()
    assert torch.equal(g.get_grid_values().view(-1)[idx[:4096].long()], sdf.view(-1))
    # the SDF occupancy rule with beta = exp(10 min(0.8, variance)): a lower variance (wider band) never occupies
    # fewer voxels
    n_now = g.get_nr_occupied_voxels()
    m.variance = 0.2
    m.update_occupancy_grid(150)
    assert g.get_nr_occupied_voxels() >= n_now and surf_mod.Surf.OCCUPANCY_THRESH == 1e-4


@pytest.mark.gpu
def test_sphere_init_phase_then_first_phase():
    m = _method(bg_color=(0.0, 0.0, 0.0), hp={"init_phase_end_iter": 3, "use_occupancy_grid": False})
    rendered = []
    orig = m.render_rays
    m.render_rays = lambda *a, **k: rendered.append(1) or orig(*a, **k)
    o, d = _rays(256, 1)
    gt = torch.rand(256, 3, device="cuda")
    from volsurfs_amd.trainer import train_step
    nr = 256
    for it in range(3):
        losses, nr = train_step(m, o, d, gt, None, iter_nr=it, is_first_iter=it == 0, nr_rays=nr,
                                target_nr_of_training_samples=m.hyper_params.target_nr_of_training_samples)
        assert rendered == [] and m.lr_scheduler is None and m.last_nr_samples == 0
        assert losses["sdf"] > 0.0 and losses["rgb"] == 0.0 and nr == 256
    assert m.in_process_of_sphere_init
    losses, nr = train_step(m, o, d, gt, None, iter_nr=3, nr_rays=nr,
                            target_nr_of_training_samples=m.hyper_params.target_nr_of_training_samples)
    assert rendered == [1] and m.lr_scheduler is not None and not m.in_process_of_sphere_init
    assert m.cos_anneal_ratio == 0.0 and m.variance == m.hyper_params.first_phase_variance_start_value
    assert losses["rgb"] > 0.0 and losses["eikonal"] > 0.0 and losses["curvature"] > 0.0 and m.last_nr_samples > 0
    assert set(losses) == {"loss", "sdf", "eikonal", "rgb", "curvature", "lipshitz", "offsurface_high_sdf", "mask"}


@pytest.mark.gpu
def test_missing_init_sphere_radius_raises():
    with pytest.raises(ValueError):
        _method(init_sphere_radius=None)


@pytest.mark.gpu
def test_save_load_round_trip_and_a_reference_sdf_checkpoint(tmp_path):
    torch.manual_seed(0)
    m = _method(save=str(tmp_path), hp={"init_phase_end_iter": 1, "use_occupancy_grid": False})
    o, d = _rays(64, 2)
    gt = torch.rand(64, 3, device="cuda")
    from volsurfs_amd.trainer import train_step
    for it in range(3):
        train_step(m, o, d, gt, None, iter_nr=it, is_first_iter=it == 0)
    path = m.save(3)
    assert sorted(os.listdir(path)) == ["bg.pt", "fusedadam.pt", "rgb.pt", "sdf.pt"]
    assert path == os.path.join(str(tmp_path), "0000003", "models")
    m.is_training = False
    ro, rd = _rays(500, 3)
    a = m.render_rays(ro, rd, iter_nr=3)["renders"]["volumetric"]
    torch.manual_seed(1)
    m2 = _method(load=str(tmp_path), start_iter_nr=3, hp={"init_phase_end_iter": 1, "use_occupancy_grid": False},
                 init_sphere_radius=None)
    m2.load(3)
    m2.is_training = False
    m2.variance, m2.cos_anneal_ratio = m.variance, m.cos_anneal_ratio
    b = m2.render_rays(ro, rd, iter_nr=3)["renders"]["volumetric"]
    for k in ("rgb", "depth", "weights_sum", "normals", "rgb_bg"):
        assert torch.equal(a[k], b[k]), k
    # a lone sdf.pt in the reference's layout (what offsets_surfs loads) restores the field
    ref_root = tmp_path / "ref"
    os.makedirs(ref_root / "0010000" / "models")
    sd = {k: v.clone() for k, v in m.models["sdf"].state_dict().items()}
    torch.save(sd, ref_root / "0010000" / "models" / "sdf.pt")
    m3 = _method(load=str(ref_root), start_iter_nr=10000, init_sphere_radius=None)
    for k, v in m3.models["sdf"].state_dict().items():
        assert torch.equal(v, sd[k]), k


# ---- GPU: end to end on a synthetic scene

BALL_R, INIT_R = 0.3, 0.2
BG = (0.0, 0.0, 0.0)


def _ball_colour(p):
    return 0.5 + 0.5 * torch.stack([p[..., 0], p[..., 1], -p[..., 2]], -1) / BALL_R


def _gt_images(cameras):
    """An opaque ball by ray-sphere intersection: its colour at the first hit, else the background (float64)."""
    from volsurfs_amd.camera import get_camera_rays
    imgs = []
    for cam in cameras:
        o, d, _ = get_camera_rays(cam)
        o, d = o.cpu().double(), d.cpu().double()
        b = (o * d).sum(1)
        disc = b * b - ((o * o).sum(1) - BALL_R ** 2)
        hit = disc > 0
        t0 = -b - disc.clamp(min=0).sqrt()
        rgb = torch.where(hit[:, None], _ball_colour(o + t0[:, None] * d), torch.tensor(BG, dtype=torch.float64))
        imgs.append(rgb.float().reshape(cam.height, cam.width, 3))
    return torch.stack(imgs)


def _cameras(n, H=64, seed=0, device="cuda"):
    from volsurfs_amd.camera import Camera
    cams, golden = [], math.pi * (3 - math.sqrt(5))
    for i in range(n):
        y = 1 - 2 * (i + 0.5) / n
        r = math.sqrt(1 - y * y)
        th = golden * i + seed
        eye = (1.5 * r * math.cos(th), 1.5 * y, 1.5 * r * math.sin(th))
        cams.append(Camera.look_at(eye, focal=70.0, height=H, width=H, device=device))
    return cams


def _closed_volume_radius(mesh):
    V, F = mesh.vertices, mesh.faces.long()
    e = torch.cat([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]).sort(1).values
    _, cnt = torch.unique(e, dim=0, return_counts=True)
    vol = float((V[F[:, 0]] * torch.linalg.cross(V[F[:, 1]], V[F[:, 2]])).sum() / 6)
    return bool((cnt == 2).all()) and F.shape[0] > 100, vol, float(V.norm(dim=1).mean())


# measured on MI355X: this schedule (sphere init and data phase as two train() calls) in 21.1 s, held-out
# PSNR 30.48 dB, the zero-level mesh closed with a mean vertex radius of 0.2964 and a volume of 0.1090 (ball 0.1131);
# three runs of the same iterations as one train() call gave 31.6-32.9 dB and radii 0.2992-0.3001.  The floor
# leaves 2 dB below the lowest, the tolerance about 3x the largest error; the whole test takes about 22 s
E2E_INIT_ITERS, E2E_ITERS = 200, 1500
PSNR_FLOOR = 28.5
RADIUS_TOL = 0.01


@pytest.mark.gpu
def test_train_synthetic_ball_then_mesh_simplify_atlas_and_volsurfs(tmp_path):
    from volsurfs_amd import isosurface as iso
    from volsurfs_amd.atlas import compute_atlas
    from volsurfs_amd.camera import TensorReel
    from volsurfs_amd.evaluation import render_and_eval
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.simplify import simplify_mesh
    from volsurfs_amd.trainer import train, train_step
    torch.manual_seed(0)
    t_start = time.time()
    train_cams, test_cams = _cameras(24), _cameras(4, seed=0.5)
    gt_train, gt_test = _gt_images(train_cams), _gt_images(test_cams)
    reel = TensorReel(train_cams, gt_train)
    m = _method(bg_color=BG, init_sphere_radius=INIT_R,
                hp={"lr": 3e-3, "nr_warmup_iters": 100, "init_phase_end_iter": E2E_INIT_ITERS,
                    "first_phase_end_iter": E2E_ITERS, "sdf_nr_iters_for_c2f": 500})
    t_train = time.time()
    kw = {"nr_training_rays": 512, "target_nr_of_training_samples": m.hyper_params.target_nr_of_training_samples}
    assert train(reel, m, 0, E2E_INIT_ITERS, **kw) == E2E_INIT_ITERS
    init_mesh = iso.extract_surf_level_sets(m, 96, nr_meshes=1, iter_nr=E2E_INIT_ITERS)[0][0]
    assert train(reel, m, E2E_INIT_ITERS, E2E_ITERS, **kw) == E2E_ITERS
    torch.cuda.synchronize()
    t_train = time.time() - t_train
    res = render_and_eval(m, {"test": (test_cams, gt_test)}, save_pngs=False)
    psnr = res["test"]["psnr"]
    meshes, levels = iso.extract_surf_level_sets(m, 128, nr_meshes=1, iter_nr=E2E_ITERS)
    assert levels == [0.0]
    mesh = meshes[0]
    closed, vol, mean_r = _closed_volume_radius(mesh)
    shells, lv3 = iso.extract_surf_level_sets(m, 128, nr_meshes=3, delta_surfs=0.01, iter_nr=E2E_ITERS)
    shell_stats = [_closed_volume_radius(s) for s in shells]
    init_r = float(init_mesh.vertices.norm(dim=1).mean())
    print(f"surf e2e: {E2E_ITERS} iterations ({E2E_INIT_ITERS} sphere init) in {t_train:.1f} s "
          f"({E2E_ITERS / t_train:.0f} it/s), zero level mean radius {init_r:.4f} at init -> {mean_r:.4f} "
          f"(ball {BALL_R}), held-out PSNR {psnr:.2f} dB, mesh V={mesh.vertices.shape[0]} F={mesh.faces.shape[0]} "
          f"closed={closed} volume={vol:.4f} (ball {4 / 3 * math.pi * BALL_R ** 3:.4f}), shells {lv3}: "
          + ", ".join(f"r={r:.4f} closed={c} vol={v:.4f}" for c, v, r in shell_stats))
    assert abs(init_r - INIT_R) < 0.02            # training started from the other sphere
    assert psnr > PSNR_FLOOR
    assert closed and vol > 0
    assert abs(mean_r - BALL_R) < RADIUS_TOL
    assert all(c and v > 0 for c, v, _ in shell_stats)
    radii = [r for _, _, r in shell_stats]
    assert radii[0] < radii[1] < radii[2]
    # the K-shell stages take the mesh as it is
    simp = simplify_mesh(mesh, 0.1)
    uv = compute_atlas(simp, 512, 4)
    vs = VolSurfs([uv], using_neural_textures=True, max_rays=4096, textures_res=(256, 128, 64, 32),
                  nr_warmup_iters=2, lr=2e-3, bg_color=BG)
    vs.init_optim()
    vs.grad_scale = 1024.0
    idx, o, d, vals, _ = reel.get_next_rays_batch(1024)
    losses, _ = train_step(vs, o, d, vals["rgb"], None, iter_nr=0, is_first_iter=True, nr_rays=1024)
    assert np.isfinite(losses["loss"])
    print(f"surf e2e total {time.time() - t_start:.1f} s")
