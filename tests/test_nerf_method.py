"""The NeRF method (volsurfs_amd/nerf.py): hyper-parameters, the reference's render dict and losses, the occupancy
cadence, checkpoints, and training on a synthetic scene through meshing into the K-shell stages."""
import math
import time

import numpy as np
import pytest
import torch

# ---- CPU


def test_hyper_parameter_defaults_are_the_reference_nerf_config():
    """params/hyper_params.py + config/nerf/base.cfg (importance sampling raises min_nr_samples_per_ray to 3)."""
    from volsurfs_amd.nerf import NeRFHyperParams
    hp = NeRFHyperParams()
    want = {"lr": 1e-3, "nr_warmup_iters": 3000, "lr_milestones": [100000, 150000, 180000, 190000],
            "training_end_iter": 200000, "training_rays_batch_size": 512, "is_nr_training_rays_dynamic": True,
            "target_nr_of_training_samples": 512 * 96, "test_rays_batch_size": 16384, "is_training_masked": False,
            "is_testing_masked": False, "mask_weight": 0.0, "geom_feat_size": 32, "density_encoding_type": "permutohash",
            "density_mlp_layers_dims": [32, 32, 32], "rgb_pos_encoder_type": "permutohash",
            "rgb_dir_encoder_type": "spherical_harmonics", "rgb_mlp_layers_dims": [128, 128, 64], "sh_degree": 3,
            "appearance_predict_sh_coeffs": False, "rgb_view_dep": True, "rgb_normal_dep": False,
            "rgb_geom_feat_dep": True, "use_occupancy_grid": True, "do_importance_sampling": True,
            "max_nr_samples_per_ray": 64, "max_nr_imp_samples_per_ray": 32, "nr_samples_bg": 64,
            "density_nr_iters_for_c2f": 1000, "rgb_nr_iters_for_c2f": 0, "sparsity_weight": 1e-4,
            "nr_training_rays_per_pixel": 1, "nr_test_rays_per_pixel": 1, "min_dist_between_samples": 1e-4,
            "min_nr_samples_per_ray": 3, "bg_pos_encoder_type": "permutohash",
            "bg_dir_encoder_type": "spherical_harmonics"}
    for k, v in want.items():
        assert getattr(hp, k) == v, k
    assert NeRFHyperParams(lr=5e-3, do_importance_sampling=False).min_nr_samples_per_ray == 1
    with pytest.raises(KeyError):
        NeRFHyperParams(not_a_key=1)


def test_random_points_inside_the_bounding_primitives():
    from volsurfs_amd.background import BoundingBox, BoundingSphere
    torch.manual_seed(0)
    p = BoundingBox(side=1.2).get_random_points_inside(20000, device="cpu")
    assert p.shape == (20000, 3) and float(p.abs().max()) <= 0.6 and float(p.abs().max()) > 0.59
    assert abs(float(p.mean())) < 0.01
    s = BoundingSphere(radius=0.5).get_random_points_inside(20000, device="cpu")
    r = s.norm(dim=1)
    assert s.shape == (20000, 3) and float(r.max()) <= 0.5 + 1e-6
    # uniform in the ball: P(r < R/2) = 1/8
    assert abs(float((r < 0.25).float().mean()) - 0.125) < 0.01


# ---- GPU: the method's contract

def _method(**kw):
    from volsurfs_amd.background import BoundingSphere
    from volsurfs_amd.nerf import NeRF, NeRFHyperParams
    hp = NeRFHyperParams(**{"nr_warmup_iters": 10, **kw.pop("hp", {})})
    return NeRF(True, hp, kw.pop("load", None), kw.pop("save", None), BoundingSphere(0.5),
                bg_color=kw.pop("bg_color", None), start_iter_nr=kw.pop("start_iter_nr", 0))


def _rays(n, seed=0):
    g = torch.Generator("cuda").manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(n, 3, device="cuda", generator=g), dim=1) * 1.5
    tgt = (torch.rand(n, 3, device="cuda", generator=g) - 0.5) * 0.4
    return o.contiguous(), torch.nn.functional.normalize(tgt - o, dim=1).contiguous()


@pytest.mark.gpu
def test_density_state_dict_keys_are_the_reference_names():
    from volsurfs_amd.models import Density
    m = Density(in_channels=3, mlp_layers_dims=[32, 32, 32], encoding_type="permutohash", geom_feat_size=32)
    sd = m.state_dict()
    assert list(sd.keys()) == ["pos_encoder.encoder.lattice_values", "pos_encoder.encoder.random_shift_per_level",
                               "mlp.layers.0.weight", "mlp.layers.0.bias", "mlp.layers.2.weight", "mlp.layers.2.bias",
                               "mlp.layers.4.weight", "mlp.layers.4.bias", "mlp.layers.6.weight", "mlp.layers.6.bias"]
    assert tuple(sd["mlp.layers.0.weight"].shape) == (32, 50) and tuple(sd["mlp.layers.6.weight"].shape) == (33, 32)
    d, f = m(torch.rand(100, 3, device="cuda") - 0.5)
    assert d.shape == (100, 1) and f.shape == (100, 32) and bool((d >= 0).all())


@pytest.mark.gpu
def test_render_rays_dict_matches_the_reference():
    for bg_color in (None, (0.2, 0.4, 0.6)):
        m = _method(bg_color=bg_color)
        N = 300
        o, d = _rays(N)
        res = m.render_rays(o, d, iter_nr=0)
        assert set(res) == {"renders", "samples_3d", "samples_grad"} and res["samples_grad"] is None
        v = res["renders"]["volumetric"]
        keys = {"rgb", "rgb_fg", "rgb_bg", "depth", "weights_sum", "bg_transmittance", "nr_samples"}
        assert keys <= set(v) and (("median_depth_bg" in v) == (bg_color is None))
        for k, c in (("rgb", 3), ("rgb_fg", 3), ("rgb_bg", 3), ("depth", 1), ("weights_sum", 1),
                     ("bg_transmittance", 1), ("nr_samples", 1)):
            assert tuple(v[k].shape) == (N, c), k
        assert v["nr_samples"].dtype == torch.int32
        S = int(v["nr_samples"].sum())
        assert res["samples_3d"].shape == (S, 3) and S > 0
        assert torch.allclose(v["rgb"], v["rgb_fg"] + v["bg_transmittance"] * v["rgb_bg"], atol=1e-6)
        assert torch.allclose(v["bg_transmittance"], 1 - v["weights_sum"])


@pytest.mark.gpu
def test_sparsity_term_starts_after_iteration_5000():
    m = _method(bg_color=(0.0, 0.0, 0.0))
    o, d = _rays(256, 1)
    gt = torch.rand(256, 3, device="cuda")
    m.update_occupancy_grid = lambda *a, **k: None
    l0, _, _ = m(o, d, gt, None, 5000, is_first_iter=True)
    l1, _, _ = m(o, d, gt, None, 5001)
    assert l0["sparsity"] == 0.0
    assert isinstance(l1["sparsity"], torch.Tensor) and float(l1["sparsity"].detach()) > 0.0
    assert float(l1["loss"].detach()) > float(l1["rgb"].detach())


@pytest.mark.gpu
def test_occupancy_update_cadence():
    """nerf.py:120-122, 414-421: at construction the regular update of iteration 0 then a full-grid pass with decay
    0; then every 50th training iteration 256*256*4 random ROI voxels with decay 0.8."""
    from volsurfs_amd import nerf as nerf_mod
    calls = []
    orig = nerf_mod.NeRF.update_occupancy_grid

    def spy(self, iter_nr, decay=0.8, random_voxels=True, jitter_samples=True):
        calls.append((iter_nr, decay, random_voxels, jitter_samples))
        return orig(self, iter_nr, decay, random_voxels, jitter_samples)
    nerf_mod.NeRF.update_occupancy_grid = spy
    try:
        m = _method(bg_color=(0.0, 0.0, 0.0))
        assert calls == [(0, 0.8, True, True), (0, 0.0, False, False)]
        assert m.occupancy_grid.get_nr_voxels_per_dim() == 256
        calls.clear()
        for it in range(101):
            m.is_training = True
            m.update_method_state(it)
        assert calls == [(0, 0.8, True, True), (50, 0.8, True, True), (100, 0.8, True, True)]
    finally:
        nerf_mod.NeRF.update_occupancy_grid = orig
    assert nerf_mod.NeRF.OCCUPANCY_RANDOM_VOXELS == 256 * 256 * 4 and nerf_mod.NeRF.OCCUPANCY_THRESH == 1e-4


@pytest.mark.gpu
def test_save_load_round_trip_gives_identical_renders(tmp_path):
    import os
    torch.manual_seed(0)
    m = _method(save=str(tmp_path))
    o, d = _rays(64, 2)
    gt = torch.rand(64, 3, device="cuda")
    from volsurfs_amd.trainer import train_step
    for it in range(3):
        train_step(m, o, d, gt, None, iter_nr=it, is_first_iter=it == 0)
    path = m.save(3)
    assert sorted(os.listdir(path)) == ["bg.pt", "density.pt", "fusedadam.pt", "grid_occupancy.pt", "grid_values.pt",
                                        "rgb.pt"]
    assert path == os.path.join(str(tmp_path), "0000003", "models")
    m.is_training = False
    ro, rd = _rays(500, 3)
    a = m.render_rays(ro, rd, iter_nr=3)["renders"]["volumetric"]
    torch.manual_seed(1)
    m2 = _method(load=str(tmp_path), start_iter_nr=3)
    # (construction ends with a fresh full-grid pass over the loaded density, as nerf.py:130-132 does; loading
    # again restores the saved grid too)
    m2.load(3)
    m2.is_training = False
    b = m2.render_rays(ro, rd, iter_nr=3)["renders"]["volumetric"]
    for k in ("rgb", "depth", "weights_sum", "rgb_bg"):
        assert torch.equal(a[k], b[k]), k


# ---- GPU: end to end on a synthetic scene

BALL_R, BALL_SIGMA, SPHERE_R = 0.3, 8.0, 0.5
BG = (0.0, 0.0, 0.0)


def _ball_colour(p):
    return 0.5 + 0.5 * torch.stack([p[..., 0], p[..., 1], -p[..., 2]], -1) / BALL_R


def _gt_images(cameras, nq=256):
    """Dense CPU quadrature of the emission-absorption integral through the ball (float64)."""
    from volsurfs_amd.camera import get_camera_rays
    imgs = []
    for cam in cameras:
        o, d, _ = get_camera_rays(cam)
        o, d = o.cpu().double(), d.cpu().double()
        b = (o * d).sum(1)
        c = (o * o).sum(1) - BALL_R ** 2
        disc = b * b - c
        hit = disc > 0
        sq = disc.clamp(min=0).sqrt()
        t0, t1 = -b - sq, -b + sq
        u = (torch.arange(nq, dtype=torch.float64) + 0.5) / nq
        t = t0[:, None] + (t1 - t0)[:, None] * u[None]
        dt = ((t1 - t0) / nq)[:, None]
        p = o[:, None] + t[..., None] * d[:, None]
        alpha = 1 - torch.exp(-BALL_SIGMA * dt)
        T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha[:, :-1]], 1), 1)
        w = (alpha * T) * hit[:, None]
        rgb = (w[..., None] * _ball_colour(p)).sum(1) + (1 - w.sum(1, keepdim=True)) * torch.tensor(BG, dtype=torch.float64)
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


# measured on MI355X, three runs: 2000 iterations in 21.5-23.7 s, held-out PSNR 23.02-23.90 dB, the
# density-0.5 mesh closed with a mean vertex radius of 0.2932-0.2972 (error at most 0.0068) and a volume of 0.112
# (ball 0.113); the floor leaves 2 dB, the tolerance 3x; the whole test takes about 25 s
E2E_ITERS = 2000
PSNR_FLOOR = 21.0
RADIUS_TOL = 0.02


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
    m = _method(bg_color=BG, hp={"lr": 3e-3, "nr_warmup_iters": 100, "density_nr_iters_for_c2f": 500})
    t_train = time.time()
    done = train(reel, m, 0, E2E_ITERS, nr_training_rays=512,
                 target_nr_of_training_samples=m.hyper_params.target_nr_of_training_samples)
    torch.cuda.synchronize()
    t_train = time.time() - t_train
    assert done == E2E_ITERS
    res = render_and_eval(m, {"test": (test_cams, gt_test)}, save_pngs=False)
    psnr = res["test"]["psnr"]
    meshes, levels = iso.extract_nerf_level_sets(m, 128, nr_meshes=1, iter_nr=E2E_ITERS)
    mesh = meshes[0]
    V, F = mesh.vertices, mesh.faces.long()
    # closed: every undirected edge is shared by exactly two faces
    e = torch.cat([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]).sort(1).values
    _, cnt = torch.unique(e, dim=0, return_counts=True)
    closed = bool((cnt == 2).all())
    # outward winding: positive signed volume
    vol = float((V[F[:, 0]] * torch.linalg.cross(V[F[:, 1]], V[F[:, 2]])).sum() / 6)
    mean_r = float(V.norm(dim=1).mean())
    print(f"nerf e2e: {E2E_ITERS} iterations in {t_train:.1f} s ({E2E_ITERS / t_train:.0f} it/s), held-out PSNR "
          f"{psnr:.2f} dB, mesh V={V.shape[0]} F={F.shape[0]} closed={closed} volume={vol:.4f} "
          f"(ball {4 / 3 * math.pi * BALL_R ** 3:.4f}) mean radius {mean_r:.4f} (ball {BALL_R})")
    assert psnr > PSNR_FLOOR
    assert F.shape[0] > 100 and closed and vol > 0
    assert abs(mean_r - BALL_R) < RADIUS_TOL
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
    print(f"nerf e2e total {time.time() - t_start:.1f} s")
