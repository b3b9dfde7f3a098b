"""Held-out-view evaluation (volsurfs_amd.evaluation, csrc/image_metrics.hip): PSNR / SSIM against a float64
restatement of piq 0.8.0's definitions, the reference's CSV / PNG layout (evaluation.py:15-348), and
the trainer callback."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

# measured maxima on MI355X over every case of test_metrics_match_float64_restatement: |dpsnr| 2.7e-7 dB;
# |dssim| 8.2e-6 at 11x11 (one SSIM pixel: fp32 moments, the variance E[x^2] - E[x]^2 cancels and C2 = 9e-4 amplifies
# it), 3.2e-7 at 200x300 and below 1.3e-7 from 384x512 up, where the map's mean averages the rounding out
PSNR_TOL, SSIM_TOL = 1e-5, 1e-5     # psnr: 37x its measured maximum; ssim: the issue's bound, 1.2x the 11x11 maximum
IDENTICAL_PSNR = -10.0 * math.log10(1e-8)


# ---------------------------------------------------------------- float64 restatement (piq 0.8.0 + the 8-bit rule)
def ref_quantize(x):
    """numpy form of the 8-bit rule: trunc(clamp(x, 0, 1) * 255) computed in fp32."""
    x = np.asarray(x, dtype=np.float32)
    return (np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


def ref_values(img, quantize=False):
    """[H,W,3] float32 / uint8 -> [3,H,W] float64 of the values the metric sees (uint8: u8 / 255 in fp32)."""
    img = torch.as_tensor(img).cpu()
    if img.dtype == torch.uint8:
        v = img.float() / 255.0
    else:
        v = img.float()
        if quantize:
            v = torch.from_numpy(ref_quantize(v.numpy())).float() / 255.0
    return v.double().permute(2, 0, 1)


def ref_pool(H, W):
    return max(1, round(min(H, W) / 256))


def ref_psnr(x, y):
    return -10.0 * math.log10(float(((x - y) ** 2).mean()) + 1e-8)


def ref_ssim(x, y, downsample=True):
    """x, y: [3,H,W] float64."""
    f = ref_pool(x.shape[1], x.shape[2]) if downsample else 1
    x, y = x[None], y[None]
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    if x.shape[-1] < 11 or x.shape[-2] < 11:
        raise ValueError("too small")
    d = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(d[None] ** 2 + d[:, None] ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).expand(3, 1, 11, 11)
    conv = lambda t: F.conv2d(t, g, groups=3)  # noqa: E731
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx ** 2, conv(y * y) - my ** 2, conv(x * y) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    ss = (2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1) * cs
    return float(ss.mean())


# ---------------------------------------------------------------- CPU
def test_pool_factor_rounds_half_to_even():
    from volsurfs_amd.evaluation import pool_factor
    for side, f in ((384, 2), (640, 2), (800, 3), (1080, 4), (1200, 5), (200, 1), (11, 1), (2160, 8)):
        assert pool_factor(side, side + 500) == f == ref_pool(side, side + 500), side
    assert pool_factor(1920, 1080) == 4 and pool_factor(1600, 1200) == 5


def test_restatement_closed_form_constant_images():
    # constant a against constant b: every sigma is 0, cs = 1, ss = (2ab + C1) / (a^2 + b^2 + C1)
    a, b = 0.25, 0.75
    x = torch.full((3, 40, 30), a, dtype=torch.float64)
    y = torch.full((3, 40, 30), b, dtype=torch.float64)
    want = (2 * a * b + 1e-4) / (a * a + b * b + 1e-4)
    assert abs(ref_ssim(x, y) - want) < 1e-12
    assert abs(ref_psnr(x, y) - (-10 * math.log10(0.25 + 1e-8))) < 1e-12
    assert ref_ssim(x, x) == 1.0 and ref_psnr(x, x) == IDENTICAL_PSNR


def test_restatement_pools_before_filtering():
    # 2x2 checkerboard blocks of 0 / 1 at 512 x 512 (pool 2): pooled to a constant 0.5 -> ssim against 0.5 is 1
    i = torch.arange(512)
    board = ((i[:, None] + i[None]) % 2).double().expand(3, 512, 512)
    half = torch.full((3, 512, 512), 0.5, dtype=torch.float64)
    assert abs(ref_ssim(board, half) - 1.0) < 1e-12
    assert ref_ssim(board, half, downsample=False) < 0.1


def _csv_rows():
    from volsurfs_amd.evaluation import PerSceneEvaluator
    ev = PerSceneEvaluator("ray_traced")
    ev.update("000", 30.5, 0.9, float("nan"))
    ev.update("001", 20.25, 0.5, float("nan"))
    return ev


def test_per_scene_evaluator_csv_is_the_references_layout(tmp_path):
    ev = _csv_rows()
    assert ev.psnr_avg() == 25.375 and ev.ssim_avg() == 0.7 and math.isnan(ev.lpips_avg())
    assert set(ev.results_averaged()) == {"psnr", "ssim", "lpips"}
    rows = ev.save_to_csv(str(tmp_path))
    assert rows[-1][0] == "avg" and len(rows) == 3
    # csv.writer: no header row, floats by repr, \r\n line ends
    want = "000,30.5,0.9,nan\r\n001,20.25,0.5,nan\r\navg,25.375,0.7,nan\r\n"
    with open(tmp_path / "ray_traced.csv", "rb") as f:
        assert f.read() == want.encode()
    ev.save_to_csv(str(tmp_path), override_filename="test")
    with open(tmp_path / "test.csv", "rb") as f:
        assert f.read() == want.encode()


def test_argument_validation_before_device_work():
    from volsurfs_amd import evaluation as E
    a = torch.zeros(32, 32, 3)
    with pytest.raises(ValueError, match="shapes differ"):
        E.image_metrics(a, torch.zeros(32, 31, 3))
    with pytest.raises(ValueError, match="RGB"):
        E.image_metrics(torch.zeros(32, 32, 4), torch.zeros(32, 32, 4))
    with pytest.raises(ValueError, match="11x11"):
        E.image_metrics(torch.zeros(10, 40, 3), torch.zeros(10, 40, 3))
    with pytest.raises(ValueError, match="float32 or uint8"):
        E.image_metrics(a.double(), a.double())
    with pytest.raises(ValueError, match="same GPU"):                 # a valid pair on the CPU: no host fallback
        E.image_metrics(a, a)
    x = torch.zeros(1, 3, 32, 32)
    for kw in ({"kernel_size": 7}, {"kernel_sigma": 2.0}, {"k1": 0.02}, {"k2": 0.05}, {"full": True}):
        with pytest.raises(ValueError, match="not supported|defaults"):
            E.ssim(x, x, **kw)
    with pytest.raises(ValueError, match="data_range"):
        E.ssim(x, x, data_range=255)
    with pytest.raises(ValueError, match="data_range"):
        E.psnr(x.to(torch.uint8), x.to(torch.uint8), data_range=1.0)
    with pytest.raises(ValueError, match="reduction"):
        E.psnr(x, x, reduction="max")
    with pytest.raises(ValueError, match="N,3,H,W"):
        E.psnr(x[:, :2], x[:, :2])
    with pytest.raises(ValueError, match="every"):
        E.EvalCallback({}, 0, method=None)


# ---------------------------------------------------------------- GPU
def _smooth_noise(B, H, W, seed, noise=0.05):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B, 3, max(H // 16, 2), max(W // 16, 2), generator=g)
    smooth = F.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)
    return (smooth + noise * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1).permute(0, 2, 3, 1).contiguous()


def _random(B, H, W, seed):
    return torch.rand(B, H, W, 3, generator=torch.Generator().manual_seed(seed))


def _check_against_ref(pred, gt, quantize, maxima):
    from volsurfs_amd.evaluation import image_metrics
    res = image_metrics(pred.cuda(), gt.cuda(), quantize=quantize)
    p, s = res["psnr"].cpu(), res["ssim"].cpu()
    assert p.dtype == torch.float64 and s.dtype == torch.float64
    for b in range(pred.shape[0]):
        x, y = ref_values(pred[b], quantize), ref_values(gt[b])
        dp, ds = abs(float(p[b]) - ref_psnr(x, y)), abs(float(s[b]) - ref_ssim(x, y))
        maxima[0], maxima[1] = max(maxima[0], dp), max(maxima[1], ds)
        assert dp <= PSNR_TOL and ds <= SSIM_TOL, (tuple(pred.shape), b, dp, ds)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,B", [(11, 11, 2), (200, 300, 3), (384, 512, 2), (640, 480, 2), (801, 803, 3),
                                   (1080, 1920, 2), (1200, 1600, 4)])
def test_metrics_match_float64_restatement(H, W, B):
    maxima = [0.0, 0.0]
    gt = _smooth_noise(B, H, W, seed=H + W)
    preds = {"random": _random(B, H, W, seed=H * W),
             "smooth": _smooth_noise(B, H, W, seed=H + W + 1, noise=0.08),
             "perturbed": (gt + 0.02 * torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(7))).clamp(0, 1)}
    for kind, pred in preds.items():
        _check_against_ref(pred, torch.from_numpy(ref_quantize(gt.numpy())), True, maxima)    # fp32 + uint8
        _check_against_ref(torch.from_numpy(ref_quantize(pred.numpy())), torch.from_numpy(ref_quantize(gt.numpy())),
                           False, maxima)                                                     # uint8 + uint8
        _check_against_ref(pred, gt, False, maxima)                                           # fp32 + fp32, raw
    print(f"{H}x{W}: max |dpsnr| = {maxima[0]:.2e} dB, max |dssim| = {maxima[1]:.2e}")


def _method(seed=0, K=2):
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.methods import VolSurfs
    m = VolSurfs(nested_shells(K=K, subdiv=3), max_rays=4096, textures_res=(128, 64, 32, 16))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.bank.tables.copy_((torch.rand(m.bank.tables.shape, generator=g) * 2 - 1).cuda())
    m.bank.refresh_half_params()
    return m


def _cameras(n, size=64):
    from volsurfs_amd.camera import Camera
    return [Camera.look_at((1.5 * math.sin(0.7 * i), 0.3, -1.5 * math.cos(0.7 * i)), focal=1.6 * size,
                           height=size, width=size) for i in range(n)]


@pytest.mark.gpu
def test_metrics_on_a_render_against_a_perturbed_copy():
    m = _method()
    cam = _cameras(1, 256)[0]
    img = m.render_camera(cam)["rgb"].float().cpu()
    pert = (img + 0.03 * torch.randn(img.shape, generator=torch.Generator().manual_seed(3))).clamp(0, 1)
    maxima = [0.0, 0.0]
    _check_against_ref(pert[None], torch.from_numpy(ref_quantize(img.numpy()))[None], True, maxima)
    _check_against_ref(torch.from_numpy(ref_quantize(pert.numpy()))[None],
                       torch.from_numpy(ref_quantize(img.numpy()))[None], False, maxima)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(11, 11), (801, 803), (800, 800)])
def test_identical_images_score_exactly(H, W):
    from volsurfs_amd.evaluation import image_metrics
    x = _smooth_noise(3, H, W, seed=1).cuda()
    for a, b, q in ((x, x, False), (ref_quantize(x.cpu().numpy()), ref_quantize(x.cpu().numpy()), False), (x, x, True)):
        a, b = torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda()
        if q:
            b = torch.from_numpy(ref_quantize(x.cpu().numpy())).cuda()
        r = image_metrics(a, b, quantize=q)
        assert r["ssim"].tolist() == [1.0] * 3 and r["psnr"].tolist() == [IDENTICAL_PSNR] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(801, 803), (800, 800), (37, 45)])
def test_deterministic_and_batch_invariant(H, W):
    from volsurfs_amd.evaluation import image_metrics
    B = 4
    pred = _random(B, H, W, seed=5).cuda()
    gt = torch.from_numpy(ref_quantize(_smooth_noise(B, H, W, seed=6).numpy())).cuda()
    r1, r2 = image_metrics(pred, gt), image_metrics(pred, gt)
    for k in ("psnr", "ssim"):
        assert torch.equal(r1[k], r2[k])
        single = torch.cat([image_metrics(pred[b], gt[b])[k] for b in range(B)])
        assert torch.equal(r1[k], single), k      # odd sizes: images of the batch start at other alignments


@pytest.mark.gpu
def test_quantize_on_load_equals_quantize_u8():
    from volsurfs_amd.evaluation import image_metrics, quantize_u8
    pred = (_random(2, 384, 512, seed=9) * 1.4 - 0.2).cuda()        # values below 0 and above 1 too
    gt = torch.from_numpy(ref_quantize(_smooth_noise(2, 384, 512, seed=10).numpy())).cuda()
    a = image_metrics(pred, gt, quantize=True)
    b = image_metrics(quantize_u8(pred), gt)
    assert torch.equal(a["psnr"], b["psnr"]) and torch.equal(a["ssim"], b["ssim"])
    edges = torch.tensor([-1.0, -1e-7, 0.0, 1e-7, 1 / 255, 2 / 255, 0.5, 127 / 255, 254 / 255, 1 - 1e-7, 1.0, 1.0001,
                          7.0] + [k / 255 for k in range(256)], dtype=torch.float32)
    got = quantize_u8(edges.cuda()).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, ref_quantize(edges.numpy()))


@pytest.mark.gpu
def test_piq_call_shapes():
    from volsurfs_amd import evaluation as E
    pred = _smooth_noise(2, 96, 80, seed=11)
    gt = _smooth_noise(2, 96, 80, seed=12)
    x, y = pred.permute(0, 3, 1, 2).cuda(), gt.permute(0, 3, 1, 2).cuda()
    p = E.psnr(x, y, data_range=1.0, reduction="none").cpu()
    s = E.ssim(x, y, data_range=1.0, reduction="none").cpu()
    for b in range(2):
        xr, yr = ref_values(pred[b]), ref_values(gt[b])
        assert abs(float(p[b]) - ref_psnr(xr, yr)) <= PSNR_TOL and abs(float(s[b]) - ref_ssim(xr, yr)) <= SSIM_TOL
    assert torch.equal(E.psnr(x, y), p.cuda().mean()) and torch.equal(E.ssim(x, y, reduction="sum"), s.cuda().sum())
    big_x, big_y = _smooth_noise(1, 600, 600, seed=13), _smooth_noise(1, 600, 600, seed=14)
    s_nods = float(E.ssim(big_x.permute(0, 3, 1, 2).cuda(), big_y.permute(0, 3, 1, 2).cuda(), downsample=False))
    assert abs(s_nods - ref_ssim(ref_values(big_x[0]), ref_values(big_y[0]), downsample=False)) <= SSIM_TOL
    u8x, u8y = torch.from_numpy(ref_quantize(pred.numpy())), torch.from_numpy(ref_quantize(gt.numpy()))
    pu = E.psnr(u8x.permute(0, 3, 1, 2).cuda(), u8y.permute(0, 3, 1, 2).cuda(), data_range=255, reduction="none")
    assert abs(float(pu[0].cpu()) - ref_psnr(ref_values(u8x[0]), ref_values(u8y[0]))) <= PSNR_TOL


def _read_csv(path):
    import csv
    with open(path) as f:
        return list(csv.reader(f))


@pytest.mark.gpu
def test_render_and_eval_end_to_end(tmp_path):
    from volsurfs_amd.evaluation import eval_rendered_imgs, render_and_eval
    from volsurfs_amd.renderers import VolsurfsRenderer
    m = _method()
    cams = _cameras(3)
    gts = torch.stack([m.render_camera(c)["rgb"] for c in cams])                 # [3,H,W,3] f32 on the device
    splits = {"test": (cams, gts), "train": (cams[:2], gts[:2].cpu())}
    same = render_and_eval(m, splits, save_path=str(tmp_path), iter_nr=5)
    for split in splits:
        assert same[split]["psnr"] == IDENTICAL_PSNR and same[split]["ssim"] == 1.0
        assert math.isnan(same[split]["lpips"])
    root = tmp_path / "0000005" / "renders" / "test"
    assert sorted(os.listdir(root / "ray_traced" / "rgb")) == ["000.png", "001.png", "002.png"]
    assert sorted(os.listdir(root / "ray_traced" / "gt")) == ["000.png", "001.png", "002.png"]
    rows = _read_csv(root / "ray_traced.csv")
    assert [r[0] for r in rows] == ["000", "001", "002", "avg"]
    assert _read_csv(tmp_path / "results" / "test.csv") == rows
    assert len(_read_csv(tmp_path / "results" / "train.csv")) == 3

    # perturbed weights: both metrics drop; the PNGs written score the same bits offline
    with torch.no_grad():
        m.bank.tables.add_(0.3 * torch.randn(m.bank.tables.shape, generator=torch.Generator().manual_seed(1)).cuda())
    m.bank.refresh_half_params()
    worse = render_and_eval(m, {"test": (cams, gts)}, save_path=str(tmp_path), iter_nr=6, lpips_fn=lambda a, b: 0.5)
    assert worse["test"]["psnr"] < 60.0 and worse["test"]["ssim"] < 1.0 and worse["test"]["lpips"] == 0.5
    online = _read_csv(tmp_path / "0000006" / "renders" / "test" / "ray_traced.csv")
    [ev] = eval_rendered_imgs(str(tmp_path / "0000006" / "renders" / "test"))
    assert ev.render_mode == "ray_traced" and list(ev.imgs_results) == ["000", "001", "002"]
    for row in online[:3]:
        r = ev.imgs_results[row[0]]
        assert repr(r["psnr"]) == row[1] and repr(r["ssim"]) == row[2], row

    # the baked deploy renderer evaluates the same way (baked == live bit for bit)
    baked = render_and_eval(VolsurfsRenderer(m), {"test": (cams, gts)})
    assert baked["test"]["psnr"] == worse["test"]["psnr"] and baked["test"]["ssim"] == worse["test"]["ssim"]


@pytest.mark.gpu
def test_render_and_eval_keeps_the_feedback_buffer():
    from volsurfs_amd.camera import pinhole_rays
    from volsurfs_amd.evaluation import render_and_eval
    m = _method()
    o, d = pinhole_rays(32, 32, focal=50.0)
    m.render_rays(o, d, iter_nr=0)                        # a small "training" trace allocates the buffer
    fb = m.raytracer._fb
    assert fb is not None
    ptr, n = fb[0].data_ptr(), fb[1]
    cams = _cameras(2, 96)                                # 96 x 96 rays per view: more than the buffer holds
    assert 96 * 96 > n
    render_and_eval(m, {"test": (cams, torch.rand(2, 96, 96, 3))})
    assert m.raytracer._fb is fb and m.raytracer._fb[0].data_ptr() == ptr and m.raytracer._fb[1] == n


@pytest.mark.gpu
def test_eval_callback_in_trainer(tmp_path):
    from volsurfs_amd.camera import TensorReel
    from volsurfs_amd.evaluation import EvalCallback
    from volsurfs_amd.trainer import train
    target = _method(seed=0)
    cams = _cameras(6, 48)
    rgbs = torch.stack([target.render_camera(c)["rgb"] for c in cams]).float()
    reel = TensorReel(cams[:4], rgbs[:4])
    m = _method(seed=1)
    cb = EvalCallback({"test": (cams[4:], rgbs[4:])}, every=8, method=m, save_path=str(tmp_path), save_pngs=False)
    done = train(reel, m, iter_finish_nr=30, callbacks=[cb], nr_training_rays=2048)
    assert done == 30
    assert [it for it, _ in cb.history] == [7, 15, 23, 29]
    assert os.path.exists(tmp_path / "0000029" / "renders" / "test" / "ray_traced.csv")
    first, last = cb.history[0][1]["test"], cb.history[-1][1]["test"]
    assert last["psnr"] > first["psnr"], (first, last)
