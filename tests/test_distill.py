"""Teacher distillation: virtual cameras on a hemisphere drawn on the GPU (csrc/hemisphere_camera.h,
`vsa_hemisphere_cameras` / `vsa_virtual_rays_batch` / `vsa_distill_rays_batch`), `camera.VirtualCameras` /
`mixed_rays_batch`, and `trainer.train(teacher_method=...)` / `load_teacher`.

`sample_cameras_on_hemisphere` is mvdatasets' (an empty submodule of the reference checkout): parity is UNPINNED, the
rule is this library's own.  The CPU tests check the numpy restatement (tests/distill_restated.py) through geometry and
through the uniform law; the GPU tests pin the kernels to it bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

import distill_restated as D
from oracle import raygen as OR
from oracle.packed import Pcg32

AXES = [(a, s) for a in (0, 1, 2) for s in (1, -1)]
BANDS = [(0.0, 0.95), (0.3, 0.6)]
RADIUS = 1.3


def _up(axis, sign):
    up = np.zeros(3)
    up[axis] = sign
    return up


def _stream(advances):
    g = Pcg32()
    for _ in range(advances):
        g.advance()
    return g


# ------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("axis,sign", AXES)
def test_restated_cameras_sit_on_the_hemisphere_and_look_at_the_origin(axis, sign, band):
    from volsurfs_amd.camera import Camera
    up = _up(axis, sign)
    K = np.array([[40.0, 0.0, 16.0], [0.0, 41.5, 12.0], [0.0, 0.0, 1.0]])
    kinv = np.linalg.inv(K).astype(np.float32)
    worst = {"centre": 0.0, "orth": 0.0, "det": 0.0, "look_at": 0.0, "ray": 0.0}
    for call in range(3):
        stats = {}
        poses = D.hemisphere_cameras(_stream(call), 50, RADIUS, axis, sign, *band, stats=stats).astype(np.float64)
        # (a candidate passes the narrow band with probability 0.24: 1.3 % of its cameras fall back, inside the band too)
        assert stats["fallbacks"] == 0 or band != BANDS[0]
        for pose in poses:
            R, c = pose[:, :3], pose[:, 3]
            worst["centre"] = max(worst["centre"], abs(np.linalg.norm(c) / RADIUS - 1.0))
            h = float(c @ up) / RADIUS
            assert band[0] - 1e-6 <= h <= band[1] + 1e-6
            worst["orth"] = max(worst["orth"], np.abs(R.T @ R - np.eye(3)).max())
            worst["det"] = max(worst["det"], abs(np.linalg.det(R) - 1.0))
            assert np.abs(R[:, 2] + c / np.linalg.norm(c)).max() < 1e-6          # z points at the origin
            assert R[:, 1] @ up < 0.0                                              # world up is image-up (y is down)
            ref = Camera.look_at(tuple(c), up=tuple(up), device="cpu").c2w.double().numpy()
            worst["look_at"] = max(worst["look_at"], np.abs(ref - pose).max())
            o, d = OR.pinhole_ray(pose.astype(np.float32), kinv, K[0, 2], K[1, 2])
            o, d = o.astype(np.float64), d.astype(np.float64)
            worst["ray"] = max(worst["ray"], np.linalg.norm(o - (o @ d) * d / (d @ d)))
    print("worst:", worst)
    assert worst["centre"] < 1e-6 and worst["orth"] < 1e-6 and worst["det"] < 1e-6
    assert worst["look_at"] < 1e-6
    assert worst["ray"] < 1e-6 * RADIUS


def test_restated_cameras_are_uniform_over_the_band_and_never_fall_back():
    """200 successive calls x 100 cameras at [0, 0.95].  Uniform by area = uniform in height: mean 0.475, sigma of the
    mean 0.95 / sqrt(12 n) = 0.0019 at n = 20 000; a quadrant's share has sigma sqrt(0.25 * 0.75 / n) = 0.0031.  Both
    bounds are more than five sigma."""
    g = Pcg32()
    heights, azimuth, fallbacks, most = [], [], 0, 0
    for _ in range(200):
        stats = {}
        c = D.hemisphere_cameras(g, 100, RADIUS, 2, 1, 0.0, 0.95, stats=stats)[:, :, 3]
        g.advance()
        heights.append(c[:, 2] / RADIUS)
        azimuth.append(np.arctan2(c[:, 1], c[:, 0]))
        fallbacks, most = fallbacks + stats["fallbacks"], max(most, stats["max_attempts"])
    heights, azimuth = np.concatenate(heights).astype(np.float64), np.concatenate(azimuth)
    quadrants = np.bincount(np.floor((azimuth + np.pi) / (np.pi / 2)).astype(int).clip(0, 3), minlength=4) / 20000.0
    print("mean height %.4f, quadrants %s, most candidates tried %d of %d" % (heights.mean(), quadrants, most, D.ATTEMPTS))
    assert fallbacks == 0
    assert abs(heights.mean() - 0.475) < 0.01
    assert np.abs(quadrants - 0.25).max() < 0.02


@pytest.mark.parametrize("axis,sign", [(2, 1), (0, -1)])
def test_restated_fallback_is_mid_height_at_azimuth_zero(axis, sign):
    lo, hi = 0.2, 0.7
    want = np.zeros(3)
    hm = 0.5 * (lo + hi)
    want[axis], want[(axis + 1) % 3] = sign * hm, math.sqrt(1.0 - hm * hm)
    info = {}
    pose = D.hemisphere_camera(Pcg32(), 7, RADIUS, axis, sign, lo, hi, attempts=0, info=info)
    assert info["fell_back"]
    assert np.abs(pose[:, 3] - RADIUS * want).max() < 1e-6
    # a band of one height, which no candidate's fp32 value hits: every attempt is refused (the host check allows it)
    D.check_args(RADIUS, axis, sign, 0.45, 0.45)
    pose = D.hemisphere_camera(Pcg32(), 7, RADIUS, axis, sign, 0.45, 0.45, info=info)
    assert info["fell_back"] and info["attempts"] == D.ATTEMPTS
    want[axis], want[(axis + 1) % 3] = sign * 0.45, math.sqrt(1.0 - 0.45 * 0.45)
    assert np.abs(pose[:, 3] - RADIUS * want).max() < 1e-6
    R = pose[:, :3].astype(np.float64)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6


def test_refused_arguments_raise():
    from volsurfs_amd import _lib
    from volsurfs_amd.camera import VirtualCameras, sample_cameras_on_hemisphere
    K = np.eye(3)
    bad = [dict(max_height=1.0), dict(min_height=-0.1), dict(min_height=0.7, max_height=0.6), dict(radius=0.0),
           dict(radius=float("nan")), dict(up_axis=3), dict(up_sign=0), dict(max_height=float("nan"))]
    for kw in bad:
        args = dict(radius=1.0, up_axis=2, up_sign=1, min_height=0.0, max_height=0.95)
        args.update(kw)
        with pytest.raises(ValueError):
            D.check_args(**args)
        with pytest.raises(ValueError):
            sample_cameras_on_hemisphere(K, 8, 8, nr_cameras=4, **args)
        with pytest.raises(ValueError):
            VirtualCameras(K, 8, 8, nr_cameras=4, **args)
    # the C-ABI's own checks, through the paths that return before any launch
    L = _lib.lib()
    null, u64, f = ctypes.c_void_p(0), ctypes.c_uint64(1), ctypes.c_float
    ERR_ARG = -1
    assert L.vsa_hemisphere_cameras(4, f(1.0), 2, 1, f(0.0), f(0.95), u64, u64, null, null) == ERR_ARG      # no output
    assert L.vsa_hemisphere_cameras(0, f(1.0), 2, 1, f(0.0), f(0.95), u64, u64, null, null) == 0            # no cameras
    assert L.vsa_hemisphere_cameras(-1, f(1.0), 2, 1, f(0.0), f(0.95), u64, u64, null, null) == ERR_ARG
    assert L.vsa_hemisphere_cameras(0, f(1.0), 2, 1, f(0.0), f(1.0), u64, u64, null, null) == ERR_ARG       # height 1
    assert L.vsa_hemisphere_cameras(0, f(1.0), 2, 1, f(-0.5), f(0.5), u64, u64, null, null) == ERR_ARG
    assert L.vsa_hemisphere_cameras(0, f(1.0), 2, 1, f(0.6), f(0.5), u64, u64, null, null) == ERR_ARG
    assert L.vsa_hemisphere_cameras(0, f(1.0), 3, 1, f(0.0), f(0.5), u64, u64, null, null) == ERR_ARG
    assert L.vsa_hemisphere_cameras(0, f(-1.0), 2, 1, f(0.0), f(0.5), u64, u64, null, null) == ERR_ARG
    assert L.vsa_virtual_rays_batch(null, 4, 8, 8, f(1.0), 2, 1, f(0.0), f(0.95), 16, 1, u64, u64, null, null, null,
                                    null, null) == ERR_ARG
    assert L.vsa_virtual_rays_batch(null, 4, 8, 8, f(1.0), 2, 1, f(0.0), f(0.95), 0, 1, u64, u64, null, null, null,
                                    null, null) == 0
    assert L.vsa_virtual_rays_batch(null, 4, 8, 8, f(1.0), 2, 1, f(0.0), f(0.95), -1, 1, u64, u64, null, null, null,
                                    null, null) == ERR_ARG
    reel = (null, null, null, null, 2, 8, 8)
    assert L.vsa_distill_rays_batch(null, 4, f(1.0), 2, 1, f(0.0), f(0.95), 8, 1, u64, u64, *reel, 8, 1, 1, u64, u64,
                                    null, null, null, null, null, null, null, null) == ERR_ARG
    assert L.vsa_distill_rays_batch(null, 4, f(1.0), 2, 1, f(0.0), f(0.95), 0, 1, u64, u64, *reel, 0, 1, 1, u64, u64,
                                    null, null, null, null, null, null, null, null) == 0
    assert L.vsa_distill_rays_batch(null, 4, f(1.0), 2, 1, f(0.0), f(0.95), -1, 1, u64, u64, *reel, 0, 1, 1, u64, u64,
                                    null, null, null, null, null, null, null, null) == ERR_ARG
    assert L.vsa_distill_rays_batch(null, 4, f(1.0), 2, 1, f(0.0), f(0.95), 0, 1, u64, u64, *reel, 4, 0, 1, u64, u64,
                                    null, null, null, null, null, null, null, null) == ERR_ARG             # R < 1


# ------------------------------------------------------------------------------------------------------------ GPU

def _skewed(seed=1):
    from test_raygen import _cam_np
    K, _, H, W = _cam_np(seed)
    return K, H, W


@pytest.mark.gpu
@pytest.mark.parametrize("advances", [0, 3])
@pytest.mark.parametrize("C", [1, 100, 257])
def test_hip_hemisphere_cameras_vs_restatement(C, advances):
    from volsurfs_amd import camera as Cm
    from volsurfs_amd.volsurfs import _Pcg32State
    for axis, sign in AXES:
        for band in BANDS:
            rng = _Pcg32State()
            for _ in range(advances):
                rng.advance()
            cams = Cm.sample_cameras_on_hemisphere(np.eye(3), 8, 8, RADIUS, C, axis, sign, *band, rng=rng)
            got = np.stack([c.c2w.cpu().numpy() for c in cams])
            assert np.array_equal(got, D.hemisphere_cameras(_stream(advances), C, RADIUS, axis, sign, *band))
            assert rng.state == _stream(advances + 1).state


@pytest.mark.gpu
@pytest.mark.parametrize("C,B,jitter", [(100, 700, True), (1, 1, True), (3, 257, False)])
def test_hip_virtual_rays_batch_vs_restatement(C, B, jitter):
    from volsurfs_amd import camera as Cm
    K, H, W = _skewed()
    vc = Cm.VirtualCameras(K, H, W, RADIUS, C, up_axis=1, up_sign=-1, min_height=0.1, max_height=0.9)
    kinv = vc.intrinsics_inv.cpu().numpy()
    before = vc.cameras()
    cam, o, d, p = vc.get_next_rays_batch(B, jitter)
    rc, ro, rd, rp = D.virtual_batch(Pcg32(), C, kinv, H, W, B, jitter, RADIUS, 1, -1, 0.1, 0.9)
    assert cam.dtype == torch.int32 and np.array_equal(cam.cpu().numpy(), rc)
    assert np.array_equal(o.cpu().numpy(), ro) and np.array_equal(d.cpu().numpy(), rd)
    assert np.array_equal(p.cpu().numpy(), rp)
    if C == 100:
        assert len(set(rc.tolist())) > 90
    # cameras() before the call: the poses the call's rays start from, and the rays get_camera_rays would make
    assert len(before) == C
    centres = torch.stack([c.c2w[:, 3] for c in before])
    assert torch.equal(o, centres[cam.long()])
    b0 = before[int(cam[0])]
    assert torch.equal(b0.intrinsics_inv, vc.intrinsics_inv)
    _, d0 = OR.pinhole_ray(b0.c2w.cpu().numpy(), kinv, *p[0].tolist())
    assert np.array_equal(d[0].cpu().numpy(), d0)
    # a second call is a new draw from new cameras
    cam2, o2, d2, _ = vc.get_next_rays_batch(B, jitter)
    assert not torch.equal(o, o2) and not torch.equal(d, d2)
    r2 = _stream(1)
    assert np.array_equal(o2.cpu().numpy(), D.virtual_batch(r2, C, kinv, H, W, B, jitter, RADIUS, 1, -1, 0.1, 0.9)[1])


def _reel(with_mask, seed=5):
    from test_raygen import _cam_np
    from volsurfs_amd import camera as Cm
    g = np.random.default_rng(seed)
    cams = []
    for s in range(5):
        K, pose, H, W = _cam_np(10 + s)
        cams.append(Cm.Camera(K, pose, H, W))
    rgbs = g.uniform(0, 1, (5, H, W, 3)).astype(np.float32)
    masks = (g.uniform(0, 1, (5, H, W)) > 0.5).astype(np.float32) if with_mask else None
    return Cm.TensorReel(cams, rgbs, masks), rgbs, masks, K, H, W


@pytest.mark.gpu
@pytest.mark.parametrize("n_v,n_r", [(350, 350), (1, 1), (0, 5), (5, 0)])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("with_mask", [True, False])
def test_hip_mixed_batch_equals_the_two_separate_calls(with_mask, R, n_v, n_r):
    from volsurfs_amd import camera as Cm
    reel_a, rgbs, masks, K, H, W = _reel(with_mask)
    reel_b = _reel(with_mask)[0]
    va, vb = (Cm.VirtualCameras(K, H, W, RADIUS, 100) for _ in range(2))
    for rng in (reel_a.rng, reel_b.rng, va.rng, vb.rng):       # not the streams' starts
        rng.advance()
    o, d, gt, mask, cam_v, cam_r = Cm.mixed_rays_batch(va, reel_a, n_v, n_r, True, R)
    cv, ov, dv, _ = vb.get_next_rays_batch(n_v, True)
    cr, orr, dr, vals, _ = reel_b.get_next_rays_batch(n_r, True, R)
    n = n_v + n_r * R
    assert o.shape == d.shape == gt.shape == (n, 3)
    assert torch.equal(cam_v, cv) and torch.equal(cam_r, cr)
    assert torch.equal(o, torch.cat([ov, orr])) and torch.equal(d, torch.cat([dv, dr]))
    assert torch.equal(gt[n_v:], vals["rgb"].repeat_interleave(R, 0))
    if with_mask:
        assert mask.shape == (n, 1)
        assert bool((mask[:n_v] == 1).all())
        assert torch.equal(mask[n_v:], vals["mask"].repeat_interleave(R, 0))
    else:
        assert mask is None
        m1 = Cm.mixed_rays_batch(va, reel_a, n_v, n_r, True, R, with_mask=True)[3]     # asked for: ones
        vb.get_next_rays_batch(n_v, True), reel_b.get_next_rays_batch(n_r, True, R)
        assert m1.shape == (n, 1) and bool((m1 == 1).all())
    # both streams stand where the separate calls leave them: the next separate calls agree
    assert (va.rng.state, reel_a.rng.state) == (vb.rng.state, reel_b.rng.state)
    for x, y in zip(va.get_next_rays_batch(64, True), vb.get_next_rays_batch(64, True)):
        assert torch.equal(x, y)
    xa, xb = reel_a.get_next_rays_batch(64, False, R), reel_b.get_next_rays_batch(64, False, R)
    assert torch.equal(xa[0], xb[0]) and torch.equal(xa[2], xb[2]) and torch.equal(xa[3]["rgb"], xb[3]["rgb"])


@pytest.mark.gpu
def test_hip_mixed_batch_vs_restatement():
    from volsurfs_amd import camera as Cm
    reel, rgbs, masks, K, H, W = _reel(True)
    vc = Cm.VirtualCameras(K, H, W, RADIUS, 7, up_axis=0, up_sign=1)
    o, d, gt, mask, cam_v, cam_r = Cm.mixed_rays_batch(vc, reel, 130, 131, False, 2)
    ro, rd, rgt, rmask, rcv, rcr = D.mixed_batch(Pcg32(), 7, vc.intrinsics_inv.cpu().numpy(), RADIUS, (0, 1, 0.0, 0.95),
                                                 130, reel.c2w.cpu().numpy(), reel.intrinsics_inv.cpu().numpy(), rgbs,
                                                 masks, 131, 2, False, Pcg32())
    assert np.array_equal(o.cpu().numpy(), ro) and np.array_equal(d.cpu().numpy(), rd)
    assert np.array_equal(gt[130:].cpu().numpy(), rgt[130:]) and np.array_equal(mask.cpu().numpy(), rmask)
    assert np.array_equal(cam_v.cpu().numpy(), rcv) and np.array_equal(cam_r.cpu().numpy(), rcr)


# ---- the trainer

class _StubTeacher:
    """Records how it is called; its colour is an analytic function of the ray direction."""

    def __init__(self):
        self.is_training, self.bg_color, self.calls = True, None, []

    def render(self, rays_o, rays_d, chunk=None):
        r = rays_o.norm(dim=1)
        self.calls.append({"n": rays_o.shape[0], "is_training": self.is_training, "chunk": chunk,
                           "bg": None if self.bg_color is None else self.bg_color.clone(),
                           "r_min": float(r.min()), "r_max": float(r.max()), "grad": torch.is_grad_enabled()})
        return {"rgb": 0.5 + 0.5 * rays_d}


def _student(**kw):
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.methods import VolSurfs
    torch.manual_seed(0)
    return VolSurfs(nested_shells(K=2, subdiv=2), max_rays=4096, textures_res=(64, 32, 16, 8), lr=1e-2,
                    nr_warmup_iters=0, **kw)


def _front_reel(H=32, W=32, colour=0.3, masks=None):
    from volsurfs_amd import camera as Cm
    cams = [Cm.Camera.look_at((0.0, 0.2, -1.5), focal=45.0, height=H, width=W)]
    return Cm.TensorReel(cams, torch.full((1, H, W, 3), colour, device="cuda"), masks)


@pytest.mark.gpu
def test_train_with_a_stub_teacher():
    from volsurfs_amd import _lib
    from volsurfs_amd.trainer import train
    m, reel, teacher = _student(bg_color=(0.9, 0.8, 0.7)), _front_reel(), _StubTeacher()
    log, fused = [], []
    inner = m.fused_forward_backward
    m.fused_forward_backward = lambda o, d, gt, **kw: (fused.append(o.shape[0]), inner(o, d, gt, **kw))[1]

    class Recorder:
        def training_started(self, **kw): log.append("start")
        def iter_started(self, phase, **kw): log.append(("it", phase.iter_nr, phase.is_first_iter))
        def iter_ended(self, phase, losses, **kw): log.append(("end", phase.iter_nr, losses["loss"]))
        def training_ended(self, **kw): log.append("stop")

    done = train(reel, m, start_iter_nr=5, iter_finish_nr=13, callbacks=[Recorder()], nr_training_rays=513,
                 teacher_method=teacher, teacher_nr_cameras=20, teacher_camera_radius=1.7, teacher_up=(1, -1))
    assert done == 13 and log[0] == "start" and log[-1] == "stop"
    its = [e for e in log if isinstance(e, tuple) and e[0] == "it"]
    assert [e[1] for e in its] == list(range(5, 13)) and its[0][2] and not its[1][2]
    ends = [e for e in log if isinstance(e, tuple) and e[0] == "end"]
    assert len(ends) == 8 and all(math.isfinite(e[2]) and e[2] > 0 for e in ends)
    assert len(teacher.calls) == 8                                  # once per iteration
    for c in teacher.calls:
        assert c["n"] == 513 // 2 and c["is_training"] is False and not c["grad"] and c["chunk"] is None
        assert torch.equal(c["bg"].reshape(3), m.bg_color.reshape(3))
        assert abs(c["r_min"] / 1.7 - 1) < 1e-6 and abs(c["r_max"] / 1.7 - 1) < 1e-6
    assert teacher.is_training is True                              # restored
    # a reel without masks, unmasked training: the fused path, on the whole mixed batch
    assert m.supports_fused_step(None, False) and fused == [2 * (513 // 2)] * 8
    with pytest.raises(_lib.VolsurfsHipError):
        train(reel, m, 0, 1, nr_training_rays=1, teacher_method=teacher)
    # the default radius: the reel's camera centres' mean distance from the origin
    teacher.calls.clear()
    train(reel, m, 0, 1, nr_training_rays=64, teacher_method=teacher, teacher_up=(1, -1))
    want = math.sqrt(0.2 ** 2 + 1.5 ** 2)
    assert abs(teacher.calls[0]["r_min"] / want - 1) < 1e-6 and abs(teacher.calls[0]["r_max"] / want - 1) < 1e-6


@pytest.mark.gpu
def test_train_with_a_stub_teacher_masked():
    """Masked training on a reel with masks: gt_mask = [ones | mask], the real half's colours under the mask rule."""
    from volsurfs_amd import trainer as T
    from volsurfs_amd.camera import VirtualCameras
    H = W = 32
    masks = torch.zeros(1, H, W, device="cuda")
    masks[:, :, W // 2:] = 1.0
    m, reel, teacher = _student(bg_color=(0.9, 0.8, 0.7)), _front_reel(H, W, 0.3, masks), _StubTeacher()
    m.init_optim()
    vc = VirtualCameras(reel.intrinsics[0], H, W, 1.5, 10, up_axis=1, up_sign=-1)
    seen = {}
    inner = T.train_step

    def spy(method, rays_o, rays_d, gt_rgb, gt_mask=None, *a, **kw):
        seen.update(o=rays_o, d=rays_d, gt=gt_rgb.clone(), mask=gt_mask.clone())
        return inner(method, rays_o, rays_d, gt_rgb, gt_mask, *a, **kw)
    T.train_step = spy
    try:
        losses, _ = T.train_step_distilled(m, vc, reel, teacher, 400, nr_rays_per_pixel=2, is_training_masked=True,
                                           is_first_iter=True)
    finally:
        T.train_step = inner
    assert math.isfinite(losses["loss"]) and losses["loss"] > 0
    n = 200
    assert seen["o"].shape == (n + 2 * n, 3) and seen["mask"].shape == (3 * n, 1)
    assert bool((seen["mask"][:n] == 1).all()) and 0 < float(seen["mask"][n:].mean()) < 1
    assert torch.equal(seen["gt"][:n], 0.5 + 0.5 * seen["d"][:n])
    bg = m.bg_color.reshape(1, 3)
    want = torch.where(seen["mask"][n:] > 0, torch.full((2 * n, 3), 0.3, device="cuda") * 1.0, bg.expand(2 * n, 3))
    assert torch.allclose(seen["gt"][n:], want, atol=1e-7)


@pytest.mark.gpu
def test_train_without_a_teacher_is_the_parent_path():
    """teacher_method=None: the loop of before.  Same batches (the reel's stream ends in the same state), the same
    first loss to the bit (no parameter has moved yet), and the later ones within what two eager runs of one loop
    differ by (the order of the gradient atomics: 5e-3, tests/test_train_graph.py)."""
    from volsurfs_amd.trainer import train, train_step_from_reel
    got = []

    class Rec:
        def iter_ended(self, phase, losses, **kw): got.append(losses["loss"])

    m, reel = _student(), _front_reel()
    train(reel, m, 0, 6, callbacks=[Rec()], nr_training_rays=512, teacher_method=None)
    m2, reel2 = _student(), _front_reel()
    m2.init_optim()
    want = [train_step_from_reel(m2, reel2, 512, iter_nr=i, is_first_iter=i == 0)[0]["loss"] for i in range(6)]
    assert reel.rng.state == reel2.rng.state
    assert got[0] == want[0]
    assert all(abs(a - b) < 5e-3 for a, b in zip(got, want)), (got, want)


@pytest.mark.gpu
def test_a_teacher_improves_a_view_no_photograph_covers():
    """One front camera of constant colour; the teacher returns the same constant everywhere.  After the same number
    of iterations from the same seeds, a held-out BACK view is closer to the constant with the teacher than without
    (both measured here; the teacher-less loop is the baseline)."""
    from volsurfs_amd import camera as Cm
    from volsurfs_amd.trainer import train

    class Constant(_StubTeacher):
        def render(self, rays_o, rays_d, chunk=None):
            return {"rgb": torch.full_like(rays_d, 0.3)}

    back = Cm.Camera.look_at((0.0, -0.3, 1.5), focal=45.0, height=32, width=32)
    err = {}
    for name, teacher in (("without", None), ("with", Constant())):
        m, reel = _student(), _front_reel()
        train(reel, m, 0, 60, nr_training_rays=1024, teacher_method=teacher, teacher_camera_radius=1.5,
              teacher_up=(1, -1))
        err[name] = float((m.render_camera(back)["rgb"].float() - 0.3).abs().mean())
    print("held-out back view, mean L1: without a teacher %.4f, with %.4f" % (err["without"], err["with"]))
    assert err["with"] < err["without"]


@pytest.mark.gpu
def test_load_teacher_round_trip_and_train(tmp_path):
    from volsurfs_amd import _lib
    from volsurfs_amd.background import BoundingSphere
    from volsurfs_amd.nerf import NeRF, NeRFHyperParams
    from volsurfs_amd.trainer import load_teacher, train, train_step
    torch.manual_seed(0)
    hp = NeRFHyperParams(nr_warmup_iters=10, test_rays_batch_size=300)
    saved = NeRF(True, hp, None, str(tmp_path / "ckpt"), BoundingSphere(0.5), bg_color=(1.0, 1.0, 1.0))
    g = torch.Generator("cuda").manual_seed(2)
    o = torch.nn.functional.normalize(torch.randn(500, 3, device="cuda", generator=g), dim=1) * 1.5
    d = torch.nn.functional.normalize(-o + 0.2 * torch.randn(500, 3, device="cuda", generator=g), dim=1)
    o, d = o.contiguous(), d.contiguous()
    gt = torch.rand(64, 3, device="cuda")
    for it in range(2):
        train_step(saved, o[:64], d[:64], gt, None, iter_nr=it, is_first_iter=it == 0)
    saved.save(1)                                                      # an older checkpoint: not the one taken
    train_step(saved, o[:64], d[:64], gt, None, iter_nr=2)
    saved.update_occupancy_grid(iter_nr=3, decay=0.0, random_voxels=False, jitter_samples=False)   # as a load rebuilds it
    saved.save(3)
    saved.is_training = False
    a = saved.render(o, d)
    with pytest.raises(_lib.VolsurfsHipError):
        load_teacher(str(tmp_path / "none"), hp, BoundingSphere(0.5))
    (tmp_path / "empty").mkdir()
    with pytest.raises(_lib.VolsurfsHipError):
        load_teacher(str(tmp_path / "empty"), hp, BoundingSphere(0.5))
    torch.manual_seed(1)
    teacher = load_teacher(str(tmp_path / "ckpt"), hp, BoundingSphere(0.5), bg_color=(1.0, 1.0, 1.0))
    assert teacher.is_training is False and teacher.optimizer is None
    b = teacher.render(o, d)
    for k in ("rgb", "depth", "weights_sum"):
        assert torch.equal(a[k], b[k]), k
    got = []

    class Rec:
        def iter_ended(self, phase, losses, **kw): got.append(losses["loss"])

    m, reel = _student(), _front_reel()
    train(reel, m, 0, 3, callbacks=[Rec()], nr_training_rays=512, teacher_method=teacher, teacher_up=(1, -1))
    assert len(got) == 3 and all(math.isfinite(v) and v > 0 for v in got)
    assert teacher.is_training is False
