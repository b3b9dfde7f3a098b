"""Texture export (`volsurfs_amd.texture_export`, csrc/texture_io.hip): the baker's `--extract_textures` — baked shell
textures as RGBA PNGs + scene.json in the reference's layout — and `load_scene`, which renders an exported scene again
through the baked-shading kernels."""
import json
import os
import time

import numpy as np
import pytest
import torch

SMALL = (64, 32, 16, 8)
FULL = (2048, 1024, 512, 256)
# measured on MI355X (tests/test_texture_export.py::test_full_size_round_trip); the bounds are twice that
FULL_EXPORT_S_MAX = 2.0       # measured 0.88 s
FULL_LOAD_S_MAX = 1.0         # measured 0.47 s
RENDER_KEYS = ("rgb", "surfs_rgb", "surfs_alpha", "surfs_normals")


# ---------------------------------------------------------------------------------------------------------------------
# helpers

def _cpu_camera(eye, fx, fy, cx, cy, W, H):
    from volsurfs_amd.camera import Camera
    pose = Camera.look_at(eye, focal=fx, height=H, width=W, device="cpu").c2w
    return Camera([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], pose, H, W, device="cpu")


def _randomize(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.bank.tables.copy_((torch.rand(m.bank.tables.shape, generator=g) * 2 - 1).cuda())
    m.bank.refresh_half_params()
    return m


def _method(meshes, res=SMALL, **kw):
    from volsurfs_amd.methods import VolSurfs
    return _randomize(VolSurfs(meshes, max_rays=4096, textures_res=res, **kw))


def _shells(K=2, subdiv=3):
    from volsurfs_amd.mesh import nested_shells
    return nested_shells(K=K, subdiv=subdiv)


def _atlas_shells(K=2, subdiv=3):
    """Shells through compute_atlas with its defaults (1024, padding 4): every chart at least one texel inside the
    border at 256."""
    from volsurfs_amd.atlas import compute_atlas
    return [compute_atlas(m) for m in _shells(K, subdiv)]


def _view(H=56, W=56, focal=90.0):
    from volsurfs_amd.camera import pinhole_rays
    return pinhole_rays(H, W, focal=focal)


def _assert_same_render(a, b):
    for k in RENDER_KEYS:
        assert torch.equal(a[k], b[k]), k


def _no_footprint_in_apron(m, o, d):
    """Every hit's bilinear footprint (nt_footprint, lerp) lies in the R x R interior at every degree."""
    _, hit_slot, hit_uv = m.raytracer.trace_all(o.contiguous(), d.contiguous())
    tex_uv = m.baked.tex_uv_only(hit_slot, hit_uv, m.face_uvs)
    uv = tex_uv[hit_slot >= 0]
    assert uv.shape[0] > 200
    for R in m.baked.tex_res:
        a, b = uv[:, 0] * R, uv[:, 1] * R
        ap, bp = R - b, a
        i0, j0 = torch.floor(ap - 0.5), torch.floor(bp - 0.5)
        assert float(torch.minimum(i0, j0).min()) >= 0 and float(torch.maximum(i0, j0).max()) + 1 <= R - 1, R


def _rows(bank, s, d):
    """[R+2, R+2, row bytes] texel rows of (shell, degree) over the whole domain (apron included)."""
    from volsurfs_amd.neural_textures import MAX_DEG, ROW_QUADS
    R = bank.tex_res[d]
    W, Q, sd = R + 2, ROW_QUADS[d], s * MAX_DEG + d
    off = int(bank.plan.dom_off[sd])
    rel = (bank.slot_of[off:off + W * W] - bank.seg_start[sd]).long()
    idx = (int(bank.plan.row_base[sd]) + rel[:, None] * Q) * 4 + torch.arange(Q * 4, device=rel.device)
    return bank.texels[idx].view(W, W, Q * 4)


def _reference_planes(tex, s, d, R, has_alpha):
    """The reference's layout restated literally (baker.py:826-897, neural_texture.py:200-251): the network at the
    texel centres of meshgrid(u_pix, v_pix, indexing="ij") through pix_to_texel_center_uv_coord(flip=True),
    reshaped to [R, R, C], split into [3, n] / [1, n], concatenated and flipud.  The values are looked up in
    baked_textures() ([iy, ix] of the network input (x, y))."""
    from oracle import uv as OUV
    n = 2 * d + 1
    u_pix, v_pix = torch.meshgrid(torch.arange(R), torch.arange(R), indexing="ij")
    uv = OUV.pix_to_texel_center_uv_coord(torch.stack([u_pix.flatten(), v_pix.flatten()], 1), (R, R), flip=True)
    ix, iy = torch.floor(uv[:, 0] * R).long(), torch.floor(uv[:, 1] * R).long()
    rgb = tex[(s, 0, d)].cpu()[iy, ix].reshape(R, R, 3 * n).numpy().reshape(R, R, 3, n)
    if has_alpha:
        alpha = tex[(s, 1, d)].cpu()[iy, ix].reshape(R, R, n).numpy().reshape(R, R, 1, n)
    else:
        alpha = np.full((R, R, 1, n), 255, np.uint8)
    full = np.flipud(np.concatenate([rgb, alpha], axis=2))
    return [np.ascontiguousarray(full[:, :, :, i]) for i in range(n)]


def _read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.mode, np.asarray(im)


# ---------------------------------------------------------------------------------------------------------------------
# CPU

def test_opengl_camera_projects_pixel_centres_and_depth_range():
    from oracle.raygen import pinhole_ray
    from volsurfs_amd.texture_export import FAR, NEAR, camera_from_opengl, opengl_camera
    cases = [((0.3, -0.2, -1.5), 700.0, 650.0, 330.0, 210.0, 640, 400),
             ((1.2, 0.4, 0.9), 420.0, 450.0, 180.5, 260.0, 360, 480),
             ((-0.5, 1.1, -0.2), 900.0, 900.0, 510.0, 355.0, 1000, 720)]
    rng = np.random.default_rng(0)
    for eye, fx, fy, cx, cy, W, H in cases:
        cam = _cpu_camera(eye, fx, fy, cx, cy, W, H)
        P, M = opengl_camera(cam)
        assert P.dtype == np.float64 and M.dtype == np.float64 and P.shape == M.shape == (4, 4)
        view = P @ np.linalg.inv(M)
        c2w, kinv = cam.c2w.numpy(), cam.intrinsics_inv.numpy()
        for _ in range(20):
            x, y = rng.integers(0, W), rng.integers(0, H)
            o, d = pinhole_ray(c2w, kinv, x + 0.5, y + 0.5)
            for t in (0.5, 2.0, 7.0):
                clip = view @ np.append(o.astype(np.float64) + t * d.astype(np.float64), 1.0)
                ndc = clip[:3] / clip[3]
                px, py = (ndc[0] + 1) / 2 * W, (1 - ndc[1]) / 2 * H
                assert abs(px - (x + 0.5)) < 1e-3 and abs(py - (y + 0.5)) < 1e-3, (eye, x, y, t, px, py)
        # depths near / far along the optical axis -> ndc z = -1 / +1
        c2w4 = np.eye(4)
        c2w4[:3, :4] = c2w
        for z, want in ((NEAR, -1.0), (FAR, 1.0)):
            clip = view @ (c2w4 @ np.array([0.0, 0.0, z, 1.0]))
            assert abs(clip[2] / clip[3] - want) < 1e-9
        back = camera_from_opengl(P, M, W, H, device="cpu")
        assert (back.height, back.width) == (H, W)
        assert torch.allclose(back.intrinsics, cam.intrinsics, atol=1e-4)
        assert torch.allclose(back.c2w, cam.c2w, atol=1e-6)


def test_scene_info_has_the_reference_keys_and_file_names():
    from volsurfs_amd.texture_export import meshes_info_of, scene_info
    sh_range = (15.0, 12.0, 9.0, 6.0)
    info = meshes_info_of(3, FULL, sh_range, 4, [True, False, False])
    cams = {"train": [_cpu_camera((0.0, 0.0, -1.5), 800.0, 800.0, 400.0, 300.0, 800, 600)] * 3,
            "test": [_cpu_camera((1.0, 0.0, -1.0), 800.0, 800.0, 400.0, 300.0, 800, 600)] * 2}
    sc = scene_info(info, (800, 600), (1.0, 1.0, 1.0), cams)
    assert set(sc) == {"resolution", "bg_color", "meshes", "cameras", "volsurfs_amd"}
    assert sc["resolution"] == [[800, 600]] and sc["bg_color"] == "white"
    assert sc["volsurfs_amd"] == {"format": 1, "lerp": True, "with_alpha_decay": True}
    assert [m["mesh_path"] for m in sc["meshes"]] == [os.path.join("meshes", f"{m}.obj") for m in range(3)]
    assert [m["ignore_alpha"] for m in sc["meshes"]] == [True, False, False]
    for m, mesh in enumerate(sc["meshes"]):
        assert set(mesh) == {"mesh_path", "textures", "ignore_alpha"}
        want = [(d, i) for d in range(4) for i in range(2 * d + 1)]
        assert len(mesh["textures"]) == 16
        for (d, i), t in zip(want, mesh["textures"]):
            assert set(t) == {"texture_path", "texture_scale", "texture_resolution"}
            assert t["texture_path"] == os.path.join("textures", f"mesh_{m}_texture_{d}_feature_{i}.png")
            assert t["texture_scale"] == [-sh_range[d], sh_range[d]]
            assert t["texture_resolution"] == [FULL[d], FULL[d]]
    assert set(sc["cameras"]) == {"test", "train"}
    assert list(sc["cameras"]["train"]) == [0, 1, 2] and list(sc["cameras"]["test"]) == [0, 1]
    for c in list(sc["cameras"]["train"].values()) + list(sc["cameras"]["test"].values()):
        assert set(c) == {"projectionMatrix", "matrixWorld"}
        assert np.asarray(c["projectionMatrix"]).shape == (4, 4) and np.asarray(c["matrixWorld"]).shape == (4, 4)
    back = json.loads(json.dumps(sc))
    assert list(back["cameras"]["test"]) == ["0", "1"]
    assert scene_info(info, (8, 8), None, None)["bg_color"] == "black"
    assert scene_info(info, (8, 8), (0.0, 0.0, 0.0), None)["bg_color"] == "black"
    assert scene_info(info, (8, 8), (0.25, 0.5, 1.0), None)["bg_color"] == [0.25, 0.5, 1.0]
    assert scene_info(info, (8, 8), None, None, lerp=False, with_alpha_decay=False)["volsurfs_amd"] == \
        {"format": 1, "lerp": False, "with_alpha_decay": False}


# ---------------------------------------------------------------------------------------------------------------------
# GPU

@pytest.mark.gpu
def test_export_planes_orientation_and_bytes():
    from oracle import neural_texture as ONT
    from oracle import tcnn_like
    from oracle import uv as OUV
    from test_nt_mlp import unpack_weights
    from volsurfs_amd.texture_export import export_planes
    m = _method(_shells(K=3))
    baked = m.bake()
    tex = baked.baked_textures()
    planes = export_planes(baked)
    assert set(planes) == {(s, d) for s in range(3) for d in range(4)}
    for (s, d), p in planes.items():
        R, n = SMALL[d], 2 * d + 1
        assert p.shape == (n, R, R, 4) and p.dtype == torch.uint8 and p.is_cuda
        want = _reference_planes(tex, s, d, R, has_alpha=True)
        got = p.cpu().numpy()
        for i in range(n):
            assert np.array_equal(got[i], want[i]), (s, d, i)
        # png[floor(v R), floor(u R)] is the texel a hit at uv reads under anchor addressing (nt_footprint)
        g = torch.Generator().manual_seed(7 + s * 4 + d)
        for u, v in torch.rand(16, 2, generator=g).tolist():
            r, c = int(np.floor(v * R)), int(np.floor(u * R))
            ix, iy = (R - 1) - min(max(int(np.floor(v * R)), 0), R - 1), min(max(int(np.floor(u * R)), 0), R - 1)
            rgb, alpha = tex[(s, 0, d)][iy, ix].cpu(), tex[(s, 1, d)][iy, ix].cpu()
            for i in range(n):
                px = p[i, r, c].cpu()
                assert [int(px[ch]) for ch in range(3)] == [int(rgb[ch * n + i]) for ch in range(3)]
                assert int(px[3]) == int(alpha[i])
    # against the oracle network at the texel centres of the reference's bake grid
    geom = tcnn_like.GridGeometry()
    for s, d in [(0, 3), (2, 1), (1, 0)]:
        R, n = SMALL[d], 2 * d + 1
        u_pix, v_pix = torch.meshgrid(torch.arange(R), torch.arange(R), indexing="ij")
        uv = OUV.pix_to_texel_center_uv_coord(torch.stack([u_pix.flatten(), v_pix.flatten()], 1), (R, R), flip=True)
        outs = []
        for typ, C in ((0, 3 * n), (1, n)):
            x = baked.tex_index(s, typ, d)
            feats = tcnn_like.hashgrid_forward(geom, baked.tables_h[x].cpu(), uv.float())
            w1, w2, w3 = unpack_weights(baked.weights_h[x].cpu())
            _, q = ONT.quantise(tcnn_like.mlp_forward(w1, w2, w3, feats, C))
            outs.append(q.reshape(R, R, -1, n).numpy())
        want = np.flipud(np.concatenate(outs, axis=2)).astype(np.int32)
        got = planes[(s, d)].cpu().numpy().transpose(1, 2, 3, 0).astype(np.int32)    # [R, R, 4, n]
        dq = np.abs(got - want)
        assert dq.max() <= 1 and (dq > 0).mean() < 2e-3, (s, d, dq.max())


@pytest.mark.gpu
def test_export_planes_refuses_a_bank_that_is_not_baked():
    from volsurfs_amd._lib import VolsurfsHipError
    from volsurfs_amd.texture_export import export_planes
    m = _method(_shells(K=2))
    with pytest.raises(VolsurfsHipError):
        export_planes(m.bank)


@pytest.mark.gpu
def test_extract_textures_writes_the_reference_file_set(tmp_path):
    from volsurfs_amd.mesh import load_obj
    from volsurfs_amd.texture_export import export_planes, extract_textures
    meshes = _shells(K=2)
    m = _method(meshes)
    out = str(tmp_path / "scene")
    sc = extract_textures(m, out, compress_level=1)
    names = {f"mesh_{s}_texture_{d}_feature_{i}.png" for s in range(2) for d in range(4) for i in range(2 * d + 1)}
    assert set(os.listdir(os.path.join(out, "textures"))) == names
    assert set(os.listdir(os.path.join(out, "meshes"))) == {"0.obj", "1.obj"}
    assert set(os.listdir(out)) == {"textures", "meshes", "scene.json"}
    with open(os.path.join(out, "scene.json")) as f:
        assert json.load(f) == json.loads(json.dumps(sc))
    assert sc["bg_color"] == "white" and [x["ignore_alpha"] for x in sc["meshes"]] == [False, False]
    planes = export_planes(m.baked)
    for (s, d), p in planes.items():
        for i in range(2 * d + 1):
            mode, img = _read_png(os.path.join(out, "textures", f"mesh_{s}_texture_{d}_feature_{i}.png"))
            assert mode == "RGBA" and np.array_equal(img, p[i].cpu().numpy()), (s, d, i)
    for s in range(2):
        back = load_obj(os.path.join(out, "meshes", f"{s}.obj"))
        assert torch.equal(back.vertices, meshes[s].vertices) and torch.equal(back.faces, meshes[s].faces)
        assert torch.equal(back.get_faces_uvs(), meshes[s].get_faces_uvs())


@pytest.mark.gpu
def test_round_trip_on_atlas_shells_renders_bit_identically(tmp_path):
    from volsurfs_amd.texture_export import extract_textures, load_scene
    m = _method(_atlas_shells(K=2), res=FULL)
    out = str(tmp_path / "scene")
    extract_textures(m, out, compress_level=1)
    scene = load_scene(out)
    assert scene.baked.tables is None and scene.baked.weights is None and scene.baked.features is None
    assert scene.baked.grad_rows is None
    for H, W, focal in ((64, 64, 110.0), (48, 80, 70.0)):
        o, d = _view(H, W, focal)
        _no_footprint_in_apron(m, o, d)
        want = m.render_baked(o, d)
        assert (want["surfs_alpha"].sum((1, 2)) > 0).sum() > 200
        _assert_same_render(scene.render_rays(o, d), want)


@pytest.mark.gpu
def test_import_fills_the_apron_by_clamp_to_edge(tmp_path):
    """Octahedral UVs reach the texture border: the loaded bank's interior rows are the baked bank's, byte for byte,
    and its apron rows are copies of their clamp-to-edge neighbours."""
    from volsurfs_amd.texture_export import extract_textures, load_scene
    m = _method(_shells(K=2))
    out = str(tmp_path / "scene")
    extract_textures(m, out, compress_level=1)
    loaded = load_scene(out).baked
    for s in range(2):
        for d in range(4):
            R = SMALL[d]
            a, b = _rows(loaded, s, d), _rows(m.baked, s, d)
            assert torch.equal(a[1:R + 1, 1:R + 1], b[1:R + 1, 1:R + 1]), (s, d)
            idx = torch.arange(R + 2, device=a.device).clamp(1, R)
            assert torch.equal(a, a[idx][:, idx]), (s, d)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["solid", "shared", "solid_shared", "anchor"])
def test_variants_round_trip(tmp_path, variant):
    from volsurfs_amd.texture_export import extract_textures, load_scene
    kw = {"solid": dict(is_inner_mesh_solid=True),
          "shared": dict(are_volsurfs_colors_indep=False, are_volsurfs_alphas_indep=False),
          "solid_shared": dict(is_inner_mesh_solid=True, are_volsurfs_alphas_indep=False),
          "anchor": dict(using_neural_textures_anchor=True, using_neural_textures_lerp=False)}[variant]
    m = _method(_atlas_shells(K=3), res=(512, 256, 256, 256), **kw)
    out = str(tmp_path / "scene")
    sc = extract_textures(m, out, compress_level=1)
    ignore = {"solid": [True, False, False], "solid_shared": [True, True, True]}.get(variant, [False] * 3)
    assert [x["ignore_alpha"] for x in sc["meshes"]] == ignore
    assert sc["volsurfs_amd"]["lerp"] == (variant != "anchor")
    for s, ign in enumerate(ignore):
        _, img = _read_png(os.path.join(out, "textures", f"mesh_{s}_texture_2_feature_3.png"))
        if ign:
            assert (img[..., 3] == 255).all()
    scene = load_scene(out)
    assert bool(scene.baked.plan.anchor) == (variant == "anchor")
    o, d = _view(64, 64, 110.0)
    _no_footprint_in_apron(m, o, d)
    want = m.render_baked(o, d)
    assert (want["surfs_alpha"].sum((1, 2)) > 0).sum() > 200
    _assert_same_render(scene.render_rays(o, d), want)


@pytest.mark.gpu
def test_refusals():
    from volsurfs_amd._lib import VolsurfsHipError
    from volsurfs_amd.methods import VolSurfs
    from volsurfs_amd.texture_export import extract_textures
    meshes = _shells(K=2)
    for kw in (dict(using_neural_textures=False), dict(using_sh_quantization=False),
               dict(transp_view_dep=False, sh_degree=3)):
        m = VolSurfs(meshes, max_rays=4096, textures_res=SMALL, **kw)
        with pytest.raises(VolsurfsHipError):
            extract_textures(m, "/nonexistent/never/written")


@pytest.mark.gpu
def test_load_scene_validates_and_defaults(tmp_path):
    from PIL import Image
    from volsurfs_amd._lib import VolsurfsHipError
    from volsurfs_amd.texture_export import extract_textures, load_scene
    m = _method(_atlas_shells(K=2), res=(256, 256, 256, 256))
    out = str(tmp_path / "scene")
    extract_textures(m, out, compress_level=1)
    scene_json = os.path.join(out, "scene.json")
    with open(scene_json) as f:
        meta = json.load(f)

    def write(x):
        with open(scene_json, "w") as f:
            json.dump(x, f)

    # no "volsurfs_amd" key: lerp and alpha decay, the shipped configs (the settings of this method)
    write({k: v for k, v in meta.items() if k != "volsurfs_amd"})
    o, d = _view(64, 64, 110.0)
    _assert_same_render(load_scene(out).render_rays(o, d), m.render_baked(o, d))
    # per-mesh resolutions that differ
    bad = json.loads(json.dumps(meta))
    for t in bad["meshes"][1]["textures"][:1]:
        t["texture_resolution"] = [128, 128]
    write(bad)
    with pytest.raises(VolsurfsHipError, match="every shell must match"):
        load_scene(out)
    write(meta)
    # a PNG whose size is not texture_resolution, and one without alpha
    png = os.path.join(out, "textures", "mesh_1_texture_1_feature_2.png")
    img = Image.open(png).convert("RGBA")
    img.resize((128, 128)).save(png)
    with pytest.raises(VolsurfsHipError, match="pixels"):
        load_scene(out)
    img.convert("RGB").save(png)
    with pytest.raises(VolsurfsHipError, match="RGBA"):
        load_scene(out)
    img.save(png)
    _assert_same_render(load_scene(out).render_rays(o, d), m.render_baked(o, d))


@pytest.mark.gpu
def test_render_and_eval_from_scene_matches_the_method(tmp_path):
    from volsurfs_amd.camera import Camera
    from volsurfs_amd.evaluation import render_and_eval
    from volsurfs_amd.renderers import VolsurfsRenderer
    from volsurfs_amd.texture_export import extract_textures
    m = _method(_atlas_shells(K=2), res=(512, 256, 256, 256))
    cams = [Camera.look_at(eye, focal=120.0, height=64, width=64) for eye in
            ((0.0, 0.0, -1.5), (1.0, 0.3, -1.1), (-0.8, -0.5, 1.2))]
    g = torch.Generator().manual_seed(3)
    splits = {"test": (cams[:2], torch.rand(2, 64, 64, 3, generator=g)),
              "train": (cams[2:], torch.rand(1, 64, 64, 3, generator=g))}
    out = str(tmp_path / "scene")
    sc = extract_textures(m, out, cameras={"train": cams[2:], "test": cams[:2]}, compress_level=1)
    assert sc["resolution"] == [[64, 64]]
    r = VolsurfsRenderer.from_scene(out)
    assert len(r.method.cameras["test"]) == 2 and len(r.method.cameras["train"]) == 1
    for cam, back in zip(cams[:2], r.method.cameras["test"]):
        assert torch.allclose(back.c2w.cpu(), cam.c2w.cpu(), atol=1e-5)
    want = render_and_eval(VolsurfsRenderer(m), splits, save_pngs=False)
    got = render_and_eval(r, splits, save_pngs=False)
    for split in splits:
        assert got[split]["psnr"] == want[split]["psnr"] and got[split]["ssim"] == want[split]["ssim"], split
        assert np.isfinite(got[split]["psnr"])


@pytest.mark.gpu
def test_full_size_round_trip(tmp_path):
    """K = 5 at the default textures_res and sh_degree 3: 80 PNGs, one 800 x 800 view."""
    from volsurfs_amd.camera import Camera, get_camera_rays
    from volsurfs_amd.texture_export import extract_textures, load_scene
    m = _method(_atlas_shells(K=5, subdiv=4), res=FULL)
    m.bake()
    out = str(tmp_path / "scene")
    t0 = time.perf_counter()
    extract_textures(m, out, compress_level=1)
    t1 = time.perf_counter()
    scene = load_scene(out)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"full-size export {t1 - t0:.2f} s, load {t2 - t1:.2f} s")
    assert len(os.listdir(os.path.join(out, "textures"))) == 80
    assert t1 - t0 < FULL_EXPORT_S_MAX and t2 - t1 < FULL_LOAD_S_MAX
    cam = Camera.look_at((0.0, 0.0, -1.5), focal=1500.0, height=800, width=800)
    o, d, _ = get_camera_rays(cam)
    _no_footprint_in_apron(m, o, d)
    want = m.render_baked(o, d)
    assert (want["surfs_alpha"].sum((1, 2)) > 0).sum() > 100000
    _assert_same_render(scene.render_rays(o, d), want)
