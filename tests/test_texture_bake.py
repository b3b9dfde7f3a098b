"""Texture bake of field appearance models (volsurfs_amd/texture_bake.py, csrc/texture_bake.hip): the
restatement of the sampling / ownership / mean rule and of the dilation rule against the fixture recorded from the
reference's own functions (tools/make_texture_bake_golden.py), the device passes against the fixture and against the
restatement, the properties of the supersampled bake, and the way through `extract_field_textures` into
`renderers.MeshRenderer`."""
import json
import os

import numpy as np
import pytest
import torch

import texture_bake_restated as TB

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "texture_bake.npz")
RESOLUTIONS = (32, 48, 64)
# Bounds of the device-against-fixture test (conditions, not measurements).  The reference itself, float32 against
# float64 on this fixture: 0 coverage flips at all three resolutions, values within 2.4e-7.
MAX_FLIP_SHARE = 0.002           # of the fixture's covered texels
EDGE_BAND = 1e-4                 # barycentric units: a flipped texel's centre must lie this close to a face's edge
VALUE_TOL = 1e-5                 # the bound DESIGN §21 uses for fp32 points against its fixture


def _fixture(device="cpu"):
    d = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(d[k]).to(device)
    V, F, uv = t("vertices"), t("faces"), t("uvs")
    return d, V, F, uv[F.long()].contiguous()          # per-corner UVs [F, 3, 2]


# ---- CPU

def test_fixture_is_the_recipe():
    d, V, F, uvc = _fixture()
    v, f, uv = TB.fixture_mesh()
    assert np.array_equal(d["vertices"], v.astype(np.float32)) and np.array_equal(d["faces"], f) and \
        np.array_equal(d["uvs"], uv.astype(np.float32))
    assert F.shape[0] == 281 and float(uvc.min()) >= 0 and float(uvc.max()) <= 1
    assert [int((d[f"tex_{R}"] != 0).all(2).sum()) for R in RESOLUTIONS] == [726, 1623, 2870]
    assert all(int(d[f"flips_{R}"]) == 0 and float(d[f"maxdiff_{R}"]) < 3e-7 for R in RESOLUTIONS)


@pytest.mark.parametrize("R", RESOLUTIONS)
def test_restatement_reproduces_the_reference_fixture_on_cpu(R):
    """The sampling / ownership / mean rule restated in torch gives, at S = 1 on the CPU, the coverage the reference's
    own per-face loop gave in float32 and, with the face normal taken through torch's `cross` / `F.normalize` as the
    reference takes it, its bytes.  With the rule's written-out normal the channels that do not read the normal are
    still bit-equal and the three that do are within an ulp (torch's CPU `cross` fuses a b - c d: DESIGN §22)."""
    d, V, F, uvc = _fixture()
    ref = torch.from_numpy(d[f"tex_{R}"])
    tex, owner = TB.bake_restated(TB.analytic_fn, V, F, uvc, R, 1, torch_normal=True)
    assert torch.equal((owner >= 0), (ref != 0).all(2))
    assert torch.equal(tex, ref), f"max gap {float((tex - ref).abs().max()):.3e}"
    tex, owner2 = TB.bake_restated(TB.analytic_fn, V, F, uvc, R, 1)
    assert torch.equal(owner, owner2)
    assert torch.equal(tex[..., [0, 1, 2, 6, 7]], ref[..., [0, 1, 2, 6, 7]])
    assert float((tex[..., 3:6] - ref[..., 3:6]).abs().max()) <= 2.0 ** -23       # an ulp of a value in [0.75, 1.25]


def test_dilation_restatement_reproduces_the_reference_fixtures():
    d = np.load(GOLDEN)
    for n in (5, 50):
        assert np.array_equal(TB.dilate_restated(d["tex_64"], n), d[f"tex_64_dilated_{n}"]), n
    for n in (1, 2, 5, 50):
        assert np.array_equal(TB.dilate_restated(d["syn"], n), d[f"syn_dilated_{n}"]), n
    # the fixtures hold what they are meant to: the partial-zero pixel stays, 50 iterations reach the early stop
    assert np.array_equal(d["syn_dilated_50"][12, 13], d["syn"][12, 13]) and d["syn"][12, 13, 1] == 0
    assert np.array_equal(d["tex_64_dilated_50"], TB.dilate_restated(d["tex_64"], 500))
    assert not np.array_equal(d["tex_64_dilated_5"], d["tex_64_dilated_50"])


def test_uniform_is_a_function_of_its_key_only():
    """Guards the restatement's generator only (the device's is held to it by the bit-for-bit GPU test): a number
    depends on nothing but its key."""
    t = torch.arange(0, 5000, dtype=torch.int64)
    a = TB.uniform(3, 7, t, 12, 5, 1)
    assert torch.equal(a[1234:1235], TB.uniform(3, 7, t[1234:1235], 12, 5, 1))
    assert float(a.min()) >= 0 and float(a.max()) < 1 and abs(float(a.mean()) - 0.5) < 4 / (12 * 5000) ** 0.5
    assert not torch.equal(a, TB.uniform(4, 7, t, 12, 5, 1)) and not torch.equal(a, TB.uniform(3, 7, t, 12, 5, 0))


def test_header_declares_the_texture_bake_entry_points():
    import ctypes
    from volsurfs_amd import _lib
    names = ["vsa_tb_workspace_bytes", "vsa_tb_max_chunks", "vsa_tb_samples", "vsa_tb_emit", "vsa_tb_resolve",
             "vsa_tb_dilate"]
    declared, protos = _lib.declared_symbols(), _lib.declared_prototypes()
    for n in names:
        assert n in declared and n in protos
    assert protos["vsa_tb_workspace_bytes"] == (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int])
    assert len(protos["vsa_tb_samples"][1]) == 12 and protos["vsa_tb_samples"][1][4] is ctypes.c_ulonglong
    assert len(protos["vsa_tb_emit"][1]) == 14 and len(protos["vsa_tb_dilate"][1]) == 8
    L = _lib.lib()
    assert L.vsa_tb_workspace_bytes(0, 64) == -1 and L.vsa_tb_workspace_bytes(10, 8193) == -1
    assert L.vsa_tb_max_chunks(64, 65, 1000) == -1 and L.vsa_tb_max_chunks(64, 12, 11) == -1
    assert L.vsa_tb_max_chunks(4096, 12, 12) == -1 and L.vsa_tb_max_chunks(2048, 12, 1 << 20) == 50
    assert L.vsa_tb_samples(None, 10, 64, 12, 0, 1000, None, 0, None, None, 0, None) == -1
    assert L.vsa_tb_dilate(None, 4, 4, 3, 1, None, None, None) == -1


def test_argument_refusals_that_need_no_device():
    from volsurfs_amd import texture_bake as tb
    from volsurfs_amd._lib import VolsurfsHipError
    from volsurfs_amd.mesh import TensorMesh
    _, V, F, uvc = _fixture()
    mesh = TensorMesh(V, F, uvc, device="cpu")
    for R in (0, 8193):
        with pytest.raises(ValueError, match="texture_res"):
            tb.bake_samples(mesh, R, 1)
    for S in (0, 65):
        with pytest.raises(ValueError, match="nr_samples_per_texel"):
            tb.bake_samples(mesh, 64, S)
    with pytest.raises(ValueError, match="chunk_rows"):
        tb.bake_samples(mesh, 64, 12, chunk_rows=11)
    with pytest.raises(VolsurfsHipError, match="no UVs"):
        tb.bake_samples(TensorMesh(V, F, None, device="cpu"), 64, 1)
    with pytest.raises(ValueError, match="cuda"):
        tb.bake_samples(mesh, 64, 1)
    with pytest.raises(ValueError, match="cuda tensor"):
        tb.dilate_texture(torch.zeros(4, 4, 3), 1)


# ---- GPU: the bake

def _device_mesh():
    from volsurfs_amd.mesh import TensorMesh
    d, V, F, uvc = _fixture("cuda")
    return d, TensorMesh(V, F, uvc, device="cuda")


def _edge_distance(uvc, R, texels):
    """Per texel (ix, iy rows of `texels`): the smallest |barycentric coordinate| of its centre over all faces, in
    float64."""
    uv = uvc.double().cpu().numpy()
    c = (texels.astype(np.float64) + 0.5) / R
    p1, p2, p3 = uv[:, 0], uv[:, 1], uv[:, 2]
    v0, v1 = p3 - p1, p2 - p1
    d00, d01, d11 = (v0 * v0).sum(1), (v0 * v1).sum(1), (v1 * v1).sum(1)
    inv = 1.0 / (d00 * d11 - d01 * d01)
    v2 = c[:, None, :] - p1[None]
    d02, d12 = (v0[None] * v2).sum(2), (v1[None] * v2).sum(2)
    b2, b1 = (d11 * d02 - d01 * d12) * inv, (d00 * d12 - d01 * d02) * inv
    b = np.stack([1 - b1 - b2, b1, b2], 2)
    return np.abs(b).min(2).min(1)


@pytest.mark.gpu
def test_device_bake_against_the_reference_fixture():
    """S = 1 on the device, the callable evaluated by torch on the device, against the reference's recorded textures.
    Measured on MI355X: see DESIGN §22 (the figures are printed before the assertion)."""
    from volsurfs_amd.texture_bake import bake_field_texture
    d, mesh = _device_mesh()
    failures = []
    for R in RESOLUTIONS:
        tex, owner = bake_field_texture(TB.analytic_fn, mesh, R, 1, return_owner=True)
        ref = torch.from_numpy(d[f"tex_{R}"]).cuda()
        cov, rcov = owner >= 0, (ref != 0).all(2)
        assert tex.shape == ref.shape and tex.dtype == torch.float32
        assert torch.equal(cov, (tex != 0).all(2))
        flips = (cov != rcov).nonzero().cpu().numpy()
        far = int((_edge_distance(mesh.faces_uvs, R, flips) > EDGE_BAND).sum()) if len(flips) else 0
        both = cov & rcov
        gap = float((tex - ref).abs()[both].max())
        print(f"texture bake fixture R = {R}: {int(cov.sum())} covered (reference {int(rcov.sum())}), {len(flips)} "
              f"flips, {far} of them farther than {EDGE_BAND} from every edge, max value gap {gap:.3e}")
        if len(flips) > MAX_FLIP_SHARE * int(rcov.sum()) or far or gap > VALUE_TOL:
            failures.append((R, len(flips), far, gap))
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("S", (1, 4, 12))
def test_device_bake_matches_the_restatement_bit_for_bit(S):
    from volsurfs_amd.texture_bake import bake_field_texture
    _, mesh = _device_mesh()
    R = 64
    tex, owner = bake_field_texture(TB.analytic_fn, mesh, R, S, seed=5, return_owner=True)
    want, wowner = TB.bake_restated(TB.analytic_fn, mesh.vertices, mesh.faces, mesh.faces_uvs, R, S, seed=5)
    assert torch.equal(owner, wowner), f"{int((owner != wowner).sum())} owners differ"
    assert torch.equal(tex, want), f"max gap {float((tex - want).abs().max()):.3e}"
    again = bake_field_texture(TB.analytic_fn, mesh, R, S, seed=5)
    assert torch.equal(tex, again)
    if S > 1:
        assert not torch.equal(tex, bake_field_texture(TB.analytic_fn, mesh, R, S, seed=6))
    for chunk_rows in (4096, 1000):
        assert torch.equal(tex, bake_field_texture(TB.analytic_fn, mesh, R, S, seed=5, chunk_rows=chunk_rows))


def _row_is_batch_independent(fn):
    g = torch.Generator("cuda").manual_seed(5)
    big = (torch.rand(100000, 3, device="cuda", generator=g) - 0.5) * 0.8
    nrm = torch.nn.functional.normalize(torch.rand(100000, 3, device="cuda", generator=g) - 0.5, dim=1)
    a = 40000
    with torch.no_grad():
        alone = fn(big[a:a + 1000].clone(), nrm[a:a + 1000].clone())
        inside = fn(big, nrm)[a:a + 1000]
    return torch.equal(alone, inside)


@pytest.mark.gpu
@pytest.mark.parametrize("encoder", ("gridhash", "permutohash"))
def test_chunking_does_not_change_model_bakes(encoder):
    """First the premise (a row's output does not depend on the batch it is in, for ColorSH and RGB with both position
    encoders and the fused MLP), then: one chunk, 4096-row and 1000-row chunks give the same bytes."""
    from volsurfs_amd.models import RGB, ColorSH
    from volsurfs_amd.texture_bake import extract_texture_from_color_model
    _, mesh = _device_mesh()
    torch.manual_seed(3)
    sh = ColorSH(3, [64, 32], encoder, out_channels=3, sh_deg=2, bb_sides=1.0)
    rgb = RGB(3, [64, 32], encoder, "spherical_harmonics", out_channels=3, sh_deg=3, bb_sides=1.0)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for m in (sh, rgb):
            for p in m.pos_encoder.parameters():
                p.copy_(((torch.rand(p.shape, generator=g) * 2 - 1) * 0.5).cuda())
    assert _row_is_batch_independent(lambda p, n: sh(p, samples_dirs=None, normals=n))
    assert _row_is_batch_independent(lambda p, n: rgb(p, samples_dirs=-n, normals=n))
    for model, export_rgb, C in ((sh, False, 27), (rgb, True, 3)):
        args = (model, mesh.vertices, mesh.faces, mesh.faces_uvs)
        one = extract_texture_from_color_model(*args, texture_res=64, nr_samples_per_texel=4, export_rgb=export_rgb)
        assert one.shape == (64, 64, C) and bool((one != 0).any())
        for chunk_rows in (4096, 1000):
            assert torch.equal(one, extract_texture_from_color_model(*args, texture_res=64, nr_samples_per_texel=4,
                                                                     export_rgb=export_rgb, chunk_rows=chunk_rows))


@pytest.mark.gpu
def test_supersampled_bake_properties():
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.texture_bake import bake_field_texture, bake_samples
    _, mesh = _device_mesh()
    R = 64
    t1, o1 = bake_field_texture(TB.analytic_fn, mesh, R, 1, return_owner=True)
    t12, o12 = bake_field_texture(TB.analytic_fn, mesh, R, 12, seed=2, return_owner=True)
    assert bool(((o1 < 0) | (o12 >= 0)).all()) and int((o12 >= 0).sum()) > int((o1 >= 0).sum())
    assert bool((o12 >= o1).all())
    # a per-face constant: every covered texel holds exactly its owner's normal; the owner is the restatement's
    nrm, on = bake_field_texture(lambda p, n: n, mesh, R, 12, seed=2, return_owner=True)
    _, wowner = TB.bake_restated(lambda p, n: n, mesh.vertices, mesh.faces, mesh.faces_uvs, R, 12, seed=2)
    assert torch.equal(on, o12) and torch.equal(on, wowner)
    tri = mesh.vertices[mesh.faces.long()]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    n = n / torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    cov = on >= 0
    # The texel's value is the rule's mean of k copies of the constant v, ((v + v) + ... + v) / k in fp32: v itself for
    # k <= 2, and not always v beyond (3 v need not be a float), in the reference's vals_sum / mask_sum as well.  So:
    # exactly that mean, and exactly v where k <= 2.
    smp = bake_samples(mesh, R, 12, seed=2)
    k = (smp.row_start[1:] - smp.row_start[:-1]).view(R, R)
    assert torch.equal(k > 0, cov)
    v = n[on.clamp(min=0).long()]
    total = v.clone()
    for j in range(1, 12):
        total = torch.where((k > j)[..., None], total + v, total)
    mean = total / k.clamp(min=1).float()[..., None]
    assert torch.equal(nrm[cov], mean[cov])
    assert torch.equal(nrm[cov & (k <= 2)], v[cov & (k <= 2)]) and int((cov & (k <= 2)).sum()) > 0
    assert float((nrm[cov] - v[cov]).abs().max()) <= 2 ** -21
    assert bool((nrm[~cov] == 0).all())
    # |S = 12 value - S = 1 value| <= Lipschitz constant x the texel's 3-D extent on the face, where both have one owner
    same = (o1 >= 0) & (o1 == o12)
    uv, f = mesh.faces_uvs.double(), o1[same].long()
    J = torch.linalg.solve(torch.stack([uv[f, 1] - uv[f, 0], uv[f, 2] - uv[f, 0]], 1),
                           torch.stack([tri[f, 1] - tri[f, 0], tri[f, 2] - tri[f, 0]], 1).double())   # [n, 2, 3]
    reach = torch.linalg.matrix_norm(J, ord=2) * (2 ** 0.5) * (0.5 + 1e-6) / R
    L = torch.tensor(TB.AnalyticAppearance.LIPSCHITZ, dtype=torch.float64, device="cuda")
    gap = (t12[same] - t1[same]).abs().double()
    print(f"S = 12 against S = 1 on {int(same.sum())} texels: largest gap {float(gap.max()):.3e}, largest share of its "
          f"bound {float((gap / (L[None] * reach[:, None] + 1e-6)).max()):.3f}")
    assert bool((gap <= L[None] * reach[:, None] + 1e-6).all())       # 1e-6: fp32 rounding of values up to 3
    # the jitter, read off a mesh whose points are its UVs: two triangles over the unit square
    sq = TensorMesh([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 1, 2], [0, 2, 3]],
                    [[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], device="cuda")
    S = 32
    smp = bake_samples(sq, R, S, seed=8)
    cnt = smp.row_start[1:] - smp.row_start[:-1]
    full = (cnt == S).nonzero()[:, 0]                                   # texels with every sample inside one face
    rows = smp.row_start[full].long()[:, None] + torch.arange(1, S, device="cuda")[None]
    centre = torch.stack([(full // R).float() + 0.5, (full % R).float() + 0.5], 1).double() / R
    jit = (smp.points[rows.reshape(-1)][:, :2].double().reshape(-1, S - 1, 2) - centre[:, None]).reshape(-1, 2) * R
    assert jit.shape[0] >= 100000
    se = (1 / 12) ** 0.5 / jit.shape[0] ** 0.5
    print(f"jitter of {jit.shape[0]} samples (texel units): mean {jit.mean(0).tolist()}, standard error {se:.2e}, "
          f"range [{float(jit.min()):.7f}, {float(jit.max()):.7f}]")
    assert bool(((jit.mean(0) + 1e-6).abs() <= 4 * se).all())
    # the points are barycentric reconstructions of the sample positions: 4 ulp of a coordinate below 1, in texels
    slack = 4 * 2.0 ** -24 * R
    assert float(jit.min()) >= -0.5 - 1e-6 - slack and float(jit.max()) < 0.5 - 1e-6 + slack
    assert bool((smp.normals == torch.tensor([0.0, 0.0, 1.0], device="cuda")).all())


@pytest.mark.gpu
def test_dilation_on_the_device_reproduces_the_reference_fixtures():
    from volsurfs_amd.texture_bake import dilate_texture
    d = np.load(GOLDEN)
    for key, iters in (("tex_64", (5, 50)), ("syn", (1, 2, 5, 50))):
        src = torch.from_numpy(d[key]).cuda()
        for n in iters:
            out = dilate_texture(src, n)
            assert torch.equal(out, torch.from_numpy(d[f"{key}_dilated_{n}"]).cuda()), (key, n)
        assert torch.equal(src, torch.from_numpy(d[key]).cuda())            # the input is not written
        assert torch.equal(dilate_texture(src, 0), src)
        assert torch.equal(dilate_texture(src, 500), dilate_texture(src, 50))   # the early stop


# ---- GPU: the way into the renderer

def _legacy_method(K=1, subdiv=4, seed=2, **kw):
    from volsurfs_amd.atlas import compute_atlas
    from volsurfs_amd.mesh import nested_shells
    from volsurfs_amd.methods import VolSurfs
    torch.manual_seed(seed)
    meshes = [compute_atlas(m, 1024, 4) for m in nested_shells(K=K, subdiv=subdiv, r0=0.3, dr=0.03)]
    m = VolSurfs(meshes, max_rays=4096, using_neural_textures=False, appearance_predict_sh_coeffs=True, sh_degree=2,
                 rgb_pos_encoder_type="permutohash", rgb_mlp_layers_dims=(64, 32), bb_sides=1.0, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        # The seeded initial weights give a field too flat to tell a flipped layout (lattice values of 1e-5, small
        # last-layer weights: a flipped oracle bake lost 7.6 dB), so they are perturbed: the 8 coarsest lattice levels
        # (scales 1 to 0.06, well resolved by a texel) drawn from N(0, 0.5^2), the last layer's weights times 10.
        for mod in m.models.values():
            lv = mod.pos_encoder.encoder.lattice_values
            lv[:8].copy_((torch.randn(lv[:8].shape, generator=g) * 0.5).cuda())
            mod.mlp.layers[-1].weight.mul_(10.0)
    return m


def _psnr(a, b):
    return float(-10.0 * torch.log10(((a - b) ** 2).mean()))


@pytest.mark.gpu
def test_end_to_end_bake_renders_like_the_model(tmp_path):
    """A one-shell legacy VolSurfs -> extract_field_textures (R = 1024, S = 4) -> MeshRenderer(scene_path) against the
    models evaluated directly at the hit points.  The yardstick is an oracle bake: the models evaluated exactly at the
    texel centres of the owner map, which isolates the interpolation error.  Figures: DESIGN §22."""
    from volsurfs_amd.camera import Camera, get_camera_rays
    from volsurfs_amd.models import sh_eval
    from volsurfs_amd.renderers import MeshRenderer
    from volsurfs_amd.texture_bake import bake_field_texture, extract_field_textures, to_renderer_layout
    m = _legacy_method()
    R = 1024
    scene = extract_field_textures(m, str(tmp_path), R, nr_samples_per_texel=4)
    assert scene["meshes"][0]["ignore_alpha"] is False
    tex = np.load(tmp_path / "textures" / "mesh_0.npy")
    assert tex.shape == (R, R, 36) and tex.dtype == np.float32
    cam = Camera.look_at((0.5, 0.4, -1.0), focal=220.0, height=128, width=128)
    o, d, _ = get_camera_rays(cam)
    mesh = m.tensor_meshes[0]
    rgb_m, alpha_m = m.models["rgb_0"], m.models["alpha_0"]

    def render(renderer):
        out = renderer.render_rays(o, d)["renders"]["ray_traced"]
        return torch.cat([out["rgb"], out["alpha"]], 1), out["is_hit"][:, 0] > 0

    got, hit = render(MeshRenderer(scene_path=str(tmp_path)))
    assert int(hit.sum()) > 2000
    tr = MeshRenderer(tensor_mesh=mesh, texture=tex).raytracer.trace(o, d)
    pts, dirs = tr["positions"][hit], d[hit]
    with torch.no_grad():
        coeffs = torch.cat([rgb_m(pts, samples_dirs=None), alpha_m(pts, samples_dirs=None)], 1).view(-1, 4, 9)
        direct = torch.sigmoid(sh_eval(coeffs, dirs, degree=2))
    # the oracle bake: the models at the owner's texel-centre points
    centre, owner = bake_field_texture(lambda p, n: torch.cat([p, n], 1), mesh, R, 1, return_owner=True)
    cov = owner >= 0
    with torch.no_grad():
        cp = centre[cov][:, :3].contiguous()
        oracle = torch.zeros(R, R, 36, device="cuda")
        oracle[cov] = torch.cat([rgb_m(cp, samples_dirs=None), alpha_m(cp, samples_dirs=None)], 1)
    want, hit2 = render(MeshRenderer(tensor_mesh=mesh, texture=to_renderer_layout(oracle)))
    flipped, _ = render(MeshRenderer(tensor_mesh=mesh, texture=oracle))
    assert torch.equal(hit, hit2)
    e_dev, e_or = (got[hit] - direct).abs().mean(), (want[hit] - direct).abs().mean()
    p_dev, p_or, p_flip = _psnr(got[hit], direct), _psnr(want[hit], direct), _psnr(flipped[hit], direct)
    print(f"end to end: mean |error| device bake {float(e_dev):.3e}, oracle bake {float(e_or):.3e}; PSNR device "
          f"{p_dev:.2f} dB, oracle {p_or:.2f} dB, oracle in the un-flipped layout {p_flip:.2f} dB")
    assert p_flip <= p_or - 10.0, "the field is too flat to tell a flipped layout"
    assert float(e_dev) <= 1.5 * float(e_or) and p_dev >= p_or - 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("kw,K", (({"is_inner_mesh_solid": True}, 2),
                                  ({"are_volsurfs_colors_indep": False, "are_volsurfs_alphas_indep": False}, 2),
                                  ({}, 3)))
def test_scene_round_trip_and_dilation(tmp_path, kw, K):
    from volsurfs_amd.camera import Camera, get_camera_rays
    from volsurfs_amd.mesh import load_obj
    from volsurfs_amd.renderers import MeshRenderer
    from volsurfs_amd.texture_bake import extract_field_textures, extract_textures
    m = _legacy_method(K=K, subdiv=3, **kw)
    R = 128
    plain, dil = tmp_path / "plain", tmp_path / "dilated"
    scene = extract_field_textures(m, str(plain), R, nr_samples_per_texel=2)
    extract_field_textures(m, str(dil), R, nr_samples_per_texel=2, dilate=True, nr_dilation_iters=3)
    with open(plain / "scene.json") as f:
        assert json.load(f)["meshes"] == scene["meshes"] and len(scene["meshes"]) == K
    o, d, _ = get_camera_rays(Camera.look_at((0.0, 0.3, -1.2), focal=60.0, height=48, width=48))
    for k in range(K):
        solid = bool(kw.get("is_inner_mesh_solid")) and k == 0
        assert scene["meshes"][k]["ignore_alpha"] is solid
        tex, none = extract_textures(k, m, R, 2)
        assert none is None and tex.shape == (R, R, 27 if solid else 36)
        a, b = np.load(plain / "textures" / f"mesh_{k}.npy"), np.load(dil / "textures" / f"mesh_{k}.npy")
        assert np.array_equal(a, torch.flip(tex, [1]).cpu().numpy())
        covered = (a != 0).all(2)
        assert np.array_equal(a[covered], b[covered]) and int(((b != 0).all(2) & ~covered).sum()) > 0
        mesh = load_obj(str(plain / "meshes" / f"{k}.obj"))
        assert mesh.faces.shape == m.tensor_meshes[k].faces.shape
        if solid:       # no alpha model: the renderer wants 4 channels of coefficients, the test supplies an opaque one
            opaque = np.zeros((R, R, 9), np.float32)
            opaque[..., 0] = 100.0
            a = np.concatenate([a, opaque], 2)
        out = MeshRenderer(tensor_mesh=mesh, texture=a).render_rays(o, d)["renders"]["ray_traced"]
        assert int(out["is_hit"].sum()) > 100 and bool(torch.isfinite(out["rgb"]).all())
    if kw.get("are_volsurfs_colors_indep") is False:
        assert set(m.models.keys()) == {"rgb", "alpha"}


@pytest.mark.gpu
def test_refusals_on_the_device(tmp_path):
    from volsurfs_amd import texture_bake as tb
    from volsurfs_amd._lib import VolsurfsHipError
    from volsurfs_amd.mesh import TensorMesh, nested_shells
    from volsurfs_amd.methods import VolSurfs
    _, mesh = _device_mesh()
    for bad in (1.5, -0.25, float("nan"), float("inf")):
        uv = mesh.faces_uvs.clone()
        uv[17, 1, 0] = bad
        with pytest.raises(VolsurfsHipError, match="outside \\[0, 1\\]"):
            tb.bake_field_texture(TB.analytic_fn, TensorMesh(mesh.vertices, mesh.faces, uv), 64, 2)
    with pytest.raises(VolsurfsHipError, match="no UVs"):
        tb.bake_field_texture(TB.analytic_fn, TensorMesh(mesh.vertices, mesh.faces, None), 64, 2)
    with pytest.raises(ValueError, match="nr_samples_per_texel"):
        tb.bake_field_texture(TB.analytic_fn, mesh, 64, 0)
    with pytest.raises(ValueError, match="texture_res"):
        tb.bake_field_texture(TB.analytic_fn, mesh, 10000, 1)
    with pytest.raises(VolsurfsHipError, match="returned"):
        tb.bake_field_texture(lambda p, n: p[:-1], mesh, 64, 2)
    for bad in (-1, int(mesh.vertices.shape[0])):
        faces = mesh.faces.clone()
        faces[40, 2] = bad
        with pytest.raises(VolsurfsHipError, match="face indices out of range"):
            tb.extract_texture_from_color_model(TB.AnalyticAppearance(), mesh.vertices, faces, mesh.faces_uvs, 64, 2)
    with pytest.raises(ValueError, match="2\\^20 chunks"):
        tb.bake_field_texture(TB.analytic_fn, mesh, 4096, 12, chunk_rows=12)
    nt = VolSurfs(nested_shells(K=1, subdiv=2), max_rays=1024, textures_res=(64, 32, 16, 8))
    with pytest.raises(VolsurfsHipError, match="texture_export.extract_textures"):
        tb.extract_field_textures(nt, str(tmp_path), 64)
    # a degenerate face (zero UV area) covers nothing and breaks nothing
    uv = mesh.faces_uvs.clone()
    uv[5] = uv[5, 0]
    tex, owner = tb.bake_field_texture(TB.analytic_fn, TensorMesh(mesh.vertices, mesh.faces, uv), 64, 4,
                                       return_owner=True)
    assert not bool((owner == 5).any()) and bool(torch.isfinite(tex).all())
