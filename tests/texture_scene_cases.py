"""Scenes shared by tests/test_texture_transfer.py and tests/test_texture_fit.py: a stack of nested icospheres with
atlases, planes of random, constant and smooth bytes, a `BakedScene` of them and a camera."""
import functools

import torch

RADII = (0.5, 0.6, 0.7)
SH_RANGE = (15.0, 12.0, 9.0, 6.0)
RENDER_KEYS = ("rgb", "surfs_rgb", "surfs_alpha", "bg_transmittance")
BG_COLOR = (0.25, 0.5, 1.0)


@functools.lru_cache(maxsize=None)
def stack(subdiv, resolution=64, padding=2, *, K=3):
    """The first K of the nested icospheres (80 faces at subdiv 1, 320 at 2) of radii 0.5 / 0.6 / 0.7 with UVs from
    compute_atlas."""
    from volsurfs_amd.atlas import compute_atlas
    from volsurfs_amd.mesh import TensorMesh, icosphere
    out = []
    for r in RADII[:K]:
        v, f = icosphere(subdiv, r)
        out.append(compute_atlas(TensorMesh(v, f, None), resolution, padding))
    return tuple(out)


def random_planes(K, res, seed, solid=False, no_alpha=False):
    """Random bytes; alpha 255 on every shell (no_alpha) or on the inner one (solid)."""
    g = torch.Generator().manual_seed(seed)
    planes = {}
    for s in range(K):
        for d, R in enumerate(res):
            p = torch.randint(0, 256, (2 * d + 1, R, R, 4), generator=g, dtype=torch.uint8)
            if no_alpha or (solid and s == 0):
                p[..., 3] = 255
            planes[(s, d)] = p.cuda()
    return planes


def constant_byte(s, d, i):
    return (53 * s + 29 * d + 7 * i + 11) % 256


def constant_planes(K, res, solid):
    planes = {}
    for s in range(K):
        for d, R in enumerate(res):
            p = torch.empty(2 * d + 1, R, R, 4, dtype=torch.uint8)
            for i in range(2 * d + 1):
                p[i] = constant_byte(s, d, i)
            if solid and s == 0:
                p[..., 3] = 255
            planes[(s, d)] = p.cuda()
    return planes


def smooth_planes(K, res, seed):
    """Smooth random planes with bytes in 64..191: a coarse random grid, bilinearly enlarged."""
    g = torch.Generator().manual_seed(seed)
    planes = {}
    for s in range(K):
        for d, R in enumerate(res):
            coarse = torch.rand(2 * d + 1, 4, 5, 5, generator=g)
            fine = torch.nn.functional.interpolate(coarse, size=(R, R), mode="bilinear", align_corners=True)
            planes[(s, d)] = (64 + 127 * fine).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
    return planes


def scene(meshes, planes, lerp=True, solid=False, builder="device", *, shared_alpha=False, bg_color=BG_COLOR):
    """A BakedScene of the planes with SH_RANGE's ranges; shared_alpha and bg_color by keyword only."""
    from volsurfs_amd.texture_transfer import scene_from_planes
    D = len({d for _, d in planes})
    return scene_from_planes(meshes, planes, SH_RANGE[:D], inner_solid=solid, shared_alpha=shared_alpha, lerp=lerp,
                             bg_color=bg_color, builder=builder)


def camera(eye, size=64, focal=60.0):
    from volsurfs_amd.camera import Camera
    return Camera.look_at(eye, focal=focal, height=size, width=size)
