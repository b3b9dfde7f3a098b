"""The rules of the texture bake (include/volsurfs_hip.h, "texture bake") restated in plain torch / numpy for any device,
written from the behaviour of volsurfs_py/utils/texture_extraction.py: the per-face loop with its sampling, ownership
and mean rule (`bake_restated`), the counter-based jitter (`uniform`), the dilation rule (`dilate_restated`), and the
fixture's mesh and analytic appearance callable, which tools/make_texture_bake_golden.py hands to the reference's own
functions.  Not collected by pytest."""
import numpy as np
import torch

_M, _INC, _U64 = 0x5851f42d4c957f2d, 1442695040888963407, (1 << 64) - 1


def _i64(x):
    x &= _U64
    return x - (1 << 64) if x >= (1 << 63) else x


def _shr(h, k):
    """Logical shift right of an int64 tensor holding 64 unsigned bits."""
    return (h >> k) & ((1 << (64 - k)) - 1)


def uniform(seed, face, texel, S, s, axis):
    """r(seed, face, texel, s, axis) in [0, 1) as float32; `texel` an int64 tensor, the rest ints.  int64 products
    wrap, which is the unsigned 64-bit arithmetic of the rule."""
    h0 = ((int(seed) + int(face) + 1) * _M) & _U64
    h0 ^= h0 >> 32
    h = (texel * S + s) * 2 + axis + _i64(h0 + 1)
    h = h * _M
    h = h ^ _shr(h, 32)
    h = h * _M + _i64(_INC)
    x = _shr(_shr(h, 18) ^ h, 27) & 0xFFFFFFFF
    k = _shr(h, 59)
    o = ((x >> k) | (x << ((32 - k) & 31))) & 0xFFFFFFFF
    bits = ((o >> 9) | 0x3F800000).to(torch.int32)
    return bits.view(torch.float32) - 1.0


def face_box(uv, R):
    """[x0, x1) x [y0, y1) of a face's corner UVs (numpy float32 [3, 2])."""
    fR = np.float32(R)
    lo, hi = uv.min(0) * fR, uv.max(0) * fR
    clip = lambda v: int(min(max(v, 0), R))
    return clip(np.floor(lo[0])), clip(np.ceil(hi[0])), clip(np.floor(lo[1])), clip(np.ceil(hi[1]))


@torch.no_grad()
def bake_restated(fn, vertices, faces, faces_uvs, R, S=1, seed=0, nr_channels=None, torch_normal=False):
    """-> (texture [R, R, C], owner [R, R] int32).  Faces in ascending order, each writing over the last; per face the
    texels of its UV box, S samples each (sample 0 the centre), the model on every sample, the mean over the inside
    ones summed in sample order.  Divisions by R are by a tensor, not a Python scalar: torch turns a division by a
    scalar into a multiplication by its reciprocal on the GPU.  torch_normal: the face normal through torch's own
    `cross` and `F.normalize`, as the reference calls them, instead of the rule's written-out operations (torch's CPU
    `cross` contracts a b - c d into a fused multiply-add, so the two differ in the last bit on some faces)."""
    dev = vertices.device
    uv_np = faces_uvs.detach().cpu().numpy().astype(np.float32)
    Rt = torch.tensor(float(R), dtype=torch.float32, device=dev)
    half = float(np.float32(1.0 / (2.0 * R)))
    texture, owner = None, torch.full((R, R), -1, dtype=torch.int32, device=dev)
    for f in range(int(faces.shape[0])):
        x0, x1, y0, y1 = face_box(uv_np[f], R)
        if x1 <= x0 or y1 <= y0:
            continue
        IX, IY = torch.meshgrid(torch.arange(x0, x1, device=dev), torch.arange(y0, y1, device=dev), indexing="ij")
        IX, IY = IX.reshape(-1), IY.reshape(-1)
        p1, p2, p3 = faces_uvs[f, 0], faces_uvs[f, 1], faces_uvs[f, 2]
        v0, v1 = p3 - p1, p2 - p1
        dot00 = v0[0] * v0[0] + v0[1] * v0[1]
        dot01 = v0[0] * v1[0] + v0[1] * v1[1]
        dot11 = v1[0] * v1[0] + v1[1] * v1[1]
        denom = dot00 * dot11 - dot01 * dot01
        if float(denom) == 0.0 or not np.isfinite(float(denom)):
            continue
        inv = 1.0 / denom
        A, B, C = (vertices[int(i)] for i in faces[f])
        e1, e2 = B - A, C - A
        n = torch.stack([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
        n = n / torch.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]).clamp_min(1e-12)
        if torch_normal:
            n = torch.nn.functional.normalize(torch.linalg.cross(e1, e2), p=2, dim=-1)
        cx, cy = IX.float() / Rt + half, IY.float() / Rt + half
        texel = IX * R + IY
        total, count = None, torch.zeros(IX.shape[0], dtype=torch.int32, device=dev)
        for s in range(S):
            px, py = cx, cy
            if s > 0:
                px = cx + ((uniform(seed, f, texel, S, s, 0) - 0.5) - 1e-6) / Rt
                py = cy + ((uniform(seed, f, texel, S, s, 1) - 0.5) - 1e-6) / Rt
            v2x, v2y = px - p1[0], py - p1[1]
            dot02 = v0[0] * v2x + v0[1] * v2y
            dot12 = v1[0] * v2x + v1[1] * v2y
            b2 = (dot11 * dot02 - dot01 * dot12) * inv
            b1 = (dot00 * dot12 - dot01 * dot02) * inv
            b0 = (1.0 - b1) - b2
            inside = (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & ((((b0 + b1) + b2) - 1.0).abs() < 1e-6)
            pts = (b0[:, None] * A + b1[:, None] * B) + b2[:, None] * C
            vals = fn(pts, n.expand(pts.shape[0], 3).contiguous())
            first = inside & (count == 0)
            if total is None:
                total = torch.zeros_like(vals)
            total = torch.where(first[:, None], vals, torch.where(inside[:, None], total + vals, total))
            count = count + inside.to(torch.int32)
        cov = count > 0
        if texture is None:
            texture = torch.zeros(R, R, total.shape[1], dtype=torch.float32, device=dev)
        mean = total / count.clamp_min(1).to(torch.float32)[:, None]
        texture[IX[cov], IY[cov]] = mean[cov]
        owner[IX[cov], IY[cov]] = f
    if texture is None:
        texture = torch.zeros(R, R, int(nr_channels), dtype=torch.float32, device=dev)
    return texture, owner


_OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def dilate_restated(img, nr_iterations):
    """The dilation rule in numpy: iteration i fills every empty pixel (all channels 0) that has, among its 8
    neighbours, a pixel filled in iteration i - 1 (iteration 1: a full pixel, no channel 0), from the first such
    neighbour in the order of _OFFSETS; stops when an iteration fills nothing."""
    out = np.array(img, copy=True)
    H, W = out.shape[:2]
    stamp = np.where((out != 0).all(2), 0, np.where((out == 0).all(2), -1, -2))
    for it in range(1, int(nr_iterations) + 1):
        src = np.pad(stamp == it - 1, 1)
        todo = stamp == -1
        pick = np.full((H, W), -1)
        for k in range(7, -1, -1):
            dr, dc = _OFFSETS[k]
            pick[src[1 + dr:1 + dr + H, 1 + dc:1 + dc + W] & todo] = k
        rr, cc = np.nonzero(pick >= 0)
        if rr.size == 0:
            break
        off = np.asarray(_OFFSETS)[pick[rr, cc]]
        out[rr, cc] = out[rr + off[:, 0], cc + off[:, 1]]
        stamp[rr, cc] = it
    return out


# ---- the fixture's mesh and appearance callable

def fixture_mesh():
    """icosphere(2, 0.4) with per-corner octahedral UVs, the faces that straddle the octahedral fold (UV extent > 0.3
    on an axis) dropped, UVs mapped by u * 0.9137 + 0.0421, un-welded to 3 F vertices -> (vertices [3F, 3], faces
    [F, 3] = 0 .. 3F - 1, per-vertex uvs [3F, 2]) as float64 / int64 numpy arrays."""
    from volsurfs_amd.mesh import icosphere, octahedral_uv
    v, f = icosphere(2, 0.4)
    v64 = v.astype(np.float64)
    uv = octahedral_uv(v64 / np.linalg.norm(v64, axis=1, keepdims=True))[f]
    keep = ((uv.max(1) - uv.min(1)) <= 0.3).all(1)
    uv = (uv[keep] * 0.9137 + 0.0421).astype(np.float32).astype(np.float64)
    verts = v64[f[keep]].reshape(-1, 3)
    return verts, np.arange(verts.shape[0], dtype=np.int64).reshape(-1, 3), uv.reshape(-1, 2)


class AnalyticAppearance:
    """8 channels, smooth in the point, linear in the normal, never 0 on the fixture's mesh; the call signature of
    models.ColorSH.  float64 points are computed in float64 and returned as float32."""
    out_channels = 8
    # per-channel Lipschitz constants in the point on |p| <= 0.4 (the normal is constant on a face)
    LIPSCHITZ = (3.0, 2.0, 0.5, 0.0, 0.0, 0.0, 0.4, 3.0 ** 0.5)

    def __call__(self, points, samples_dirs=None, normals=None, iter_nr=None):
        x, y, z = points[:, 0:1], points[:, 1:2], points[:, 2:3]
        out = torch.cat([torch.sin(3.0 * x + 0.3) + 1.5, torch.cos(2.0 * y) + 1.7, z * 0.5 + 2.0,
                         normals.to(points.dtype) * 0.25 + 1.0, x * y + 2.0, torch.sin((x + y) + z) + 1.5], 1)
        return out.float()


def analytic_fn(points, normals):
    return AnalyticAppearance()(points, normals=normals)


def synthetic_dilation_image():
    """[40, 40, 3] float32: isolated full pixels, a pixel with one zero channel, full pixels on the border and in a
    corner, and pairs of sources that compete for one empty pixel from several directions."""
    g = np.random.default_rng(11)
    img = np.zeros((40, 40, 3), np.float32)
    val = lambda: g.uniform(0.5, 2.0, 3).astype(np.float32)
    for r, c in ((5, 5), (20, 31), (33, 12)):                       # isolated
        img[r, c] = val()
    img[12, 12] = val()
    img[12, 13] = (0.7, 0.0, 1.1)                                   # one zero channel: neither source nor destination
    for r, c in ((0, 17), (39, 8), (22, 0), (9, 39), (0, 0), (39, 39)):   # border and corners
        img[r, c] = val()
    for (r0, c0), (r1, c1) in (((26, 20), (26, 22)), ((28, 26), (30, 26)), ((15, 24), (17, 26)), ((15, 32), (17, 30)),
                               ((34, 30), (35, 32)), ((3, 28), (5, 29))):   # two sources, one empty pixel between
        img[r0, c0], img[r1, c1] = val(), val()
    return img
