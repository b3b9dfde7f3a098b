#!/usr/bin/env python3
"""Generate tests/golden/texture_bake.npz by running the REFERENCE's own `extract_texture_from_color_model` and
`dilate_texture` (volsurfs_py/utils/texture_extraction.py, imported in place through tools/ref_import.py) on the CPU.

Runs only in the build container (it needs the reference tree); only arrays go into the fixture.  The mesh, the
analytic appearance callable and the synthetic dilation image are those of tests/texture_bake_restated.py.
  * the S = 1 bake (no random numbers) at R = 32, 48, 64 in float32 -> tex_R; the same with float64 vertices and UVs
    gives the coverage flips and the largest value difference, printed and stored (flips_R, maxdiff_R);
  * dilate_texture of the R = 64 texture at 5 and 50 iterations, and of the synthetic image at 1, 2, 5, 50.
Usage:  python tools/make_texture_bake_golden.py"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

import ref_import  # noqa: E402
import texture_bake_restated as TB  # noqa: E402

RESOLUTIONS = (32, 48, 64)


def main():
    ref_import.install_placeholders()
    from volsurfs_py.utils.texture_extraction import dilate_texture, extract_texture_from_color_model
    verts, faces, uvs = TB.fixture_mesh()
    model = TB.AnalyticAppearance()
    arrs = {"vertices": verts.astype(np.float32), "faces": faces.astype(np.int32), "uvs": uvs.astype(np.float32)}
    f = torch.from_numpy(faces)
    for R in RESOLUTIONS:
        out = {}
        for dt in (torch.float32, torch.float64):
            out[dt] = extract_texture_from_color_model(model, torch.from_numpy(verts).to(dt), f,
                                                       torch.from_numpy(uvs).to(dt), texture_res=R,
                                                       nr_samples_per_texel=1).numpy()
        t32, t64 = out[torch.float32], out[torch.float64]
        c32, c64 = (t32 != 0).all(2), (t64 != 0).all(2)
        flips = int((c32 != c64).sum())
        both = c32 & c64
        maxdiff = float(np.abs(t32.astype(np.float64) - t64)[both].max())
        print(f"R = {R}: {int(c32.sum())} covered texels, {flips} flips float32 / float64, max value difference "
              f"{maxdiff:.2e}")
        arrs[f"tex_{R}"], arrs[f"flips_{R}"], arrs[f"maxdiff_{R}"] = t32, np.int64(flips), np.float64(maxdiff)
    syn = TB.synthetic_dilation_image()
    arrs["syn"] = syn
    with contextlib.redirect_stdout(io.StringIO()):
        for n in (5, 50):
            arrs[f"tex_64_dilated_{n}"] = dilate_texture(arrs["tex_64"], n)
        for n in (1, 2, 5, 50):
            arrs[f"syn_dilated_{n}"] = dilate_texture(syn, n)
    path = os.path.join(GOLD, "texture_bake.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
