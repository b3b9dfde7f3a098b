#!/usr/bin/env python3
"""Generate tests/golden/sphere_trace.npz by running the REFERENCE's own sphere tracing loop
(volsurfs_py/utils/sphere_tracing.py, imported in place through tools/ref_import.py) on the CPU in float32.

Runs only in the build container (it needs the reference tree); only arrays and names go into the fixture.  The
reference's native `RaySampler.init_with_one_sample_per_ray` is replaced by an object with `samples_3d` and
`samples_dirs`; the bounding sphere, the rays and the analytic fields are those of tests/sphere_trace_restated.py.
Per case `<field>_<setting>` (fields: FIXTURE_FIELDS, settings: FIXTURE_SETTINGS) the final points, samples_z and hit
flags, the latter also with unconverged_are_hits.  `--check64` prints, per case, how many hit flags the reference flips
between float32 and float64 and its largest point gap (the numbers that tests/test_sphere_trace.py's bounds rest on).
Usage:  python tools/make_sphere_trace_golden.py [--check64]"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

import ref_import  # noqa: E402
import sphere_trace_restated as R  # noqa: E402


class _OneSamplePerRay:
    @staticmethod
    def init_with_one_sample_per_ray(samples_3d, samples_dirs):
        return SimpleNamespace(samples_3d=samples_3d, samples_dirs=samples_dirs, samples_z=None)


def _reference_loop():
    ref_import.install_placeholders({"volsurfs": {"RaySampler": _OneSamplePerRay},
                                     "matplotlib": {}, "matplotlib.pyplot": {}})
    from volsurfs_py.utils.sphere_tracing import sphere_trace
    return sphere_trace


def main():
    sphere_trace = _reference_loop()
    check64 = "--check64" in sys.argv[1:]
    o, d = R.fixture_rays()
    prim = R.TorchBoundingSphere(R.FIXTURE_RADIUS)
    arrs = {"rays_o": o.numpy(), "rays_d": d.numpy(), "radius": np.float32(R.FIXTURE_RADIUS)}
    for sname, (rounds, thresh) in R.FIXTURE_SETTINGS.items():
        for fname, (fn, surf_idx) in R.FIXTURE_FIELDS.items():
            out = {}
            for dt in (torch.float32, torch.float64) if check64 else (torch.float32,):
                for uah in (False, True):
                    pack, hit = sphere_trace(fn, o.to(dt), d.to(dt), prim, nr_sphere_traces=rounds,
                                             sdf_converged_tresh=thresh, surf_idx=surf_idx, unconverged_are_hits=uah)
                    out[dt, uah] = (pack.samples_3d, pack.samples_z, hit)
            case = f"{fname}_{sname}"
            p, z, hit = out[torch.float32, False]
            arrs[case + "_points"], arrs[case + "_z"], arrs[case + "_hit"] = p.numpy(), z.numpy(), hit.numpy()
            arrs[case + "_hit_unconverged"] = out[torch.float32, True][2].numpy()
            assert torch.equal(out[torch.float32, True][0], p)
            line = f"{case}: {int(hit.sum())} hits of {hit.numel()}, {int(out[torch.float32, True][2].sum())} with " \
                   "unconverged_are_hits"
            if check64:
                p64, _, hit64 = out[torch.float64, False]
                same = hit == hit64
                gap = (p.double() - p64).abs().amax(-1)
                both = same & hit
                line += f"; fp32 / fp64: {int((~same).sum())} flips, point gap {float(gap[both].max()):.2e} on hits, " \
                        f"{float(gap[same & ~hit].max()):.2e} on the other rays with equal flags"
            print(line)
    path = os.path.join(GOLD, "sphere_trace.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
