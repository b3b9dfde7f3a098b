"""Exact mesh crossings (volsurfs_amd.mesh_intersect, csrc/mesh_cross.hip): do the shells the pipeline
makes cross, and what does it cost to know -- in one process on one GPU.

Workloads:
  lobed   K = 5 level sets of the noisy lobed SDF of tools/simplify_bench.py on an n^3 grid at the reference's
          delta_surfs = 0.0025, each simplified to 0.025 of its faces (the shells tools/visibility_bench.py builds), one
          device-built tracer: `shell_crossings` over the four consecutive pairs (count passes only), `self_crossings`
          of each shell (count, read, emit, sort), and `mesh_crossings` of every consecutive pair.
  sphere  the unsimplified n^3 sphere shell against its neighbour level: `mesh_crossings` with segments.

Baselines, on the same meshes:
  torch   the same rule, operation for operation, as a chunked brute force over all pairs in torch float64 on the same
          GPU.  lobed: every pair of shells and every shell against itself, the pairs asserted equal to the device's.
          sphere: all pairs are out of reach (F^2 ~ 10^11), so the first --subset query faces against all of the
          neighbour, asserted equal to that prefix of the device's pairs; its time is also given per face pair.
  numpy   the restatement of tests/mesh_intersect_restated.py on the host, on the first --subset query faces of shell 0
          against shell 1 (all pairs would take minutes per pair of shells), asserted equal to the device's prefix;
          time per face pair.

Timed --reps times after a warm-up, host clock around calls that end in a device synchronise (every call here ends in
a blocking read), min / median / max in ms.  No speed threshold is a pass condition.  Needs a GPU; writes one JSON file.

    python tools/mesh_intersect_bench.py [--out profiles/mesh_intersect.json] [--n 512] [--reps 10] [--subset 256]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, DELTA, RATIO = 5, 0.0025, 0.025


def _timed(fn, reps):
    import torch
    fn()                                                    # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def _orient(a, b, c, d):
    px, py, pz = a[..., 0] - d[..., 0], a[..., 1] - d[..., 1], a[..., 2] - d[..., 2]
    qx, qy, qz = b[..., 0] - d[..., 0], b[..., 1] - d[..., 1], b[..., 2] - d[..., 2]
    rx, ry, rz = c[..., 0] - d[..., 0], c[..., 1] - d[..., 1], c[..., 2] - d[..., 2]
    m0 = qy * rz - qz * ry
    m1 = qx * rz - qz * rx
    m2 = qx * ry - qy * rx
    return (px * m0 - py * m1) + pz * m2


def _torch_crosses(A, B):
    """bool [a, b]: the rule on triangles A [a, 1, 3, 3] and B [1, b, 3, 3] (float64), every determinant computed."""
    def opposite(s, t):
        return ((s < 0) & (t > 0)) | ((s > 0) & (t < 0))

    def one_sign(x, y, z):
        return ((x >= 0) & (y >= 0) & (z >= 0)) | ((x <= 0) & (y <= 0) & (z <= 0))

    sB = [_orient(B[..., 0, :], B[..., 1, :], B[..., 2, :], A[..., i, :]) for i in range(3)]
    sA = [_orient(A[..., 0, :], A[..., 1, :], A[..., 2, :], B[..., j, :]) for j in range(3)]
    numbers = sA[0] == sA[0]
    for s in sA[1:] + sB:
        numbers = numbers & (s == s)
    e = [[_orient(A[..., i, :], A[..., (i + 1) % 3, :], B[..., j, :], B[..., (j + 1) % 3, :]) for j in range(3)]
         for i in range(3)]
    out = None
    for i in range(3):
        pa = opposite(sB[i], sB[(i + 1) % 3]) & one_sign(e[i][0], e[i][1], e[i][2])
        pb = opposite(sA[i], sA[(i + 1) % 3]) & one_sign(e[0][i], e[1][i], e[2][i])
        out = pa | pb if out is None else out | pa | pb
    return out & numbers


def _torch_pairs(a, b, chunk, self_mode=False, nr_query=None):
    """[P, 2] int64, sorted: the crossing pairs of meshes a and b by brute force (self_mode: a is b, pairs i < j)."""
    import torch
    A = a.vertices.double()[a.faces.long()]
    B = b.vertices.double()[b.faces.long()]
    if nr_query is not None:
        A = A[:nr_query]
    out = []
    for lo in range(0, A.shape[0], chunk):
        m = _torch_crosses(A[lo:lo + chunk, None], B[None])
        ij = m.nonzero()
        ij[:, 0] += lo
        out.append(ij[ij[:, 1] > ij[:, 0]] if self_mode else ij)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_intersect.json"))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--subset", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=128)
    a = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("mesh_intersect_bench needs a GPU")
    import mesh_intersect_restated as R
    from tools.simplify_bench import _fields
    from volsurfs_amd import isosurface as iso, mesh_intersect as MI
    from volsurfs_amd.mesh import TensorMesh
    from volsurfs_amd.raytrace import RayTracer
    from volsurfs_amd.simplify import simplify_mesh

    result = {"device": torch.cuda.get_device_name(0), "grid": a.n, "reps": a.reps, "subset": a.subset}

    def prefix(mesh, n):
        return TensorMesh(mesh.vertices, mesh.faces[:n].contiguous(), device="cuda")

    # ---- lobed: the five simplified shells
    meshes, _ = iso.extract_level_sets(_fields()["lobed_noisy"], a.n, K, delta_surfs=DELTA)
    meshes = [simplify_mesh(m, RATIO) for m in meshes]
    tracer = RayTracer(meshes, builder="device")
    lobed = {"faces": [int(m.faces.shape[0]) for m in meshes], "tree_depth": tracer.max_depth}
    lobed["shell_crossings"] = MI.shell_crossings(tracer)
    lobed["shell_crossings_ms"] = _timed(lambda: MI.shell_crossings(tracer), a.reps)
    lobed["nested"] = MI.shells_nested(tracer)
    selfs = [MI.self_crossings((tracer, k)) for k in range(K)]
    lobed["self_crossings"] = [int(s.pairs.shape[0]) for s in selfs]
    lobed["self_crossing_faces"] = [int((s.count > 0).sum()) for s in selfs]
    lobed["self_crossings_ms"] = _timed(lambda: [MI.self_crossings((tracer, k)) for k in range(K)], a.reps)
    between = [MI.mesh_crossings((tracer, k), (tracer, k + 1), segments=True) for k in range(K - 1)]
    lobed["crossing_length"] = [c.length() for c in between]
    lobed["mesh_crossings_ms"] = _timed(
        lambda: [MI.mesh_crossings((tracer, k), (tracer, k + 1), segments=True) for k in range(K - 1)], a.reps)
    # torch brute force: the same pairs
    ref_between = [_torch_pairs(meshes[k], meshes[k + 1], a.chunk) for k in range(K - 1)]
    ref_self = [_torch_pairs(meshes[k], meshes[k], a.chunk, self_mode=True) for k in range(K)]
    for k in range(K - 1):
        assert torch.equal(ref_between[k], between[k].pairs), f"shells {k}, {k + 1}: torch brute force differs"
    for k in range(K):
        assert torch.equal(ref_self[k], selfs[k].pairs), f"shell {k}: torch brute force differs (self)"
    lobed["equal_to_torch_brute_force"] = True
    reps = max(1, min(a.reps, 2))
    lobed["torch_between_ms"] = _timed(
        lambda: [_torch_pairs(meshes[k], meshes[k + 1], a.chunk) for k in range(K - 1)], reps)
    lobed["torch_self_ms"] = _timed(
        lambda: [_torch_pairs(meshes[k], meshes[k], a.chunk, self_mode=True) for k in range(K)], reps)
    lobed["torch_over_device_between"] = round(lobed["torch_between_ms"]["median"] / lobed["mesh_crossings_ms"]["median"], 1)
    lobed["torch_over_device_self"] = round(lobed["torch_self_ms"]["median"] / lobed["self_crossings_ms"]["median"], 1)
    # numpy on the host: a prefix of shell 0 against shell 1
    v0, f0 = meshes[0].vertices.cpu().numpy(), meshes[0].faces.cpu().numpy()
    v1, f1 = meshes[1].vertices.cpu().numpy(), meshes[1].faces.cpu().numpy()
    t0 = time.perf_counter()
    ref = R.mesh_crossings(v0, f0[:a.subset], v1, f1)
    numpy_s = time.perf_counter() - t0
    got = MI.mesh_crossings(prefix(meshes[0], a.subset), (tracer, 1), segments=True)
    assert np.array_equal(got.pairs.cpu().numpy(), ref["pairs"]), "numpy restatement differs (pairs)"
    assert np.array_equal(got.segments.cpu().numpy(), ref["segments"]), "numpy restatement differs (segments)"
    face_pairs = min(a.subset, len(f0)) * len(f1)
    full = len(f0) * len(f1)
    device_ns = 1e6 * lobed["mesh_crossings_ms"]["median"] / sum(
        lobed["faces"][k] * lobed["faces"][k + 1] for k in range(K - 1))
    lobed["numpy"] = {"query_faces": min(a.subset, len(f0)), "seconds": round(numpy_s, 3),
                      "ns_per_face_pair": round(1e9 * numpy_s / face_pairs, 3),
                      "seconds_for_all_of_shell_0_extrapolated": round(numpy_s * full / face_pairs, 1),
                      "device_ns_per_face_pair": round(device_ns, 6), "equal_pairs_and_segments": True}
    result["lobed"] = lobed
    del tracer, selfs, between, ref_between, ref_self

    # ---- sphere: an unsimplified shell against its neighbour level
    spheres, _ = iso.extract_level_sets(_fields()["sphere"], a.n, 2, delta_surfs=DELTA)
    tracer = RayTracer(spheres, builder="device")
    sphere = {"faces": [int(m.faces.shape[0]) for m in spheres], "tree_depth": tracer.max_depth}
    res = MI.mesh_crossings((tracer, 0), (tracer, 1), segments=True)
    sphere["pairs"] = int(res.pairs.shape[0])
    sphere["mesh_crossings_ms"] = _timed(lambda: MI.mesh_crossings((tracer, 0), (tracer, 1), segments=True), a.reps)
    sphere["crossing_stats_ms"] = _timed(lambda: MI.crossing_stats((tracer, 0), (tracer, 1)), a.reps)
    sphere["self_crossings"] = int(MI.self_crossings((tracer, 0)).pairs.shape[0])
    sphere["self_crossings_ms"] = _timed(lambda: MI.self_crossings((tracer, 0)), a.reps)
    n = min(4 * a.subset, sphere["faces"][0])
    chunk = max(1, min(a.chunk, (1 << 22) // sphere["faces"][1]))
    want = _torch_pairs(spheres[0], spheres[1], chunk, nr_query=n)
    assert torch.equal(want, res.pairs[res.pairs[:, 0] < n]), "sphere: torch brute force differs on the prefix"
    t = _timed(lambda: _torch_pairs(spheres[0], spheres[1], chunk, nr_query=n), 1)
    sphere["torch_prefix"] = {"query_faces": n, "ms": t["median"], "equal_pairs": True,
                              "ns_per_face_pair": round(1e6 * t["median"] / (n * sphere["faces"][1]), 6),
                              "device_ns_per_face_pair": round(
                                  1e6 * sphere["mesh_crossings_ms"]["median"] / (sphere["faces"][0] * sphere["faces"][1]), 9)}
    result["sphere"] = sphere

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
