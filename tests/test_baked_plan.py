"""The checks and the byte layout that every stage consuming a baked 8-bit bank shares (csrc/nt_common.h
`nt_baked_plan_args` / `nt_baked_plan_supported` / `nt_plane_layout`, `texture_export.plane_layout`).
Nothing here needs a GPU: host buffers stand in as "device" pointers, and every call returns before it reads one."""
import ctypes
import itertools

ERR_ARG, ERR_UNSUPPORTED = -1, -2
MAX_SHELLS, MAX_RES = 16, 16384

# one way to break a plan each: (field, index or None, value)
ARG_FAULTS = {"shells=0": ("nr_shells", None, 0), "shells=max+1": ("nr_shells", None, MAX_SHELLS + 1),
              "degrees=0": ("rgb_degrees", None, 0), "degrees=5": ("rgb_degrees", None, 5),
              "res=0": ("tex_res", 1, 0), "res=max+1": ("tex_res", 0, MAX_RES + 1)}
UNSUPPORTED_FAULTS = {"row_format=1": ("row_format", None, 1), "alpha!=rgb": ("alpha_degrees", None, 1)}
ENTRIES = ("vsa_nt_planes_bytes", "vsa_nt_export_planes", "vsa_nt_import_planes", "vsa_texel_fit_state_bytes",
           "vsa_texel_fit_init", "vsa_texel_fit_step", "vsa_textransfer_planes")

A, U = ERR_ARG, ERR_UNSUPPORTED
# The status of every entry (ENTRIES' order) for every broken plan, recorded from the library as it was built BEFORE the
# checks were written once (the commit "Refit baked textures to target views").  The stages do not agree on precedence:
# texture_io and texture_transfer look at row_format / alpha_degrees before they look at tex_res, texel_fit after.
# How it was recorded, and how to record it again: check that commit out, `make -C volsurfs_amd/csrc`, copy this file
# into its tests/ and run `python tests/test_baked_plan.py`: it prints the table below from whichever library is built
# (nothing in it reads this table).
PARENTS = {
    "shells=0":                  (A, A, A, A, A, A, A),
    "shells=max+1":              (A, A, A, A, A, A, A),
    "degrees=0":                 (A, A, A, A, A, A, A),
    "degrees=5":                 (A, A, A, A, A, A, A),
    "res=0":                     (A, A, A, A, A, A, A),
    "res=max+1":                 (A, A, A, A, A, A, A),
    "row_format=1":              (U, U, U, U, U, U, U),
    "alpha!=rgb":                (U, U, U, U, U, U, U),
    "shells=0 + row_format=1":   (A, A, A, A, A, A, A),
    "shells=0 + alpha!=rgb":     (A, A, A, A, A, A, A),
    "shells=max+1 + row_format=1": (A, A, A, A, A, A, A),
    "shells=max+1 + alpha!=rgb": (A, A, A, A, A, A, A),
    "degrees=0 + row_format=1":  (A, A, A, A, A, A, A),
    "degrees=0 + alpha!=rgb":    (A, A, A, A, A, A, A),
    "degrees=5 + row_format=1":  (A, A, A, A, A, A, A),
    "degrees=5 + alpha!=rgb":    (A, A, A, A, A, A, A),
    "res=0 + row_format=1":      (U, U, U, A, A, A, U),
    "res=0 + alpha!=rgb":        (U, U, U, A, A, A, U),
    "res=max+1 + row_format=1":  (U, U, U, A, A, A, U),
    "res=max+1 + alpha!=rgb":    (U, U, U, A, A, A, U),
}


def _broken_plans():
    """{name: faults} for each fault alone and each ARG fault paired with each UNSUPPORTED fault."""
    out = {k: [v] for k, v in itertools.chain(ARG_FAULTS.items(), UNSUPPORTED_FAULTS.items())}
    for (ka, va), (ku, vu) in itertools.product(ARG_FAULTS.items(), UNSUPPORTED_FAULTS.items()):
        out[f"{ka} + {ku}"] = [va, vu]
    return out


def _statuses(faults):
    """What each of ENTRIES returns for a good two-degree plan of one shell with `faults` applied; every other argument
    is good (16-byte aligned addresses of a host buffer nothing reads, exact byte counts)."""
    from volsurfs_amd import _lib
    from volsurfs_amd.neural_textures import Plan
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    a16 = (ctypes.addressof(buf) + 15) & ~15
    plan = Plan()
    plan.nr_shells, plan.rgb_degrees, plan.alpha_degrees = 1, 2, 2
    plan.tex_res[0], plan.tex_res[1] = 8, 8
    plan.row_base[len(plan.row_base) - 1] = 24
    for field, index, value in faults:
        if index is None:
            setattr(plan, field, value)
        else:
            getattr(plan, field)[index] = value
    ref = ctypes.byref(plan)
    nbytes = 4 * 8 * 8 * 4
    res = (ctypes.c_int32 * 4)(8, 8, 8, 8)
    roots, frames = (ctypes.c_int32 * 1)(0), (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    base1 = (ctypes.c_longlong * 2)(0, 4)
    need = L.vsa_textransfer_workspace_bytes(1, 8)
    return (L.vsa_nt_planes_bytes(ref),
            L.vsa_nt_export_planes(ref, a16, a16, a16, a16, nbytes, None),
            L.vsa_nt_import_planes(ref, a16, nbytes, a16, a16, a16, None),
            L.vsa_texel_fit_state_bytes(ref),
            L.vsa_texel_fit_init(ref, a16, a16, a16, a16, a16 + 16, a16 + 32, None),
            L.vsa_texel_fit_step(ref, a16, a16, a16, 1.0, a16, a16 + 16, a16 + 32, a16, 0.01, 0.9, 0.99, 1e-15, 1, a16,
                                 None),
            L.vsa_textransfer_planes(ref, 0, a16, nbytes, a16, a16, roots, frames, 1, 10, a16, a16, a16, base1, res, 1,
                                     1.0, a16, need, a16, nbytes, a16, None))


def test_baked_plan_statuses_are_the_parents():
    plans = _broken_plans()
    assert set(plans) == set(PARENTS) and len(plans) == 20
    for name, faults in plans.items():
        got = _statuses(faults)
        assert got == PARENTS[name], (name, dict(zip(ENTRIES, got)))


def test_plane_layout_totals_are_the_librarys():
    """`plane_layout`'s total is `vsa_nt_planes_bytes` (host only) for K in {1, 3}, D in 1..4 and per-degree
    resolutions that differ; the offsets are the running sum in (shell, degree) order."""
    from volsurfs_amd import _lib
    from volsurfs_amd.neural_textures import Plan
    from volsurfs_amd.texture_export import plane_layout
    L = _lib.lib()
    for K in (1, 3):
        for D in (1, 2, 3, 4):
            for res in ((5, 8, 3, 1), (1, 2, 16, 7)):
                plan = Plan()
                plan.nr_shells, plan.rgb_degrees, plan.alpha_degrees = K, D, D
                for d in range(4):
                    plan.tex_res[d] = res[d]
                layout, total = plane_layout(res, K, D)
                assert total == L.vsa_nt_planes_bytes(ctypes.byref(plan)), (K, D, res)
                assert [(s, d) for s, d, _, _, _ in layout] == [(s, d) for s in range(K) for d in range(D)]
                off = 0
                for s, d, o, n, R in layout:
                    assert (o, n, R) == (off, 2 * d + 1, res[d])
                    off += n * R * R * 4
                assert off == total


if __name__ == "__main__":          # print the table of the library that is built (see PARENTS)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    letter = {ERR_ARG: "A", ERR_UNSUPPORTED: "U"}
    for name, faults in _broken_plans().items():
        row = ", ".join(letter.get(s, str(s)) for s in _statuses(faults))
        print("    %-30s (%s)," % ('"' + name + '":', row))
