"""bench.py's contract (one JSON line on stdout, the keys the driver reads) for every workload,
at sizes that finish in seconds."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True,
                       text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]          # ONE line on stdout, nothing else (RCCL's banner included)
    return json.loads(lines[0])


def test_kernel_source_hash_guards_the_traffic_file():
    sys.path.insert(0, ROOT)
    import bench
    h = bench.kernel_source_hash()
    assert len(h) == 64 and h == bench.kernel_source_hash()
    tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["workloads"]
    # one collection per workload key (VERDICT r3 weak #12, r4 missing #4): the 1080p K = 7 line quotes its own
    # collection, never the 800x800 K = 5 one; every entry carries the hash of the kernel sources it was taken at
    head = bench.workload_key(bench.parse([]))
    k7 = bench.workload_key(bench.parse(["--res", "1080", "--width", "1920", "--shells", "7", "--subdiv", "8"]))
    assert head in tj and head != k7 and bench.workload_key(bench.parse(["--stress"])) != head
    for entry in tj.values():
        assert "_kernel_source_sha256" in entry and "nt_mlp_bwd" in entry


@pytest.mark.gpu
def test_frame_workload_line():
    d = _run("--res", "128", "--shells", "2", "--subdiv", "3", "--steps", "3", "--warmup", "1",
             "--cpu-sample-rays", "64")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "h", "Mhits/s"):
        assert k in d, k
    assert d["unit"] == "Mrays/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 0
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and "workload" in d["config"]
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["peak"] in (8000.0, 2500.0) and 0 < rf["frac"] < 1
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    assert 0 < d["h"] <= 1
    # the non-ideal scene beside the headline (noisy shells, fragmented uv charts, spread parameters)
    assert d["value_noisy"] > 0 and d["noisy"]["unique_texels_per_frame"] > 0 and 0 < d["noisy"]["h"] <= 1
    assert "charts" in d["noisy"]["scene"] and "perfect spheres" in d["config"]["scene"]
    # the stress scene (non-convex lobed shells, 256 charts, 12x triangle spread) and the figures
    # WITHOUT any inter-frame feedback on a camera that moves every step
    assert d["value_stress"] > 0 and "non-convex" in d["stress"]["scene"] and d["stress"]["hits_per_frame"] > 0
    assert d["value_cold"] > 0 and "VSA_TRACE_FEEDBACK=0" in d["cold"]["regime"] and "orbits" in d["cold"]["regime"]
    assert d["value_stress_cold"] > 0
    assert d["roofline"]["traffic"] is None      # profiles/traffic.json is another workload's (800x800, K = 5)


@pytest.mark.gpu
def test_one_rank_rccl_group_drives_the_data_parallel_schedule():
    """RCCL for real.  `--gpus 1 --force-dist` forms a ONE-rank `nccl` process group
    on the MI355X (init_process_group(device_id=...)) and runs the data-parallel step through it: the
    gradient slices are all-reduced by RCCL shell by shell while backward runs (GradientOverlap)."""
    d = _run("--res", "128", "--shells", "2", "--subdiv", "3", "--steps", "3", "--warmup", "1",
             "--no-cpu-baseline", "--force-dist", "--dist-backend", "nccl")
    assert d["n_gpus"] == 1 and d["ranks_seen"] == 1 and d["dist_backend"] == "nccl" and d["value"] > 0
    # r5: the data-parallel step is the one-GPU graph + device flags; the collectives run beside it
    assert "grad_allreduce" in d["stages_ms"] and d["config"]["launch"] == "hip-graph replay"
    # r6: the phase split is chosen from times measured on this group's wire — a one-rank group's all-reduce hides behind
    # the next step's head, so ONE phase (the schedule then costs what the plain step costs) — and every rank's reduced
    # gradients are checksummed into the line (the first multi-GPU run validates its own collectives)
    assert d["config"]["dp_phases"] == [2] and d["config"]["dp_phases_chosen_from"]["t_comm_ms"] >= 0
    assert d["grad_checksums_equal"] is True and len(d["grad_checksum_per_rank"]) == 1
    assert d["grad_checksum_per_rank"][0][1] > 0 and d["grad_checksum_per_rank"][0][3] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["train", "train-permuto"])
def test_training_workload_lines(workload):
    d = _run("--workload", workload, "--res", "128", "--views", "3", "--shells", "2", "--subdiv", "3",
             "--steps", "6", "--warmup", "3", "--target-hits", "4096")
    assert d["unit"] == "it/s" and d["value"] > 0 and d["steps"] == 6
    assert d["hits_per_iter"] > 0 and d["rays_per_iter"] > 0 and 0 < d["fixed_share"]
    assert "workload" in d["config"] and d["config"]["parameters"] > 0


@pytest.mark.gpu
def test_render_workload_line():
    d = _run("--workload", "render", "--res", "128", "--shells", "2", "--subdiv", "3", "--steps", "3", "--warmup", "1")
    assert d["unit"] == "Mrays/s" and d["value"] > 0 and d["baked"]["Mrays/s"] > 0


def test_dump_outputs_writes_float32_within_budget_and_samples_the_same_entries(tmp_path):
    """bench.dump_outputs on host tensors: small arrays whole, an array over its share of the 64 MB budget as a
    sample whose entries are the same on every call (two builds are compared file for file)."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    small = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    big = torch.arange(10 << 20, dtype=torch.float32).reshape(-1, 2)       # 40 MB, every entry its own index
    files = {}
    for d in ("a", "b"):
        files[d] = bench.dump_outputs(str(tmp_path / d), {"rgb": small, "tables_grad": big})
    assert files["a"] == files["b"] and set(files["a"]) == {"rgb.npy", "tables_grad_sample.npy"}
    assert files["a"]["rgb.npy"] == [4, 3]
    total = 0
    for name in files["a"]:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += a.nbytes
    assert total <= bench.DUMP_BYTES
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "rgb.npy"), small.numpy())
    s = np.load(tmp_path / "a" / "tables_grad_sample.npy")
    # distinct entries of the flattened array, in index order
    assert s.size == bench.DUMP_BYTES // 2 // 4 and (np.diff(s) > 0).all() and 0 <= s[0] and s[-1] < big.numel()
    assert (tmp_path / "a" / ".gitignore").read_text() == "*\n"


def test_steps_and_dump_outputs_arguments_are_checked():
    for argv in (["--steps", "0"], ["--workload", "train", "--dump-outputs", "x"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                           timeout=120, cwd=ROOT)
        assert r.returncode == 2 and r.stdout.strip() == "", argv


@pytest.mark.gpu
def test_frame_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    """--dump-outputs: the last timed step's colours and gradients; the same arguments give the same inputs, so two
    runs give the same colours (no float atomics in the forward) and the same gradients up to summation order."""
    import numpy as np
    args = ("--res", "128", "--shells", "2", "--subdiv", "3", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
            "--no-noisy")
    runs = [_run(*args, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    assert runs[0]["steps"] == 3 and runs[0]["ms_per_step"] > 0
    files = runs[0]["dumped_outputs"]["files"]
    assert files == runs[1]["dumped_outputs"]["files"]
    assert set(files) == {"rgb.npy", "weights_grad.npy", "tables_grad_sample.npy"} and files["rgb.npy"] == [128 * 128, 3]
    total = 0
    for name in files:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and list(a.shape) == files[name] and np.isfinite(a).all()
        total += a.nbytes
        if name == "rgb.npy":
            assert np.array_equal(a, b)
        else:
            # the backward accumulates with atomics in arrival order: measured on MI355X 1.6e-4 of the largest entry
            # (tables.grad); bounded by the gradient tolerance smoke() holds against the oracle
            assert np.abs(a).max() > 0 and np.abs(a - b).max() <= 1e-3 * np.abs(a).max(), name
    assert total <= 64 << 20


def test_world_size_that_contradicts_gpus_is_refused():
    """A launcher that started a different number of ranks than --gpus says: exit non-zero before
    anything touches a GPU (runs on CPU)."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True,
                       text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr and r.stdout.strip() == ""


@pytest.mark.gpu
@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_gpus_flag_launches_the_ranks_itself(scaling):
    """`python bench.py --gpus 2` with no launcher around it starts two ranks (gloo on one device
    here: the pool gives one GPU per box) and reports what the process group really was."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
                        "--single-device", "--scaling", scaling, "--res", "128", "--shells", "2", "--subdiv", "3",
                        "--steps", "3", "--warmup", "1", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["dist_backend"] == "gloo"
    assert d["scaling"] == scaling and d["value"] > 0
    assert d["config"]["global_rays"] == (128 * 128 if scaling == "strong" else 2 * 128 * 128)


@pytest.mark.gpu
def test_data_parallel_training_replicas_stay_one_model():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
                        "--single-device", "--workload", "train-permuto", "--res", "128", "--views", "3",
                        "--shells", "2", "--subdiv", "3", "--steps", "6", "--warmup", "3", "--target-hits", "4096"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.strip()][0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["replicas_in_sync"] is True
