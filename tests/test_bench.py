"""bench.py's host side on the CPU: every workload's CPU baseline case (the
reference's own loops from oracle/_ref, or the C restatement) runs and sizes
its sample as the GPU line reports it.  No GPU needed."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

WORKLOADS = {"resize_normalize": 1920 * 1080, "resize_normalize_720p": 1920 * 1080, "warp": 1280 * 720, "cvt_normalize": 1920 * 1080,
             "cubic_stats": 2560 * 1440, "yuv_resize": 1920 * 1080}


@pytest.mark.parametrize("workload", sorted(WORKLOADS))
def test_cpu_case_runs(workload):
    import bench
    one, imgs, px, kind, what = bench.cpu_case(workload)
    assert px == WORKLOADS[workload]
    assert kind in ("reference", "port") and what
    out = one(imgs[0])
    assert out is not None


def test_workload_choices_match_parser(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert a.workload == "resize_normalize" and a.gpus == 1 and a.batch == 0
    for w in WORKLOADS:
        monkeypatch.setattr(sys, "argv", ["bench.py", "--workload", w])
        assert bench.parse().workload == w


def test_plain_run_is_the_default(monkeypatch):
    """--full and --dump-outputs are off unless asked for."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_files(monkeypatch, tmp_path):
    """dump_outputs on host tensors: small arrays whole and in shape, u8 as
    float32 (exact), float64 kept; an array over the cap as a sample of its
    flattened values whose indices depend on its size and the seed alone."""
    import json

    import numpy as np
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    big = torch.arange(5000, dtype=torch.float32).reshape(50, 100) * 0.5
    frames = torch.arange(2 * 3 * 4 * 3, dtype=torch.int64).reshape(2, 3, 4, 3).to(torch.uint8)
    sums = torch.tensor([[1.0, 2.0], [3.0, 1e300]], dtype=torch.float64)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"output": big, "frames": frames, "sums": sums})
    a = tmp_path / "a"
    got = np.load(a / "frames.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 4, 3) and np.array_equal(got, frames.numpy())
    got = np.load(a / "sums.npy")
    assert got.dtype == np.float64 and np.array_equal(got, sums.numpy())
    got = np.load(a / "output.npy")
    idx = np.random.default_rng(bench.DUMP_SEED).integers(0, 5000, size=1000, dtype=np.int64)
    assert got.dtype == np.float32 and got.shape == (1000,) and np.array_equal(got, big.numpy().reshape(-1)[idx])
    assert np.array_equal(got, np.load(tmp_path / "b" / "output.npy"))
    m = json.loads((a / "manifest.json").read_text())
    assert m["output"]["shape"] == [50, 100] and m["output"]["sample"]["seed"] == bench.DUMP_SEED
    assert m["frames"]["sample"] is None and m["frames"]["source_dtype"] == "uint8"
    assert sorted(p.name for p in a.iterdir()) == ["frames.npy", "manifest.json", "output.npy", "sums.npy"]


def _run_bench(args, env_extra=None, timeout=240):
    import json
    import os
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK",
                                                                "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, str(REPO / "bench.py")] + args, env=env, capture_output=True,
                       text=True, timeout=timeout)
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    return p.returncode, lines, p.stderr


@pytest.mark.parametrize("workload", ["resize_normalize", "cubic_stats"])
def test_gpus_flag_spawns_ranks(workload):
    """bench.py --gpus 2 with no torchrun environment starts two rank processes
    itself (gloo here, via --dry-run); rank 0 alone prints the line, and the
    rank count comes from the process group, not from the flag."""
    rc, lines, err = _run_bench(["--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1",
                                 "--workload", workload])
    assert rc == 0, err
    assert len(lines) == 1, lines
    out = lines[0]
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2" and out["dry_run"] is True
    assert out["steps"] == 3 and out["warmup"] == 1


def test_gpus_flag_must_match_world_size():
    """Under torchrun the flag and WORLD_SIZE must agree: a mismatch fails
    instead of reporting a 1-GPU number under an N-GPU label."""
    rc, lines, err = _run_bench(["--gpus", "4", "--dry-run", "--steps", "1", "--warmup", "0"],
                                {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert rc != 0 and not lines and "WORLD_SIZE" in err


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["cubic_stats", "warp"])
def test_bench_main_two_ranks_on_one_gpu(workload):
    """bench.py's real world > 1 path -- main() with the kernels, the barriers,
    the shard-size check, cfg5's all-reduce and the MAX-over-ranks merge --
    with two ranks on the box's one GPU: VACV_BENCH_BACKEND=gloo replaces RCCL
    (which needs a GPU per rank).  The parent spawns the ranks before anything
    touches the GPU.  --full: the kernel's own timing (roofline) and the
    global-statistics check are not part of a plain run.  One JSON line, n_gpus 2, dp2, a roofline and a finite
    step time; cfg5's statistics are global (the count covers both shards)."""
    import math
    rc, lines, err = _run_bench(["--gpus", "2", "--workload", workload, "--steps", "3", "--warmup", "1",
                                 "--full", "--no-cpu-baseline"], {"VACV_BENCH_BACKEND": "gloo"}, timeout=300)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    out = lines[0]
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2"
    assert out["config"]["backend"] == "gloo" and out["config"]["global_batch"] == 2 * out["config"]["batch_per_gpu"]
    assert math.isfinite(out["ms_per_step"]) and out["ms_per_step"] > 0
    r = out["roofline"]
    assert r["bound"] == "hbm" and r["kernel_ms"] > 0 and 0 < r["frac"] < 1.2
    assert out["value"] > 0 and out["cpu_baseline"] is None
    if workload == "cubic_stats":
        assert out["global_stats_check"]["ok"], out["global_stats_check"]


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(hip_device, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` run: the headline line
    with ms_per_step for exactly K steps and a roofline, no CPU baseline (that
    is --full's), and --dump-outputs holding what the step computed -- bit for
    bit what the same seeded workload gives in this process."""
    import math

    import numpy as np
    import torch
    rc, lines, err = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                                 "--dump-outputs", str(tmp_path / "dump")], timeout=120)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    out = lines[0]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "Mpixels/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert math.isfinite(out["ms_per_step"]) and out["ms_per_step"] > 0
    # value = frames' pixels / step time; the line rounds ms_per_step to 1e-4 ms and value to 0.01
    want = 2 * 1920 * 1080 / (out["ms_per_step"] / 1e3) / 1e6
    assert abs(out["value"] - want) <= want * 0.5e-4 / (out["ms_per_step"] - 0.5e-4) + 0.01
    assert out["cpu_baseline"] is None and out["roofline"]["kernel_ms"] > 0
    got = np.load(tmp_path / "dump" / "output.npy")
    assert got.dtype == np.float32 and got.shape == (2, 360, 640, 3)

    import bench
    from vacv_amd import ops
    wl = bench.make_workload("resize_normalize", 2, hip_device, 0, 1, ops)
    wl["main"]()
    torch.cuda.synchronize()
    assert np.array_equal(got, wl["outputs"]()["output"].cpu().numpy())


def test_gpus_8_dry_run_single_line():
    """The driver's 8-GPU scaling run, rehearsed on the CPU: `--gpus 8` spawns
    eight ranks (gloo, --dry-run), cfg5's step all-reduces its sums across all
    eight, and rank 0 alone prints one dp8 line."""
    rc, lines, err = _run_bench(["--gpus", "8", "--dry-run", "--steps", "2", "--warmup", "1",
                                 "--workload", "cubic_stats"], timeout=400)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    out = lines[0]
    assert out["n_gpus"] == 8 and out["config"]["parallelism"] == "dp8" and out["dry_run"] is True


def test_only_rank0_builds(monkeypatch, tmp_path):
    """A rank other than 0 never runs the build: with the library missing it
    exits non-zero instead of racing rank 0's make into the same lib/."""
    import bench
    sys.path.insert(0, str(REPO / "arm-neon-opencv_amd"))
    import vacv_amd
    calls = []
    monkeypatch.setattr(vacv_amd._lib, "HIP_LIB", tmp_path / "libvacv_hip.so")
    monkeypatch.setattr(vacv_amd._lib, "build", lambda: calls.append("build"))
    with pytest.raises(SystemExit) as e:
        bench.ensure_built(rank=1, world=1)
    assert e.value.code == 2 and calls == []
    with pytest.raises(SystemExit):
        bench.ensure_built(rank=0, world=1)  # rank 0 builds (stubbed: still missing -> exit)
    assert calls == ["build"]
