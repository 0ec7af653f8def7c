"""bench.py command-line contract: a plain run reports the headline
figure only, --full adds roofline / per-kernel / CPU-baseline figures,
--steps sets the number of timed steps, and --dump-outputs writes the
last timed step's results as float64 .npy files."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype",
            "ms_per_step")
FULL_ONLY = ("roofline", "cpu_baseline", "kernel_ms_per_pair")
# smallest workload that still runs the headline path: 256^3 keeps the
# ~10% x-overlap wide enough for the ground-truth gate inside bench.py
SMALL = ["--size", "256", "--pairs", "4", "--distinct", "2",
         "--steps", "3", "--warmup", "1"]


def _run(*extra):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", *SMALL, *extra],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_dump_outputs_writes_float64_npy(tmp_path):
    import bench

    res = [dict(shift=np.array([1.5, -2.0, 0.25]), r=0.9, valid=True),
           dict(shift=np.array([0.0, 3.0, -1.0]), r=0.1, valid=False)]
    out = os.path.join(str(tmp_path), "nested", "dump")
    bench.dump_outputs(out, res, rank=0, world=1)
    assert sorted(os.listdir(out)) == ["r.npy", "shift.npy", "valid.npy"]
    shift = np.load(os.path.join(out, "shift.npy"))
    assert shift.dtype == np.float64 and shift.shape == (2, 3)
    assert np.array_equal(shift, [[1.5, -2.0, 0.25], [0.0, 3.0, -1.0]])
    assert np.array_equal(np.load(os.path.join(out, "r.npy")), [0.9, 0.1])
    valid = np.load(os.path.join(out, "valid.npy"))
    assert valid.dtype == np.float64 and np.array_equal(valid, [1.0, 0.0])


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr


@pytest.mark.gpu
def test_bench_inputs_identical_between_contexts():
    """Same arguments -> bit-identical resident tiles (the device renderer
    sums overlapping blobs in an order-independent way)."""
    import bench
    from bigstitcher_spark_amd import Context

    size, got = 256, []
    for _ in range(2):
        with Context(0) as ctx:
            shifts = bench.make_rank_pairs(ctx, 0, size, 1, 0.1)
            got.append((shifts, ctx.download(0, (size,) * 3),
                        ctx.download(1, (size,) * 3)))
    assert got[0][0] == got[1][0]
    assert got[0][1].max() > 1000  # blobs rendered, not just the noise floor
    assert np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][2], got[1][2])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    out = os.path.join(str(tmp_path), "dump")
    line = _run("--dump-outputs", out)
    for k in CONTRACT:
        assert k in line, k
    for k in FULL_ONLY:
        assert k not in line, k
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    # value is whole-job pairs/s over exactly --steps timed steps
    assert line["value"] == pytest.approx(
        4 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    shift = np.load(os.path.join(out, "shift.npy"))
    r = np.load(os.path.join(out, "r.npy"))
    valid = np.load(os.path.join(out, "valid.npy"))
    assert shift.dtype == r.dtype == valid.dtype == np.float64
    assert shift.shape == (4, 3) and r.shape == (4,) and valid.shape == (4,)
    assert np.all(valid == 1.0) and np.all(np.isfinite(shift))
    # pairs cycle over the 2 distinct scenes
    assert np.allclose(shift[0], shift[2], atol=1e-3)
    assert np.abs(shift).max() > 100  # the ~0.9*size x offset was found


@pytest.mark.gpu
def test_full_run_adds_roofline_and_cpu_baseline():
    line = _run("--full")
    for k in CONTRACT + FULL_ONLY:
        assert k in line, k
    assert line["roofline"]["kernel"] in line["kernel_ms_per_pair"]
    assert line["cpu_baseline"]["value"] > 0
    assert line["cpu_baseline"]["kind"] == "port"
