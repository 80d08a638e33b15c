"""bench.py's command line: a plain run (timed steps + the result line only), --full (the CPU
baseline on top) and --dump-outputs (the last step's outputs as .npy, identical from run to run)."""
import importlib.util
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench_module():
    spec = importlib.util.spec_from_file_location("mrs_bench", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_long_ctrl_table_equals_one_call(arm7_model):
    """the sliced, threaded table build of a long run gives the values of one synth.ctrl_table call
    (600 periods: two full slices and a partial one)"""
    import torch
    from mujoco_ros2_simulation_amd import synth
    bench = _bench_module()
    ids = np.arange(5, 5 + 33)
    want = synth.ctrl_table(arm7_model, ids, 600, 10).astype(np.float32)
    got = bench.ctrl_table_device(torch, synth, arm7_model, ids, 600, 10, "cpu")
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)


def test_dump_rows_fixed_sample():
    """an output under the per-array cap is kept whole; a larger one keeps the same sorted rows every
    time, sized to the cap"""
    bench = _bench_module()
    assert np.array_equal(bench.dump_rows(8192, 28), np.arange(8192))
    row = 640 * 480 * 4
    a, b = bench.dump_rows(2048, row), bench.dump_rows(2048, row)
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0) and a.max() < 2048
    assert len(a) == bench.DUMP_ARRAY_BYTES // row and len(a) * row <= bench.DUMP_ARRAY_BYTES


def _run(*args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--envs", "64", "--steps", "3",
                        "--warmup", "1", *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(tmp_path, arm7_model):
    """a plain run times exactly --steps steps, reports ms_per_step and measures no CPU baseline; its
    dumped outputs are float32, finite, shaped [envs, dim], and identical in a second run"""
    dirs = [tmp_path / "a", tmp_path / "b"]
    res = [_run("--dump-outputs", str(d)) for d in dirs]
    d = res[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["ms_per_step"] > 0 and "cpu_baseline" not in d
    assert d["value"] == pytest.approx(64 * 3 * 10 / (d["ms_per_step"] * 3e-3))
    dims = {"qpos": arm7_model.nq, "qvel": arm7_model.nv, "sensordata": arm7_model.nsensordata}
    assert sorted(p.name for p in dirs[0].iterdir()) == sorted(k + ".npy" for k in dims)
    for name, dim in dims.items():
        a, b = np.load(dirs[0] / f"{name}.npy"), np.load(dirs[1] / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (64, dim) and np.isfinite(a).all()
        assert np.array_equal(a, b), name
    q0 = np.load(dirs[0] / "qpos.npy")
    assert np.ptp(q0, axis=0).max() > 0   # per-env synthetic inputs: the envs differ


@pytest.mark.gpu
def test_full_adds_cpu_baseline():
    d = _run("--full", "--cpu-seconds", "0.2")
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["unit"] == "env-steps/s"
