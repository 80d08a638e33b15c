"""Wall time of ending a scattered 1/16 of the episodes of the C3 batch (scenes/arm7_lidar.xml, 8192
envs), two ways: (a) one mrs_batch_reset(key, e, 1) per env, (b) one mrs_batch_reset_masked_device with a
device mask.  Each run is timed on the host from the first call to mrs_batch_sync returning; the median
of --runs runs after --warmup warm-up runs is reported (the masked-reset subsection).
Prints one JSON line.  Needs the GPU: there is no fallback.

    python scripts/measure_masked_reset.py [--envs 8192] [--runs 20] [--warmup 3]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mujoco_ros2_simulation_amd import sim, synth  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=8192)
    p.add_argument("--runs", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    import torch

    model = sim.Model.load(ROOT / "scenes" / "arm7_lidar.xml")
    n = args.envs
    mask = np.random.default_rng(args.seed).random(n) < 1.0 / 16.0
    envs = [int(e) for e in np.flatnonzero(mask)]
    d_mask = torch.from_numpy(mask).cuda()
    torch.cuda.synchronize()
    b = sim.Batch(model, n)
    b.set(sim.FIELD_QPOS, synth.initial_qpos(model, np.arange(n)))
    b.step(10)
    b.sync()

    def per_env():
        for e in envs:
            b.reset(-1, e, 1)
        b.sync()

    def masked():
        b.reset_where_device(d_mask.data_ptr(), key=-1)
        b.sync()

    times = {"per_env_reset_ms": [], "masked_reset_ms": []}
    for run in range(args.warmup + args.runs):
        for name, call in (("per_env_reset_ms", per_env), ("masked_reset_ms", masked)):  # alternating
            b.step(1)
            b.sync()
            t0 = time.perf_counter()
            call()
            dt = 1e3 * (time.perf_counter() - t0)
            if run >= args.warmup:
                times[name].append(dt)
    out = {"scene": "arm7_lidar", "n_envs": n, "reset_envs": len(envs), "runs": args.runs, "warmup": args.warmup}
    for name, ts in times.items():
        out[name] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
    out["ratio"] = out["per_env_reset_ms"]["median"] / out["masked_reset_ms"]["median"]
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
