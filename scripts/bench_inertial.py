"""bench.py's workload with the per-env mass / inertia / armature in use: every env's values are drawn
+-20 % around the model's right after the batch is made (Batch.set_inertial), so the timed launches take the
kernels with the per-env reads.  Same arguments as bench.py, e.g.

    python scripts/bench_inertial.py --config c3 --gpus 1 --steps 200 --warmup 20

Prints bench.py's JSON line; the host time of the set_inertial call goes to stderr."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from mujoco_ros2_simulation_amd import sim  # noqa: E402

_make = sim.Batch.__init__


def _make_and_randomise(self, model, n_envs, device=0):
    _make(self, model, n_envs, device)
    rng = np.random.default_rng(0)
    draw = lambda a: a * rng.uniform(0.8, 1.2, (n_envs,) + a.shape)
    t0 = time.perf_counter()
    self.set_inertial(draw(model.body_mass), draw(model.body_inertia), draw(model.dof_armature))
    print(f"set_inertial: {n_envs} envs (nbody {model.nbody}, nv {model.nv}) in {time.perf_counter() - t0:.3f} s",
          file=sys.stderr)


sim.Batch.__init__ = _make_and_randomise

if __name__ == "__main__":
    bench.main()
