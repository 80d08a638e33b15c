"""Sensor cadence of a fused launch (step.hip step_kernel, DevModel::sens_every): step(n) evaluates and
stores the sensors on its last step only -- sensordata after n steps is that of the last step's forward
pass, each earlier step's values are overwritten unread, and sensors feed nothing back into the
dynamics.  MRS_SENSORS_EVERY_STEP=1 at batch creation evaluates them on every step, as before.  Neither
mode changes any arithmetic, so after the same calls every output of the two modes must be identical
bit for bit: qpos, qvel, qacc, qacc_warmstart, qfrc_actuator, sensordata, time, ncon, niter, warning.

Every GPU test builds the two batches of one scene in one process and asserts the mode through
layout()."""
from pathlib import Path

import numpy as np
import pytest

from mujoco_ros2_simulation_amd import sim, synth
from sensor_scenes import FLOAT, FLOAT_KNOWN, FLOAT_SENSORS, float_start, with_sensors

ROOT = Path(__file__).resolve().parents[1]
SCENES = ROOT / "scenes"
gpu = pytest.mark.gpu

FIELDS = {"qpos": sim.FIELD_QPOS, "qvel": sim.FIELD_QVEL, "qacc": sim.FIELD_QACC,
          "qacc_warmstart": sim.FIELD_QACC_WARMSTART, "qfrc_actuator": sim.FIELD_QFRC_ACTUATOR,
          "sensordata": sim.FIELD_SENSORDATA, "time": sim.FIELD_TIME, "ncon": sim.FIELD_NCON,
          "niter": sim.FIELD_SOLVER_NITER, "warning": sim.FIELD_WARNING}
NQ_ARM = 7


def test_layout_reports_the_mode():
    """(CPU) layout() names the switch right after ray_sweep, the order mrs_debug_batch_layout writes"""
    assert sim.LAYOUT_KEYS.index("sensors_every_step") == sim.LAYOUT_KEYS.index("ray_sweep") + 1
    assert len(set(sim.LAYOUT_KEYS)) == len(sim.LAYOUT_KEYS) == 16


def _perturbed(model, b, n, seed=11):
    """the start poses of tests/test_gpu_ray_sweep.py: every joint up to 1.5 rad (m) off the default"""
    rng = np.random.default_rng(seed)
    qpos = b.get(sim.FIELD_QPOS)
    if model.nq == NQ_ARM:
        qpos += rng.uniform(-1.5, 1.5, qpos.shape)
    else:  # mobile base (free joint + two wheels): x, y, yaw and the wheel angles
        qpos[:, 0:2] += rng.uniform(-1.5, 1.5, (n, 2))
        yaw = rng.uniform(-1.5, 1.5, n)
        qpos[:, 3:7] = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], axis=1)
        qpos[:, 7:] += rng.uniform(-1.5, 1.5, (n, model.nq - 7))
    b.set(sim.FIELD_QPOS, qpos)


def _run(model, n, periods, every, monkeypatch, start=_perturbed):
    """periods: per held action the step counts of its launches, e.g. [[10], [10]] or [[1] * 10] * 2;
    the synthetic action of period p (synth.ctrl_table) is set before its launches.  Returns the layout
    and every output field after each period"""
    if every:
        monkeypatch.setenv("MRS_SENSORS_EVERY_STEP", "1")
    else:
        monkeypatch.delenv("MRS_SENSORS_EVERY_STEP", raising=False)
    b = sim.Batch(model, n)
    monkeypatch.delenv("MRS_SENSORS_EVERY_STEP", raising=False)
    lay = b.layout()
    assert lay["sensors_every_step"] == int(every), lay
    start(model, b, n)
    table = synth.ctrl_table(model, np.arange(n), len(periods), 10) if model.nu else None
    out = []
    for p, launches in enumerate(periods):
        if table is not None:
            b.set(sim.FIELD_CTRL, table[p])
        for k in launches:
            b.step(k)
        out.append({name: b.get(f).copy() for name, f in FIELDS.items()})
    b.close()
    return lay, out


def _identical(a, c, what):
    assert len(a) == len(c)
    for p, (x, y) in enumerate(zip(a, c)):
        for name in FIELDS:
            u, v = x[name], y[name]
            # (bit for bit: equal as values, NaN in the same places)
            assert u.shape == v.shape and np.array_equal(u, v, equal_nan=True), \
                (what, p, name, int((u != v).sum()), float(np.nanmax(np.abs(u - v))))


def _both(model, n, periods, monkeypatch, **kw):
    lay, last = _run(model, n, periods, False, monkeypatch, **kw)
    lay_e, every = _run(model, n, periods, True, monkeypatch, **kw)
    for k in lay:
        assert k == "sensors_every_step" or lay[k] == lay_e[k], (k, lay, lay_e)
    _identical(last, every, "last step only vs every step")
    return lay, last


def _c3_layout(monkeypatch, sweep=True):
    """C3's configuration at its full size: four-wave workgroups without helper waves"""
    monkeypatch.setenv("MRS_RAY_HELPERS", "0")
    monkeypatch.setenv("MRS_G16_WPB", "4")
    if sweep:
        monkeypatch.delenv("MRS_NO_RAY_SWEEP", raising=False)
    else:
        monkeypatch.setenv("MRS_NO_RAY_SWEEP", "1")


def _fused_vs_single(n, sweep, monkeypatch):
    _c3_layout(monkeypatch, sweep)
    model = sim.Model.load(SCENES / "arm7_lidar.xml")
    lay, fused = _both(model, n, [[10], [10]], monkeypatch)
    assert lay["group"] == 16 and lay["helper_waves"] == 0 and lay["ray_sweep"] == int(sweep), lay
    _, single = _run(model, n, [[1] * 10, [1] * 10], False, monkeypatch)
    _identical(fused, single, "step(10) vs ten step(1)")
    rays = fused[-1]["sensordata"][:, :360]
    # the comparison is not of empty outputs: the lidar saw the arm, differently per env
    assert np.any(rays > 0) and np.any(rays != rays[0:1])
    assert np.all(fused[-1]["time"] == fused[-1]["time"][0]) and abs(fused[-1]["time"][0, 0] - 20 * model.timestep) < 1e-12


@gpu
def test_fused_vs_every_step_vs_single_steps(monkeypatch):
    """C3 at 40 envs: two full workgroups and a part-full one (groups past n_envs are alive)"""
    _fused_vs_single(40, True, monkeypatch)


@gpu
def test_block_passes(monkeypatch):
    """the same with the ray sweep off (MRS_NO_RAY_SWEEP=1): the block passes' stores"""
    _fused_vs_single(8, False, monkeypatch)


@gpu
@pytest.mark.parametrize("k", [1, 2])
def test_edge_launch_lengths(k, monkeypatch):
    """step(1): the only step is the last; step(2): one step without sensors"""
    _c3_layout(monkeypatch)
    model = sim.Model.load(SCENES / "arm7_lidar.xml")
    _, out = _both(model, 40, [[k], [k]], monkeypatch)
    assert np.any(out[-1]["sensordata"][:, :360] > 0)


@gpu
@pytest.mark.parametrize("solver", ["PGS", "Newton"])
def test_helper_waves(solver, monkeypatch):
    """the mobile base with one-wave workgroups and a helper wave per physics wave: the helper skips its
    ray pass on the steps before the last and still passes the three barriers of every step"""
    monkeypatch.setenv("MRS_G16_WPB", "1")
    monkeypatch.setenv("MRS_RAY_HELPERS", "1")
    monkeypatch.delenv("MRS_NO_RAY_SWEEP", raising=False)
    xml = (SCENES / "mobile_base.xml").read_text()
    pgs = 'solver="PGS" iterations="50"'
    assert pgs in xml
    if solver != "PGS":
        xml = xml.replace(pgs, f'solver="{solver}"')
    model = sim.Model.from_string(xml, str(SCENES))
    lay, out = _both(model, 8, [[5], [5]], monkeypatch)
    assert lay["group"] == 16 and lay["helper_waves"] == 1 and lay["waves_per_workgroup"] == 1, lay
    nrf = int(np.sum(np.asarray(model.sensor_type) == sim.SENS_RANGEFINDER))
    assert nrf > 0 and np.any(out[-1]["sensordata"][:, :nrf] > 0)
    assert not out[-1]["warning"].any()  # (warning[3]: a helper-wave signal timeout)


@gpu
def test_blocked_mode(monkeypatch):
    """one env per wave (G = 64, C5's scene)"""
    for k in ("MRS_GROUP", "MRS_G16_WPB", "MRS_RAY_HELPERS"):
        monkeypatch.delenv(k, raising=False)
    model = sim.Model.load(SCENES / "arm_boxes.xml")

    def start(model, b, n):
        b.set(sim.FIELD_QPOS, synth.initial_qpos(model, np.arange(n)))

    lay, out = _both(model, 4, [[3], [3]], monkeypatch, start=start)
    assert lay["group"] == 64 and lay["blocked"] == 1, lay
    assert np.any(out[-1]["ncon"] > 0)


ACC_SENSORS = (FLOAT_SENSORS + FLOAT_KNOWN + '<force name="f_tip" site="tip"/><torque name="t_tip" site="tip"/>'
               '<force name="f_corner" site="corner"/>')


@gpu
@pytest.mark.parametrize("integrator", ["Euler", "implicitfast", "implicit", "RK4"])
def test_acceleration_sensors_and_sensors_more(integrator, monkeypatch):
    """the landing box with a hinged flap: accelerometer, force, torque, touch, framelinacc and
    subtreelinvel sensors, so rne_post (which overwrites cacc, cfrc and crb in LDS) and sensors_more
    run on the last step only -- under every integrator that follows them in the step"""
    for k in ("MRS_GROUP", "MRS_G16_WPB", "MRS_RAY_HELPERS"):
        monkeypatch.delenv(k, raising=False)
    xml = with_sensors(FLOAT, ACC_SENSORS, option=' solver="PGS" iterations="100"')
    assert 'integrator="implicitfast"' in xml
    model = sim.Model.from_string(xml.replace('integrator="implicitfast"', f'integrator="{integrator}"'))
    kinds = set(np.asarray(model.sensor_type).tolist())
    assert {sim.SENS_ACCELEROMETER, sim.SENS_FORCE, sim.SENS_TORQUE, sim.SENS_TOUCH, sim.SENS_FRAMELINACC,
            sim.SENS_SUBTREELINVEL} <= kinds

    def start(model, b, n):
        s = [float_start(model, e) for e in range(n)]
        b.set(sim.FIELD_QPOS, np.array([q for q, _ in s]))
        b.set(sim.FIELD_QVEL, np.array([v for _, v in s]))

    # 4 steps per launch; the box (3-5 cm up, falling) is on the floor within the 40 steps
    lay, out = _both(model, 4, [[4]] * 10, monkeypatch, start=start)
    assert any(np.any(o["ncon"] > 0) for o in out)
    a = model.sensor_adr[model.name2id(sim.OBJ_SENSOR, "under")]
    assert any(np.any(o["sensordata"][:, a] > 0) for o in out), "the touch pad never pressed"


@gpu
def test_auto_reset(monkeypatch):
    """one env of 8 starts with a non-finite qvel: step(3) counts the warning, resets the env on its
    first step and goes on from the reset state -- the same in both modes"""
    _c3_layout(monkeypatch)
    model = sim.Model.load(SCENES / "arm7_lidar.xml")

    def start(model, b, n):
        _perturbed(model, b, n)
        qvel = b.get(sim.FIELD_QVEL)
        qvel[5, 2] = np.inf
        b.set(sim.FIELD_QVEL, qvel)

    _, out = _both(model, 8, [[3], [3]], monkeypatch, start=start)
    w = out[-1]["warning"]
    assert w[5, 1] == 1 and w.sum() == 1, w
    assert abs(out[0]["time"][5, 0] - 3 * model.timestep) < 1e-12 and np.all(np.isfinite(out[-1]["qvel"]))
    for name in FIELDS:
        assert np.all(np.isfinite(out[-1][name])), name
