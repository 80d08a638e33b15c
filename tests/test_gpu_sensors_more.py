"""velocimeter, framelinvel / frameangvel / framelinacc, frame axis, subtreecom / subtreelinvel and touch
sensors on the GPU against the fp64 reference of tests/sensor_ref.py, by the re-seeded method of
test_gpu_parity.test_imu_ft_reseeded_1e5: every step starts from the oracle's fp64 state rounded to
fp32, and sensordata after forward() and after step(1) (sensors are sensed before integration) is
compared with the reference at that start state.

Bar: per sensor the worst |gpu - ref| <= 1e-5 x max(1, largest |ref|); for touch, and framelinacc on a
body with contacts, the scale is also at least the tree's mass x |g| (the forces in balance, as for the
force sensors of test_imu_ft_reseeded_1e5).  The known sensors of the same scenes against the oracle's
own sensordata to the same bar.  Env-steps whose contact count differs from the oracle's are excluded,
at most 1 % of them, each explained by tests/flips.py."""
import ctypes

import numpy as np
import pytest

import binding
from conftest import ROOT
from flips import explain_flip
from mujoco_ros2_simulation_amd import sim, synth
from sensor_ref import SensorRef
from sensor_scenes import (ARM, ARM_KNOWN, ARM_SENSORS, FLOAT, FLOAT_KNOWN, FLOAT_OPTIONS, FLOAT_SENSORS, bare,
                           float_start, with_sensors)

pytestmark = pytest.mark.gpu
FIELDS = ((sim.FIELD_QPOS, "qpos"), (sim.FIELD_QVEL, "qvel"), (sim.FIELD_QACC_WARMSTART, "qacc_warmstart"),
          (sim.FIELD_CTRL, "ctrl"))


def _reseeded(model, sref, n, steps, starts, period=10):
    """worst |gpu - reference| and largest |reference| per sensor over the env-steps whose contact
    counts agree; the number of excluded env-steps"""
    envs = np.arange(n)
    table = synth.ctrl_table(model, envs, steps // period + 1, period) if model.nu else None
    orc = [binding.OracleData(model) for _ in envs]
    ref = [binding.OracleData(model) for _ in envs]
    for d, (q, v) in zip(orc, starts):
        d.qpos[:], d.qvel[:] = q, v
    b = sim.Batch(model, n)
    layout = b.layout()
    new = set(sref.sensors)
    err, mag = np.zeros(model.nsensor), np.zeros(model.nsensor)
    flips, unexplained = 0, []
    for t in range(steps):
        for e, (d, r) in enumerate(zip(orc, ref)):
            if t % period == 0 and model.nu:
                d.ctrl[:] = table[t // period, e]
            for k in ("qpos", "qvel", "qacc_warmstart", "ctrl"):
                getattr(r, k)[:] = getattr(d, k).astype(np.float32)
        got = []
        for call in (b.forward, lambda: b.step(1)):
            for f, k in FIELDS:
                b.set(f, np.array([getattr(r, k) for r in ref]))
            call()
            got.append(b.get(sim.FIELD_SENSORDATA))
        start = [(r.qpos.copy(), r.qvel.copy()) for r in ref]
        want = np.zeros((n, model.nsensordata))
        for e, (d, r) in enumerate(zip(orc, ref)):
            ws = r.qacc_warmstart.copy()
            r.forward()
            vals = sref.values(r.qpos, r.qvel, r.ctrl, ws, main=r)
            r.qacc_warmstart[:] = ws
            r.step()
            d.step()
            want[e] = r.sensordata  # (of the step's start state; zeros in the new sensors' slots)
            for i, v in vals.items():
                want[e, model.sensor_adr[i]:model.sensor_adr[i] + model.sensor_dim[i]] = v
        nc, nr = b.get(sim.FIELD_NCON)[:, 0].astype(int), np.array([r.ncon for r in ref])
        ok = nc == nr
        flips += int(np.sum(~ok))
        for e in np.flatnonzero(~ok):
            done, diff, _ = explain_flip(model, *start[e], b.contacts(int(e))[0])
            if not done:
                unexplained.append((t, int(e), diff))
        for s in got:
            for i in range(model.nsensor):
                a, dim = model.sensor_adr[i], model.sensor_dim[i]
                if ok.any():
                    err[i] = max(err[i], float(np.max(np.abs(s[ok, a:a + dim] - want[ok, a:a + dim]))))
                    mag[i] = max(mag[i], float(np.max(np.abs(want[ok, a:a + dim]))))
    b.close()
    assert not unexplained, unexplained[:5]
    return err, mag, flips, layout, new


def _check(model, err, mag, flips, n, steps, contact_bodies=()):
    scale = np.maximum(mag, 1.0)
    for i in range(model.nsensor):
        t = model.sensor_type[i]
        if t in (sim.SENS_TOUCH, sim.SENS_FRAMELINACC) and model.sensor_objtype[i] == sim.OBJ_SITE:
            body = model.site_bodyid[model.sensor_objid[i]]
            if body in contact_bodies:
                scale[i] = max(scale[i], float(model.body_subtreemass[model.body_rootid[body]]) * 9.81)
    rel = err / scale
    for i in range(model.nsensor):
        print(f"{model.id2name(sim.OBJ_SENSOR, i):22s} max |err| {err[i]:.2e}  scale {scale[i]:.3g}  rel {rel[i]:.2e}")
    print(f"excluded env-steps {flips} of {n * steps}")
    assert flips <= 0.01 * n * steps
    worst = int(np.argmax(rel))
    assert rel.max() <= 1e-5, (model.id2name(sim.OBJ_SENSOR, worst), rel.max())


def _arm(monkeypatch, group, helpers):
    monkeypatch.setenv("MRS_GROUP", str(group))
    for k in ("MRS_G16_WPB", "MRS_RAY_HELPERS"):
        monkeypatch.delenv(k, raising=False)
    if helpers:
        monkeypatch.setenv("MRS_G16_WPB", "1")
        monkeypatch.setenv("MRS_RAY_HELPERS", "1")
    sens = ARM_SENSORS + ARM_KNOWN
    model = sim.Model.from_string(with_sensors(ARM, sens, lidar=helpers))
    # more new sensors than a 16-lane group has lanes: the per-lane sensor loop wraps
    sref = SensorRef(bare(ARM, lidar=helpers), model)
    assert len(sref.sensors) >= 17
    n, steps = 8, 50
    q0 = synth.initial_qpos(model, np.arange(n))
    err, mag, flips, layout, new = _reseeded(model, sref, n, steps, [(q, np.zeros(model.nv)) for q in q0])
    assert layout["group"] == group and layout["helper_waves"] == (1 if helpers else 0)
    if helpers:  # (the rays against the oracle's are test_gpu_parity's business: grazing hits differ)
        for i in range(model.nsensor):
            if model.sensor_type[i] == sim.SENS_RANGEFINDER:
                err[i] = 0
    _check(model, err, mag, flips, n, steps)


@pytest.mark.parametrize("group", [16, 64])
def test_arm_sensors_reseeded_1e5(group, monkeypatch):
    """scene A: a frame sensor of each kind on a site, a body and a geom, velocimeters, subtree sensors
    on the root link and on a link further out, beside the IMU sensors"""
    _arm(monkeypatch, group, False)


def test_arm_sensors_with_helper_waves(monkeypatch):
    """scene A with a lidar in the helper-wave layout (one-wave workgroups, a helper wave per physics
    wave tracing the rays): the physics wave senses the new sensors"""
    _arm(monkeypatch, 16, True)


@pytest.mark.parametrize("group", [16, 64])
@pytest.mark.parametrize("solver", sorted(FLOAT_OPTIONS))
def test_float_sensors_reseeded_1e5(solver, group, monkeypatch):
    """scene B: a free box with a hinged flap landing on the floor; touch pads (one enclosing the
    underside, one no contact ray meets), velocimeter / framelinvel / framelinacc / subtree sensors"""
    monkeypatch.setenv("MRS_GROUP", str(group))
    model = sim.Model.from_string(with_sensors(FLOAT, FLOAT_SENSORS + FLOAT_KNOWN, option=FLOAT_OPTIONS[solver]))
    sref = SensorRef(bare(FLOAT, option=FLOAT_OPTIONS[solver]), model)
    n, steps = 8, 120
    err, mag, flips, layout, new = _reseeded(model, sref, n, steps, [float_start(model, e) for e in range(n)])
    assert layout["group"] == group
    under, miss = model.name2id(sim.OBJ_SENSOR, "under"), model.name2id(sim.OBJ_SENSOR, "miss")
    assert mag[under] > 1 and mag[miss] == 0 and err[miss] == 0
    _check(model, err, mag, flips, n, steps, contact_bodies=(model.name2id(sim.OBJ_BODY, "box"),))


def test_plugin_finds_imu_and_ft_behind_other_sensors(tmp_path):
    """the plugin maps its IMU / force-torque state interfaces by sensor name: a velocimeter and a touch
    sensor ahead of them in <sensor> shift the sensordata addresses, and the interfaces follow"""
    from mujoco_ros2_simulation_amd import plugin
    scene = (ROOT / "scenes" / "imu_ft.xml").read_text()
    scene = scene.replace('<site name="box_site" pos="0 0 0"/>',
                          '<site name="box_site" pos="0 0 0"/><site name="box_pad" type="box" size="0.12 0.12 0.02" pos="0 0 -0.1"/>')
    scene = scene.replace("<sensor>", '<sensor><velocimeter name="imu_vel" site="imu"/><touch name="box_touch" site="box_pad"/>')
    (tmp_path / "scenes").mkdir()
    (tmp_path / "scenes" / "imu_ft.xml").write_text(scene)
    s = plugin.System(ROOT / "tests" / "fixtures" / "imu_ft.urdf", {}, {"mrs_tests": str(tmp_path)})
    s.set_param("physics_thread", "false")
    assert s.on_init() == plugin.SUCCESS
    s.set_command("j1/effort", 0.3)
    s.set_command("j2/effort", -0.2)
    for _ in range(25):
        s.cycle(0.02, 10)
    m = sim.Model.load(tmp_path / "scenes" / "imu_ft.xml")
    assert m.sensor_adr[m.name2id(sim.OBJ_SENSOR, "imu_quat")] == 4 + 9
    sd = np.zeros(m.nsensordata)
    assert sim.lib().mrs_batch_get_field(s.batch_handle(), sim.FIELD_SENSORDATA, sd.ctypes.data_as(ctypes.c_void_p), 0, 1) == 0

    def val(name):
        i = m.name2id(sim.OBJ_SENSOR, name)
        return sd[m.sensor_adr[i]:m.sensor_adr[i] + m.sensor_dim[i]]

    assert [s.state(f"imu/orientation.{c}") for c in "wxyz"] == pytest.approx(list(val("imu_quat")), abs=1e-12)
    assert [s.state(f"imu/angular_velocity.{c}") for c in "xyz"] == pytest.approx(list(val("imu_gyro")), abs=1e-12)
    assert [s.state(f"imu/linear_acceleration.{c}") for c in "xyz"] == pytest.approx(list(val("imu_accel")), abs=1e-12)
    assert [s.state(f"ft/force.{c}") for c in "xyz"] == pytest.approx(list(-val("ft_force")), abs=1e-12)
    assert [s.state(f"ft/torque.{c}") for c in "xyz"] == pytest.approx(list(-val("ft_torque")), abs=1e-12)
    assert np.linalg.norm(val("imu_gyro")) > 0.1 and np.linalg.norm(val("imu_vel")) > 0.01
    # the box has landed: the pad under it reads about its weight
    assert val("box_touch")[0] == pytest.approx(1.5 * 9.81, rel=0.05)
    s.close()
