"""GPU parity of spatial tendons (MJCF <tendon><spatial> through sites and pulleys; step.hip
spatial_tendons): length, velocity and Jacobian per env against the fp64 reference tests/tendon_ref.py,
closed forms on a pendulum, and re-seeded one-step parity against the oracle stepping a twin it knows --
the scene without the tendons under qfrc_applied = J' f (springs, dampers, tendon actuators), and for
straight tendons along slide axes the same scene with <fixed> tendons (limit and friction-loss rows).
6 envs: at G = 16 one full wave of four envs and a partial one.  Bar: 1e-5 relative (atol 1e-5)."""
import numpy as np
import pytest

import binding
import tendon_ref
from mujoco_ros2_simulation_amd import sim
from test_tendon_kat import _soft
from xfrc_ref import rk4_step

pytestmark = pytest.mark.gpu

N = 6
TOL = dict(rtol=1e-5, atol=1e-5)
EFC_TLIMIT = 6


def chain_states(ft, seed):
    """per env a seeded pose and velocity of the chain whose shortest segment is at least 0.05 m"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1, 1, (N, 4)) * [1, 1, 1, 0.2]
    v = rng.uniform(-2, 2, (N, 4)) * [1, 1, 1, 0.3]
    q, v = q.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64)
    for e in range(N):
        assert ft.kin(q[e], v[e])[3] >= 0.05
    return q, v


def sensor(model, data, name):
    i = model.name2id(sim.OBJ_SENSOR, name)
    return data[:, model.sensor_adr[i]]


SCENE1_SENSORS = ('<sensor><tendonpos name="pA" tendon="A"/><tendonvel name="vA" tendon="A"/><tendonpos name="pB" tendon="B"/>'
                  '<tendonvel name="vB" tendon="B"/><tendonpos name="pC" tendon="C"/><tendonvel name="vC" tendon="C"/></sensor>')


@pytest.mark.parametrize("group", [16, 64])
def test_length_velocity_jacobian(group, monkeypatch):
    """tendonpos / tendonvel after forward() and the limit rows' J and pos (through aref) per env"""
    monkeypatch.setenv("MRS_GROUP", str(group))
    lo, hi = 0.01, 0.02  # (every pose is longer: the upper limit is active in every env)
    xml = tendon_ref.CHAIN.format(option="", extra=SCENE1_SENSORS, tendon=(
        f'<spatial name="A">{tendon_ref.PATH_A}</spatial>'
        f'<spatial name="B" range="{lo} {hi}">{tendon_ref.PATH_B}</spatial>' + tendon_ref.FIXED_C))
    ft = tendon_ref.ForceTwin(xml)
    m = ft.model
    q, v = chain_states(ft, 11)
    b = sim.Batch(m, N)
    assert b.layout()["group"] == group
    b.set(sim.FIELD_QPOS, q)
    b.set(sim.FIELD_QVEL, v)
    b.forward()
    sd = b.get(sim.FIELD_SENSORDATA)
    rows = [b.efc(e) for e in range(N)]
    b.close()
    _, K, B = _soft()
    for e in range(N):
        L, Ld, J, _ = ft.kin(q[e], v[e])
        assert L[1] > hi + 0.05
        for t, name in enumerate("ABC"):
            print(f"G={group} env {e} tendon {name}: L {L[t]:.6f} got {sensor(m, sd, 'p' + name)[e]:.6f}  "
                  f"Ldot {Ld[t]:.6f} got {sensor(m, sd, 'v' + name)[e]:.6f}")
            np.testing.assert_allclose(sensor(m, sd, "p" + name)[e], L[t], **TOL)
            np.testing.assert_allclose(sensor(m, sd, "v" + name)[e], Ld[t], **TOL)
        r = rows[e]
        assert r["type"].tolist() == [EFC_TLIMIT], r["type"]
        np.testing.assert_allclose(r["J"][0], -J[1], **TOL)
        # pos = range[1] - L, past solimp's width: aref = -B J qvel - K dmax pos
        pos = hi - L[1]
        assert abs(pos) > 0.001
        np.testing.assert_allclose(r["aref"][0], -B * (-Ld[1]) - K * 0.95 * pos, rtol=1e-5, atol=1e-5)


def test_pendulum_closed_form():
    """tendonpos = sqrt(a^2 + r^2 - 2 a r cos(th + th0)), tendonvel = a r sin(th + th0) thdot / L"""
    a, r, th0 = 0.5, 0.3, 0.4
    m = tendon_ref.pendulum(a, r, th0)
    th = np.array([-2.5, -1.0, 0.3, 0.9, 1.7, 2.6])
    thd = np.array([1.5, -2.0, 0.7, 3.0, -1.2, 0.4])
    b = sim.Batch(m, N)
    b.set(sim.FIELD_QPOS, th[:, None])
    b.set(sim.FIELD_QVEL, thd[:, None])
    b.forward()
    sd = b.get(sim.FIELD_SENSORDATA)
    b.close()
    L = np.sqrt(a * a + r * r - 2 * a * r * np.cos(th + th0))
    assert L.min() >= 0.05
    np.testing.assert_allclose(sd[:, 0], L, **TOL)
    np.testing.assert_allclose(sd[:, 1], a * r * np.sin(th + th0) * thd / L, **TOL)


def scene3(option):
    # A: a spring with a dead band (the seeded lengths fall below, inside and above it) and a damper, under
    # a motor; B: a damper under a position servo with a ctrl range; C fixed, under a motor the twin keeps.
    # Stiffness and gains are of the size of tests/test_gpu_tendon.py's: the links weigh 0.3 kg, and the bar
    # is elementwise -- an fp32 solve whose largest component is a few hundred rad/s^2 leaves 1e-7 of that
    # on its small components, which is the bar itself
    return tendon_ref.CHAIN.format(option=option, tendon=(
        f'<spatial name="A" stiffness="4" damping="0.05" springlength="0.9 1.06">{tendon_ref.PATH_A}</spatial>'
        f'<spatial name="B" damping="0.03">{tendon_ref.PATH_B}</spatial>' + tendon_ref.FIXED_C),
        extra='<actuator><motor tendon="A" gear="0.5" ctrllimited="true" ctrlrange="-1 1"/>'
              '<position tendon="B" kp="1" kv="0.05" gear="2" ctrllimited="true" ctrlrange="1.6 2.4"/>'
              '<motor tendon="C" gear="0.3"/></actuator>')


@pytest.mark.parametrize("integrator, group", [("Euler", 16), ("Euler", 64), ("RK4", 16)])
def test_step_parity_force_twin(integrator, group, monkeypatch):
    """one step from each seeded state: qpos, qvel, qacc, qfrc_actuator against the oracle stepping the
    scene without the spatial tendons under their joint-space force"""
    monkeypatch.setenv("MRS_GROUP", str(group))
    ft = tendon_ref.ForceTwin(scene3(f'integrator="{integrator}"'))
    m = ft.model
    q, v = chain_states(ft, 23)
    rng = np.random.default_rng(7)
    ctrl = rng.uniform(-1.5, 3.0, (N, m.nu)).astype(np.float32).astype(np.float64)  # (past both ctrl ranges)
    LA = np.array([ft.kin(q[e], v[e])[0][0] for e in range(N)])
    print("lengths of A", LA)
    assert (LA < 0.9).any() and ((LA >= 0.9) & (LA <= 1.06)).any() and (LA > 1.06).any()
    b = sim.Batch(m, N)
    assert b.layout()["group"] == group
    for f, x in ((sim.FIELD_QPOS, q), (sim.FIELD_QVEL, v), (sim.FIELD_CTRL, ctrl)):
        b.set(f, x)
    b.forward()
    acc, qact = b.get(sim.FIELD_QACC), b.get(sim.FIELD_QFRC_ACTUATOR)
    b.step(1)
    q1, v1 = b.get(sim.FIELD_QPOS), b.get(sim.FIELD_QVEL)
    b.close()
    for e in range(N):
        d = binding.OracleData(ft.twin)
        d.qpos[:], d.qvel[:], d.ctrl[:] = q[e], v[e], ctrl[e][ft.keep]
        qf, qa = ft.forces(q[e], v[e], ctrl[e])
        d.qfrc_applied[:] = qf
        d.forward()
        print(f"{integrator} G={group} env {e}: |qacc| {np.abs(d.qacc).max():.3g} err {np.abs(acc[e] - d.qacc).max():.2e}")
        np.testing.assert_allclose(acc[e], d.qacc, **TOL)
        np.testing.assert_allclose(qact[e], d.qfrc_actuator + qa, **TOL)
        if integrator == "RK4":
            ft.vel_of = d
            qn, vn = rk4_step(ft.twin, d, ft, ctrl[e])
        else:
            d.step()
            qn, vn = d.qpos.copy(), d.qvel.copy()
        np.testing.assert_allclose(q1[e], qn, **TOL)
        np.testing.assert_allclose(v1[e], vn, **TOL)


# two sliders along x; T1 straight from a world site to slider a: L = 0.25 + q1, limited to [0.15, 0.35]; T2 the
# same segment, then behind a pulley of divisor 2 a world site to slider b: L = (0.25 + q1) + (0.25 + q2) / 2,
# with friction loss, under a motor.  The tendons are a quarter metre long and the limit's solref is 0.1 s:
# an fp32 length carries 2^-24 L of rounding, which a limit row turns into K imp 2^-24 L of acceleration --
# 1.6e-6 m/s^2 here (K imp = 105 / s^2), against 1.6e-4 for a metre of tendon under the default solref, which
# no elementwise 1e-5 on an acceleration of a few m/s^2 can hold (the fixed twin's length is q1 itself)
SLIDERS = """<mujoco><option timestep="0.002" solver="{solver}" iterations="{it}" tolerance="1e-10"/>
<worldbody><site name="wa" pos="-0.25 0 0.5"/><site name="wb" pos="-0.25 0.3 0.5"/>
<body name="a" pos="0 0 0.5"><joint name="s1" type="slide" axis="1 0 0" damping="0.2"/>
  <geom type="box" size="0.05 0.05 0.05" mass="1" contype="0" conaffinity="0"/><site name="sa"/></body>
<body name="b" pos="0 0.3 0.5"><joint name="s2" type="slide" axis="1 0 0"/>
  <geom type="box" size="0.05 0.05 0.05" mass="2" contype="0" conaffinity="0"/><site name="sb"/></body>
</worldbody>
<tendon><spatial name="T1" range="0.15 0.35" solreflimit="0.1 1"><site site="wa"/><site site="sa"/></spatial>
<spatial name="T2" frictionloss="0.6"><site site="wa"/><site site="sa"/><pulley divisor="2"/><site site="wb"/><site site="sb"/></spatial></tendon>
<actuator><motor tendon="T2" gear="1.5"/></actuator></mujoco>"""
# (the envs outside the range are a few millimetres outside, and the speeds 0.1 m/s: the limit rows then ask
# for accelerations of order 10 m/s^2.  Deeper or faster, K pos and B vel reach hundreds of m/s^2, and an
# fp32 qacc that is the small remainder of such terms cannot hold an elementwise 1e-5)
SLIDER_Q = np.array([[-0.108, 0.1], [-0.104, -0.15], [0.0, 0.05], [0.04, -0.1], [0.103, 0.2], [0.107, -0.05]])


@pytest.mark.parametrize("solver, group", [("PGS", 16), ("PGS", 64), ("Newton", 16), ("Newton", 64), ("CG", 16)])
def test_step_parity_row_twin(solver, group, monkeypatch):
    """one step, and step(10) as one fused launch, from each seeded state against the oracle stepping the
    same scene with the equivalent fixed tendons: limit rows below / inside / above the range, a
    friction-loss row through a pulley, a tendon motor"""
    monkeypatch.setenv("MRS_GROUP", str(group))
    xml = SLIDERS.format(solver=solver, it={"PGS": 50, "Newton": 100, "CG": 100}[solver])
    m = sim.Model.from_string(xml)
    twin = sim.Model.from_string(tendon_ref.row_twin_xml(xml))
    assert twin.tendon_kind.tolist() == [sim.TENDON_FIXED] * 2
    q = SLIDER_Q
    L1 = 0.25 + q[:, 0]
    assert (L1 < 0.15).sum() >= 2 and ((L1 > 0.15) & (L1 < 0.35)).sum() >= 2 and (L1 > 0.35).sum() >= 2
    rng = np.random.default_rng(3)
    v = rng.uniform(-0.1, 0.1, (N, 2)).astype(np.float32).astype(np.float64)
    ctrl = rng.uniform(-1, 1, (N, 1)).astype(np.float32).astype(np.float64)
    b = sim.Batch(m, N)
    assert b.layout()["group"] == group
    for steps in (1, 10):
        for f, x in ((sim.FIELD_QPOS, q), (sim.FIELD_QVEL, v), (sim.FIELD_CTRL, ctrl),
                     (sim.FIELD_QACC_WARMSTART, np.zeros((N, 2)))):
            b.set(f, x)
        b.step(steps)
        q1, v1, acc, qact = (b.get(f) for f in (sim.FIELD_QPOS, sim.FIELD_QVEL, sim.FIELD_QACC, sim.FIELD_QFRC_ACTUATOR))
        for e in range(N):
            d = binding.OracleData(twin)
            d.qpos[:], d.qvel[:], d.ctrl[:] = q[e], v[e], ctrl[e]
            d.step(steps)
            print(f"{solver} G={group} steps {steps} env {e}: qacc {d.qacc} err {np.abs(acc[e] - d.qacc).max():.2e} "
                  f"qvel err {np.abs(v1[e] - d.qvel).max():.2e}")
            np.testing.assert_allclose(q1[e], d.qpos, **TOL)
            np.testing.assert_allclose(v1[e], d.qvel, **TOL)
            np.testing.assert_allclose(acc[e], d.qacc, **TOL)
            np.testing.assert_allclose(qact[e], d.qfrc_actuator, **TOL)
    b.close()


def test_set_inertial_refused():
    xml = tendon_ref.CHAIN.format(option="", extra="", tendon=f'<spatial name="A">{tendon_ref.PATH_A}</spatial>')
    m = sim.Model.from_string(xml)
    b = sim.Batch(m, N)
    with pytest.raises(sim.MrsError) as ei:
        b.set_inertial(mass=np.tile(m.body_mass, (N, 1)))
    assert ei.value.code == -4  # MRS_ERR_UNSUPPORTED
    b.close()
