"""Site transmissions (MJCF actuators with site=; mj_transmission's mjTRN_SITE branch without refsite): the
model arrays, every construct the compiler rejects by its message, dampratio from the site's moment at
qpos0 in closed form, the fp64 reference of the GPU tests (tests/site_act_ref.py) against central
differences of the site's pose, its fp32 evaluation against the GPU tests' bar, and the plugin host on a
scene with a site actuator.  No GPU."""
import numpy as np
import pytest

import binding
import site_act_ref
import tendon_ref
from conftest import REF_PID_SCENE, gpu_available
from mujoco_ros2_simulation_amd import sim
from sensor_ref import integrate_pos, quat2mat

SLIDER = """<mujoco><option gravity="0 0 0" {option}/>{default}
<worldbody><site name="w" pos="0.3 0 0"/>
<body name="a" pos="0.7 0 0"><joint name="s" type="slide" axis="1 0 0"/>
  <geom type="box" size="0.05 0.05 0.05" mass="{m}" contype="0" conaffinity="0"/><site name="sa" pos="0 0.1 0"/></body>
</worldbody><tendon><fixed name="t"><joint joint="s" coef="1"/></fixed></tendon><actuator>{act}</actuator></mujoco>"""


def slider(act, m=2.5, option="", default=""):
    return sim.Model.from_string(SLIDER.format(act=act, m=m, option=option, default=default))


def test_model_arrays():
    m = slider('<motor joint="s"/><motor name="thr" site="sa" gear="1 2 3 4 5 6"/><position site="w" kp="3"/>'
               '<motor tendon="t"/>')
    assert sim.TRN_SITE == 4
    assert m.actuator_trntype.tolist() == [sim.TRN_JOINT, sim.TRN_SITE, sim.TRN_SITE, sim.TRN_TENDON]
    sa, w = m.name2id(sim.OBJ_SITE, "sa"), m.name2id(sim.OBJ_SITE, "w")
    assert m.actuator_trnid.tolist() == [[0, -1], [sa, -1], [w, -1], [0, -1]]
    np.testing.assert_array_equal(m.actuator_gear[1], [1, 2, 3, 4, 5, 6])
    np.testing.assert_array_equal(m.actuator_gear[2], [1, 0, 0, 0, 0, 0])  # (the default: a force along the site's x)
    np.testing.assert_array_equal(m.actuator_biasprm[2, :3], [0, -3, 0])
    # through a defaults class; every actuator element takes site=
    m = slider('<motor site="sa" class="c"/><velocity site="sa" kv="2"/><general site="sa" dyntype="filter" dynprm="0.1"/>'
               '<intvelocity site="sa" kp="2" actrange="-1 1"/>',
               default='<default><default class="c"><motor gear="0 0 1 0 0 0.5"/></default></default>')
    assert m.actuator_trntype.tolist() == [sim.TRN_SITE] * 4 and m.na == 2
    np.testing.assert_array_equal(m.actuator_gear[0], [0, 0, 1, 0, 0, 0.5])


@pytest.mark.parametrize("act, option, msg", [
    ('<motor site="sa" refsite="w"/>', "", "refsite is not supported"),
    ('<motor site="nope"/>', "", "unknown site 'nope'"),
    ('<motor site="sa" joint="s"/>', "", "'site' cannot be combined with 'joint' or 'tendon'"),
    ('<motor site="sa" tendon="t"/>', "", "'site' cannot be combined with 'joint' or 'tendon'"),
    ('<velocity site="sa"/>', 'integrator="implicitfast"', "velocity-dependent actuators on sites are supported with the Euler and RK4"),
    ('<position site="sa" kp="2" kv="0.1"/>', 'integrator="implicit"', "velocity-dependent actuators on sites"),
    ('<position site="sa" kp="2" dampratio="1"/>', 'integrator="implicitfast"', "velocity-dependent actuators on sites"),
    ('<general site="sa" gaintype="affine" gainprm="1 0 0.2"/>', 'integrator="implicitfast"', "velocity-dependent actuators on sites"),
    ('<general site="sa" biastype="affine" biasprm="0 0 -0.2"/>', 'integrator="implicit"', "velocity-dependent actuators on sites"),
    ('<motor body="a"/>', "", "only joint and tendon transmissions are supported"),
    ('<motor jointinparent="s"/>', "", "only joint and tendon transmissions are supported"),
    ('<motor site="sa" cranksite="w"/>', "", "only joint and tendon transmissions are supported"),
])
def test_rejections(act, option, msg):
    with pytest.raises(sim.MrsError, match=msg):
        slider(act, option=option)


def test_velocity_free_site_actuators_load_under_the_implicit_integrators():
    for integ in ("implicit", "implicitfast"):
        m = slider('<motor site="sa"/><position site="sa" kp="2"/><general site="sa" biastype="affine" biasprm="0.3 0 0"/>',
                   option=f'integrator="{integ}"')
        assert m.actuator_trntype.tolist() == [sim.TRN_SITE] * 3


def test_dampratio_slider_closed_form():
    """a point mass on a slide joint along x, a site actuator of gear 1 0 0 0 0 0 on it: moment 1, so its
    kv is the joint actuator's, 2 dampratio sqrt(kp m)"""
    kp, dr, mass = 7.0, 0.8, 2.5
    m = slider(f'<position site="sa" kp="{kp}" dampratio="{dr}"/><position joint="s" kp="{kp}" dampratio="{dr}"/>', m=mass)
    np.testing.assert_allclose(m.actuator_biasprm[0, 2], m.actuator_biasprm[1, 2], rtol=1e-12)
    np.testing.assert_allclose(m.actuator_biasprm[0, 2], -2 * dr * np.sqrt(kp * mass), rtol=1e-12)
    # a gear across the axis has no moment at all: mass 0, kv 0
    m = slider(f'<position site="sa" kp="{kp}" dampratio="{dr}" gear="0 1 0 0 0 0"/>', m=mass)
    assert m.actuator_biasprm[0, 2] == 0


HINGE = """<mujoco><compiler angle="radian"/><option gravity="0 0 0"/>
<worldbody><body name="p" pos="0 0 1"><joint name="h" axis="0 1 0"/>
  <geom type="sphere" size="0.05" pos="{r} 0 0" mass="1.5" contype="0" conaffinity="0"/>
  <site name="tip" pos="{r} 0 0" quat="{quat}"/></body></worldbody>
<actuator><position site="tip" kp="4" dampratio="0.6" gear="{gear}"/>
  <position joint="h" kp="4" dampratio="0.6" gear="{r}"/></actuator></mujoco>"""


def test_dampratio_hinge_lever_arm():
    """a hinge about y, a site at lever arm r along x with a tangential gear (-z: omega x r = y x x): moment r,
    the same kv as the joint actuator of gear r; also with the site turned so that its x axis is the tangent"""
    r = 0.35
    for gear, quat in (("0 0 -1 0 0 0", "1 0 0 0"), ("1 0 0 0 0 0", f"{np.cos(np.pi / 4)} 0 {np.sin(np.pi / 4)} 0")):
        m = sim.Model.from_string(HINGE.format(r=r, gear=gear, quat=quat))
        np.testing.assert_allclose(m.actuator_biasprm[0, 2], m.actuator_biasprm[1, 2], rtol=1e-12)
        assert m.actuator_biasprm[0, 2] < 0
        st = site_act_ref.SiteTwin(HINGE.format(r=r, gear=gear, quat=quat))
        np.testing.assert_allclose(st.kin(m.qpos0)[0][0], [r], rtol=1e-12)


def _vee(S):
    return np.array([S[2, 1], S[0, 2], S[1, 0]])


def test_reference_moment_against_central_differences():
    """moment_j = g_lin . R' dp/dq_j + g_rot . R' omega_j, the site's velocity and angular velocity per
    unit qvel_j by central differences of its pose, at three random poses of the chain"""
    st = site_act_ref.SiteTwin(site_act_ref.scene_a())
    m = st.model
    assert m.nv == 4 and st.on_site == [0, 1, 2] and st.keep == []
    from dyn_ref import site_pose_ref
    rng = np.random.default_rng(5)
    h = 1e-6
    d = binding.OracleData(st.twin)

    def pose(q):
        d.qpos[:] = q
        return site_pose_ref(m, d, [int(m.actuator_trnid[a, 0]) for a in st.on_site])

    for _ in range(3):
        q = rng.uniform(-1, 1, 4) * [1, 1, 1, 0.2]
        mom = st.kin(q)[0]
        P0 = pose(q)
        num = np.zeros_like(mom)
        for j in range(4):
            e = np.zeros(4)
            e[j] = 1.0
            Pp, Pm = pose(integrate_pos(m, q, e, h)), pose(integrate_pos(m, q, e, -h))
            for k, a in enumerate(st.on_site):
                R = P0[k, 3:].reshape(3, 3)
                Rp, Rm = Pp[k, 3:].reshape(3, 3), Pm[k, 3:].reshape(3, 3)
                vlin = (Pp[k, :3] - Pm[k, :3]) / (2 * h)
                omega = _vee(Rp @ Rm.T - Rm @ Rp.T) / (4 * h)
                g = m.actuator_gear[a]
                num[a, j] = (R @ g[:3]) @ vlin + (R @ g[3:]) @ omega
        assert np.abs(mom).max() > 0.1
        np.testing.assert_allclose(mom, num, rtol=1e-6, atol=1e-9)
    # at qpos0 the compiler's dampratio agrees with the reference's moment
    xml = site_act_ref.scene_a().replace("</actuator>", '<position name="pd" site="s3" kp="3" dampratio="0.5" gear="0.4 -0.3 0.5 0.02 0.03 -0.04"/></actuator>')
    st2 = site_act_ref.SiteTwin(xml)
    mo = st2.kin(st2.model.qpos0)[0][3]
    M = binding.OracleData(st2.twin).mass_matrix()
    mass = sum(M[j, j] / mo[j] ** 2 for j in range(4) if mo[j] != 0)
    np.testing.assert_allclose(st2.model.actuator_biasprm[3, 2], -0.5 * 2 * np.sqrt(3 * mass), rtol=1e-10)


def test_world_site_has_zero_moment():
    st = site_act_ref.SiteTwin(tendon_ref.CHAIN.format(option="", tendon="", extra=(
        '<actuator><motor name="a" site="w0" gear="1 2 3 4 5 6"/></actuator>')).replace("<tendon></tendon>", ""))
    assert not st.kin(np.array([0.3, -0.2, 0.5, 0.1]))[0].any()


def test_twin_has_no_site_actuator():
    xml = site_act_ref.scene_a().replace("</actuator>", '<motor name="j" joint="sl"/></actuator>').replace(
        "</sensor>", '<actuatorfrc name="f_j" actuator="j"/><jointpos joint="sl"/></sensor>')
    st = site_act_ref.SiteTwin(xml)
    assert st.on_site == [0, 1, 2] and st.keep == [3] and st.twin.nu == 1
    assert st.twin.actuator_trntype.tolist() == [sim.TRN_JOINT]
    assert st.twin.sensor_type.tolist() == [sim.SENS_ACTUATORFRC, sim.SENS_JOINTPOS]


TOL = dict(rtol=1e-5, atol=1e-5)  # (the bar of tests/test_gpu_site_actuator.py)


@pytest.mark.parametrize("scene", ["A", "B", "Bcontact"])
def test_fp32_evaluation_fits_a_quarter_of_the_gpu_bar(scene):
    """the reference evaluated in fp32 (pose, Jacobians and every product rounded) against fp64, for the
    seeds the GPU tests use: force, velocity and qfrc_actuator within a quarter of their bar, and the
    acceleration that the difference in qfrc_actuator makes, M^-1 dq, within a quarter of qacc's"""
    if scene == "A":
        st = site_act_ref.SiteTwin(site_act_ref.scene_a())
        q, v, ctrl, act = site_act_ref.states_a(23)
    else:
        st = site_act_ref.SiteTwin(site_act_ref.scene_b(contact=scene == "Bcontact"))
        q, v, ctrl = site_act_ref.states_b(31, contact=scene == "Bcontact")
        act = [None] * site_act_ref.N
    for e in range(site_act_ref.N):
        a64 = st.eval(q[e], v[e], ctrl[e], act[e])
        a32 = st.eval(q[e], v[e], ctrl[e], act[e], dtype=np.float32)
        d = binding.OracleData(st.twin)
        d.qpos[:], d.qvel[:] = q[e], v[e]
        d.qfrc_applied[:] = a64["qfrc"]
        d.forward()
        Minv = np.linalg.inv(d.mass_matrix())
        for key in ("force", "velocity", "qfrc"):
            err = np.abs(a32[key].astype(np.float64) - a64[key])
            assert (err <= 0.25 * (TOL["atol"] + TOL["rtol"] * np.abs(a64[key]))).all(), (key, e, err)
        dacc = np.abs(Minv @ (a32["qfrc"].astype(np.float64) - a64["qfrc"]))
        print(f"scene {scene} env {e}: |qacc| {np.abs(d.qacc).max():.3g}  fp32 d(qacc) {dacc.max():.2e}")
        assert (dacc <= 0.25 * (TOL["atol"] + TOL["rtol"] * np.abs(d.qacc))).all(), (e, dacc, d.qacc)


def test_plan_takes_slots_only_with_site_actuators(monkeypatch):
    """a model with site actuators plans two more floats per site actuator behind the tendons' slot (rounded
    to 4); its twin without them plans what it planned before, whatever else the process has loaded"""
    st = site_act_ref.SiteTwin(site_act_ref.scene_a())
    for g in (16, 64):
        monkeypatch.setenv("MRS_GROUP", str(g))
        a, b = sim.plan_layout(st.model, 6, 256), sim.plan_layout(st.twin, 6, 256)
        assert a["group"] == b["group"] == g
        # three site actuators: 6 slot floats, rounded to 8; the filter's activation state, 4 (the twin has
        # no actuator at all; ctrl and the forces take 4 floats either way)
        assert a["lds_floats"] == b["lds_floats"] + 8 + 4


def test_plugin_host_skips_site_actuators(tmp_path, capfd):
    """the reference PID scene plus one site motor through libmrs_plugin.so: the joint -> actuator mapping
    skips the site actuator, and the interface counts are what they were.  Without a GPU on_init gets as
    far as the batch: the scene loads, and only the device is missing"""
    from mujoco_ros2_simulation_amd import plugin
    from test_plugin import URDF
    import os
    scene_dir = tmp_path / "share" / "mujoco_ros2_control"
    scene_dir.mkdir(parents=True)
    gold = REF_PID_SCENE.parents[2]
    os.symlink(gold / "ref_scenes", scene_dir / "test_resources")
    os.symlink(gold / "ref_config", scene_dir / "config")
    # a copy of the scene (scene_pid.xml includes test_robot_pid.xml, which holds the actuators) with a site
    # motor on the end effector, first in the list: every joint actuator's id moves by one
    base = sim.Model.load(REF_PID_SCENE)
    robot = (REF_PID_SCENE.parent / "test_robot_pid.xml").read_text()
    assert robot.count("<actuator>") == 1 and 'site name="ee_link"' in robot
    (tmp_path / "test_robot_pid.xml").write_text(
        robot.replace("<actuator>", '<actuator><motor name="thruster" site="ee_link" gear="0 0 1 0 0 0"/>'))
    mod = tmp_path / "scene_pid.xml"
    mod.write_text(REF_PID_SCENE.read_text())
    m = sim.Model.load(mod)
    assert m.nu == base.nu + 1 and m.actuator_trntype.tolist() == [sim.TRN_SITE] + base.actuator_trntype.tolist()
    s = plugin.System(URDF, {"use_pid": "true", "headless": "true"}, {"mujoco_ros2_control": str(scene_dir)})
    s.set_param("physics_thread", "false")
    s.set_param("mujoco_model", str(mod))
    assert s.num_joints == 2 and s.num_sensors == 2
    capfd.readouterr()
    r = s.on_init()
    err = capfd.readouterr().err
    assert "Failed to load the model" not in err, err
    if gpu_available():
        assert r == plugin.SUCCESS
        assert len(s.state_names) == 8
        assert sorted(s.command_names) == ["joint1/position", "joint1/velocity", "joint2/position", "joint2/velocity"]
        s.close()
    else:
        assert r == plugin.ERROR and "Could not create the simulation batch" in err
