"""Mocap bodies on the CPU: the compiled fields, keyframes, rejections, what the oracle (which steps a mocap
body as a static one at its compiled pose) makes of such a model, the choices the GPU tests rest on, and
the C ABI."""
import re
import subprocess

import numpy as np
import pytest

import binding
import mocap_scenes as ms
from conftest import ROOT
from mujoco_ros2_simulation_amd import sim

TWO = """<mujoco><worldbody>
  <body name="a" pos="0 0 1"><joint/><geom size="0.1"/></body>
  <body name="m0" mocap="true" pos="1 2 3" quat="0 0 2 0"><geom size="0.1"/></body>
  <body name="b" pos="0 1 1"><joint/><geom size="0.1"/><body name="b2" pos="0 0 0.3"><joint/><geom size="0.05"/></body></body>
  <body name="m1" mocap="true" pos="-1 0 0.5"><site name="s"/><body name="child" pos="0 0 0.2"><geom size="0.05"/></body></body>
  <body name="plain" mocap="false" pos="3 0 0"><geom size="0.1"/></body>
</worldbody>%s</mujoco>"""


def test_compiled_fields():
    m = sim.Model.from_string(TWO % "")
    assert m.nmocap == 2 and m.nkey == 0
    assert m.body_mocapid.tolist() == [-1, -1, 0, -1, -1, 1, -1, -1]
    assert m.body_weldid[2] == 0 and m.body_weldid[5] == 0 and m.body_weldid[6] == 0
    assert m.key_mpos.shape == (0, 6) and m.key_mquat.shape == (0, 8)
    assert np.array_equal(m.body_quat[2], [0, 0, 1, 0])  # (the start pose is normalised like any body's)


def test_keyframes():
    keys = ('<keyframe><key qpos="0.1 0.2 0.3" mpos="1 1 1 2 2 2" mquat="0 1 0 0 0.5 0.5 0.5 0.5"/>'
            '<key qpos="0.3 0.2 0.1"/></keyframe>')
    m = sim.Model.from_string(TWO % keys)
    assert m.nkey == 2
    assert m.key_mpos[0].tolist() == [1, 1, 1, 2, 2, 2] and m.key_mquat[0].tolist() == [0, 1, 0, 0, 0.5, 0.5, 0.5, 0.5]
    assert m.key_mpos[1].tolist() == [1, 2, 3, -1, 0, 0.5] and m.key_mquat[1].tolist() == [0, 0, 1, 0, 1, 0, 0, 0]
    with pytest.raises(sim.MrsError, match="'mpos' has wrong size"):
        sim.Model.from_string(TWO % '<keyframe><key mpos="1 1 1"/></keyframe>')
    with pytest.raises(sim.MrsError, match="'mquat' has wrong size"):
        sim.Model.from_string(TWO % '<keyframe><key mquat="1 0 0 0"/></keyframe>')


@pytest.mark.parametrize("body, message", [
    ('<body name="p" pos="0 0 1"><joint/><geom size="0.1"/><body mocap="true"><geom size="0.1"/></body></body>',
     "mocap body must be a child of the world"),
    ('<body name="p" mocap="true"><joint/><geom size="0.1"/></body>', "cannot have joints"),
    ('<body name="p" mocap="true"><geom size="0.1"/><light pos="0 0 1"/></body>', "lights on or below mocap bodies"),
    ('<body name="p" mocap="true"><geom size="0.1"/><body pos="0 0 1"><light pos="0 0 1"/></body></body>',
     "lights on or below mocap bodies"),
])
def test_rejections(body, message):
    with pytest.raises(sim.MrsError, match=message):
        sim.Model.from_string(f"<mujoco><worldbody>{body}</worldbody></mujoco>")


def test_mocap_false_loads_as_before():
    xml = ('<mujoco><worldbody><body %s pos="0 0 1"><geom size="0.1"/><light pos="0 0 1"/>'
           '<body pos="0 0 1"><joint/><geom size="0.1"/></body></body></worldbody></mujoco>')
    a, b = sim.Model.from_string(xml % 'mocap="false"'), sim.Model.from_string(xml % "")
    assert a.nmocap == 0 and a.body_mocapid.tolist() == [-1, -1, -1] and a.nlight == 1
    assert np.array_equal(a.body_pos, b.body_pos) and a.nq == b.nq == 1


def test_oracle_steps_a_mocap_model_as_static():
    pos, quat = ms.poses(2, 3, [0.5, 0.3, 1.2])
    models = [ms.model_of(ms.arm_scene, (pos[e], quat[e]), actuator='<actuator><motor joint="j1" gear="2"/></actuator>')
              for e in range(2)]
    for e, m in enumerate(models):
        d = binding.OracleData(m)
        d.step(50)
        assert np.all(np.isfinite(d.qpos)) and np.all(np.isfinite(d.sensordata))
        q = quat[e] / np.linalg.norm(quat[e])
        want = pos[e] + ms.rot(q, np.array([0.05, 0.02, 0.1]))
        assert np.allclose(d.sensordata[:3], want, rtol=0, atol=1e-14)
        assert np.allclose(d.sensordata[10:13], pos[e], rtol=0, atol=1e-14)
    # no other compiled constant depends on a static body's pose
    a, b = models
    for name in ("body_invweight0", "dof_invweight0", "actuator_gainprm", "actuator_biasprm", "actuator_gear",
                 "actuator_ctrlrange", "actuator_forcerange", "actuator_trnid", "body_mocapid"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_weld_pull_shows_in_the_oracle_alone():
    """the GPU weld test's start offset: over 20 steps of a moving target the oracle's body closes in"""
    pos, quat = ms.poses(5, 4, [0.0, 0.0, 1.0], tilt=0.0)
    for e in range(5):
        first, last = ms.weld_oracle_distances(pos[e], quat[e], np.array([0.05, -0.03, 0.04]))
        assert last < 0.8 * first, (e, first, last)


@pytest.mark.parametrize("on_mocap", [False, True])
def test_lidar_poses_are_away_from_silhouettes(on_mocap):
    """every ray hits something, the box is hit by some, and no 1e-4 nudge of the pose changes a ray's geom"""
    pos, quat = ms.lidar_poses(on_mocap)
    for e in range(5):
        base = ms.ray_geoms(ms.model_of(ms.lidar_scene, (pos[e], quat[e]), on_mocap=on_mocap))
        assert np.all(base >= 0), (e, base)
        obst = ms.model_of(ms.lidar_scene, (pos[e], quat[e]), on_mocap=on_mocap).name2id(sim.OBJ_GEOM, "obst")
        assert np.any(base == obst), (e, base)
        for k in range(3):
            for sgn in (-1e-4, 1e-4):
                p = pos[e].copy()
                p[k] += sgn
                assert np.array_equal(ms.ray_geoms(ms.model_of(ms.lidar_scene, (p, quat[e]), on_mocap=on_mocap)), base), (e, k)
        for sgn in (-1e-4, 1e-4):
            q = ms.quat_mul(quat[e], ms.axis_quat([0, 1, 0], sgn))
            assert np.array_equal(ms.ray_geoms(ms.model_of(ms.lidar_scene, (pos[e], q), on_mocap=on_mocap)), base), e


def test_camera_poses_keep_silhouettes_under_the_cap():
    pos, quat = ms.camera_poses()
    for e in range(5):
        img = ms.oracle_frame((pos[e], quat[e]))
        sil = ms.silhouette(img)
        assert 0 < sil.mean() <= 0.02, (e, sil.mean())
        assert img.max() - img.min() > 0.035  # (the slab, 0.04 high, is in view)


def test_header_and_symbols():
    text = (ROOT / "include" / "mrs.h").read_text()
    assert re.search(r"MRS_FIELD_COUNT\s*=\s*13\b", text)
    out = subprocess.run(["nm", "-D", "--defined-only", str(sim.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    for name in ("mrs_batch_set_mocap", "mrs_batch_get_mocap", "mrs_batch_mocap_pos_device_ptr",
                 "mrs_batch_mocap_quat_device_ptr"):
        assert re.search(rf"\bT {name}\b", out), name
