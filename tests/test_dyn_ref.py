"""Pins the analytic site Jacobian of tests/dyn_ref.py against central differences of the oracle's own site
framepos / framequat sensors, before the kernel is compared with it.  CPU only.

EPS = 1e-4: a site's position is a composition of rotations about anchors at most ~2 m away, so the third
derivative along a unit tangent is below ~2 and the central difference's truncation eps^2 |p'''| / 6 is
below 4e-9; the fp64 rounding 2^-52 |p| / eps is ~5e-12.  Both are far below the 1e-7 the test asks."""
import numpy as np
import pytest

import binding
import dyn_ref
from conftest import REF_SCENE
from mujoco_ros2_simulation_amd import sim
from sensor_ref import integrate_pos, quat2mat

EPS = 1e-4
TOL = 1e-7


def _ref_arm():
    xml = REF_SCENE.read_text()
    i = xml.rindex("</mujoco>")
    sens = "".join(f'<framepos objtype="site" objname="{s}"/><framequat objtype="site" objname="{s}"/>'
                   for s in ("ee_link", "camera_color_optical_frame"))
    model = sim.Model.from_string(xml[:i] + f"<sensor>{sens}</sensor>" + xml[i:], str(REF_SCENE.parent))
    return model, ["ee_link", "camera_color_optical_frame"], np.array([0.7, -1.1])


def _ball_free():
    model = sim.Model.from_string(dyn_ref.BALL_FREE)
    q = np.array([0.7, 0.1, -0.5, 0.5, 0.5, -0.3, 0.6, 0.4, 0.6, -0.2, 0.65])
    q[:4] /= np.linalg.norm(q[:4])
    q[7:] /= np.linalg.norm(q[7:])
    return model, ["tip", "corner"], q


def _frame_sensors(model, d, name):
    """(pos, R) of the site's framepos / framequat sensors"""
    sid = model.name2id(sim.OBJ_SITE, name)
    out = {}
    for i in range(model.nsensor):
        if model.sensor_objid[i] == sid and model.sensor_type[i] in (sim.SENS_FRAMEPOS, sim.SENS_FRAMEQUAT):
            out[int(model.sensor_type[i])] = d.sensordata[model.sensor_adr[i]:model.sensor_adr[i] + model.sensor_dim[i]].copy()
    return out[sim.SENS_FRAMEPOS], quat2mat(out[sim.SENS_FRAMEQUAT])


@pytest.mark.parametrize("scene", [_ref_arm, _ball_free])
def test_site_jacobian_against_central_differences(built, scene):
    model, names, qpos = scene()
    ids = [model.name2id(sim.OBJ_SITE, s) for s in names]
    d = binding.OracleData(model)
    d.qpos[:] = qpos
    J = dyn_ref.site_jac_ref(model, d, ids)
    pose = dyn_ref.site_pose_ref(model, d, ids)
    d.forward()
    for k, name in enumerate(names):  # the pose reference is the sensors' own value
        p, R = _frame_sensors(model, d, name)
        np.testing.assert_allclose(pose[k, :3], p, rtol=0, atol=1e-12)
        np.testing.assert_allclose(pose[k, 3:].reshape(3, 3), R, rtol=0, atol=1e-12)
    for j in range(model.nv):
        e = np.zeros(model.nv)
        e[j] = 1.0
        side = []
        for sg in (1, -1):
            d.qpos[:] = integrate_pos(model, qpos, e, sg * EPS)  # the dof's tangent: a quaternion step for ball / free
            d.forward()
            side.append([_frame_sensors(model, d, s) for s in names])
        for k in range(len(names)):
            (pp, Rp), (pm, Rm) = side[0][k], side[1][k]
            np.testing.assert_allclose(J[k, :3, j], (pp - pm) / (2 * EPS), rtol=0, atol=TOL)
            # the relative rotation's logarithm: vee of the skew part is sin(angle) * axis, angle = 2 EPS |jacr|
            S = Rp @ Rm.T
            w = np.array([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]]) / 2
            n = np.linalg.norm(w)
            w = w * (np.arcsin(n) / n if n > 0 else 1.0)
            np.testing.assert_allclose(J[k, 3:, j], w / (2 * EPS), rtol=0, atol=TOL)


def test_other_tree_columns_are_zero(built):
    model, names, qpos = _ball_free()
    ids = [model.name2id(sim.OBJ_SITE, s) for s in names]
    d = binding.OracleData(model)
    d.qpos[:] = qpos
    J = dyn_ref.site_jac_ref(model, d, ids)
    assert np.all(J[0, :, 3:] == 0) and np.all(J[1, :, :3] == 0)
    assert np.all(np.abs(J[0, :, :3]).sum(axis=0) > 0) and np.all(np.abs(J[1, :, 3:]).sum(axis=0) > 0)


def test_bias_twin_is_minus_qfrc_smooth_of_gravity_alone(built):
    """at rest the bias of the ball pendulum + free box is gravity's: the free box's translational dofs read
    m g on z"""
    model, _, qpos = _ball_free()
    b = dyn_ref.bias_ref(dyn_ref.BALL_FREE, qpos, np.zeros(model.nv))
    np.testing.assert_allclose(b[3:6], [0, 0, 2 * 9.81], rtol=0, atol=1e-12)
