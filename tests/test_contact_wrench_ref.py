"""Pins tests/contact_wrench_ref.py (CPU, fp64): a closed form on a dropped sphere, and on two contact
scenes the identity that the wrenches, taken as xfrc_applied, are the constraint force of the contact rows."""
import numpy as np

import binding
from conftest import ARM7
from contact_wrench_ref import SPHERE, SPHERE_M, contact_wrench, sphere_known, sphere_start
from mujoco_ros2_simulation_amd import sim, synth
from sensor_ref import EFC_CONTACT
from sensor_scenes import FLOAT, bare, float_start
from xfrc_ref import G, XfrcRef

ARM_BOXES = ARM7.parent / "arm_boxes.xml"


def test_sphere_closed_form():
    """a free sphere dropped onto the floor with a tangential velocity and a spin, pyramidal and elliptic:
    at every step in contact the sphere's row is m (a_lin + g) and I R alpha of the oracle's own qacc, and
    the world's row the negated force.  qacc = qacc_smooth + M^-1 J' f holds for the solver's f whatever
    its convergence, and gravity is the only smooth force, so the bar is fp64 round-off: 1e-9 of m g."""
    for option in ("", ' cone="elliptic"'):
        model = sim.Model.from_string(SPHERE % {"option": option})
        xr = XfrcRef(model)
        d = binding.OracleData(model)
        d.qpos[:], d.qvel[:] = sphere_start(model, 1)
        seen = 0
        for _ in range(12):
            d.forward()
            forces, W = contact_wrench(model, d, xr.frames(d.qpos)[0])
            if d.ncon:
                seen += 1
                want = sphere_known(d.qpos, d.qacc)
                assert forces.shape == (1, 6) and forces[0, 0] > 0 and np.any(forces[0, 1:3] != 0)
                assert not forces[:, 3:].any()
                np.testing.assert_allclose(W[1], want, rtol=0, atol=1e-9 * SPHERE_M * G)
                np.testing.assert_allclose(W[0, :3], -W[1, :3], rtol=0, atol=0)
                assert np.linalg.norm(want[3:]) > 1e-4  # (friction spins the sphere: the torque is tested)
            else:
                assert not W.any()
            d.step()
        assert seen >= 3


def _identity(model, d, xr, settle):
    for _ in range(settle):
        d.step()
    worst, checked = 0.0, 0
    for _ in range(5):
        d.forward()
        qpos = d.qpos.copy()
        forces, W = contact_wrench(model, d, xr.frames(qpos)[0])
        efc = d.efc()
        rows = np.flatnonzero(efc["type"] == EFC_CONTACT)
        want = efc["J"][rows].T @ efc["force"][rows]
        got = xr.qfrc(qpos, W)
        if len(rows):
            checked += 1
            # test_xfrc_ref.py pins XfrcRef.qfrc to 1e-8 under wrenches of order one; its error (the
            # central differences' round-off and truncation) is linear in the wrench
            bar = 1e-8 * max(1.0, float(np.max(np.abs(W))))
            worst = max(worst, float(np.max(np.abs(got - want))) / bar)
            np.testing.assert_allclose(got, want, rtol=0, atol=bar)
            np.testing.assert_allclose(W[:, :3].sum(axis=0), 0, rtol=0, atol=1e-12 * max(1.0, float(np.abs(W).max())))
        d.step()
    print(f"identity: worst error {worst:.2e} of its bar over {checked} states")
    assert checked >= 3


def test_identity_landing_box():
    """sum_b J_b(xipos_b)' W_b == sum over contact rows J_r' f_r on the landing box with its flap"""
    model = sim.Model.from_string(bare(FLOAT))
    d = binding.OracleData(model)
    d.qpos[:], d.qvel[:] = float_start(model, 3)
    _identity(model, d, XfrcRef(model), settle=42)  # (touchdown: two contacts, then three, then four)


def test_identity_arm_boxes():
    """the same on the 7-DoF arm with 8 free boxes after 20 settle steps (box-floor and box-box contacts)"""
    model = sim.Model.from_string(ARM_BOXES.read_text(), str(ARM_BOXES.parent))
    d = binding.OracleData(model)
    d.qpos[:] = synth.initial_qpos(model, np.arange(1))[0]
    _identity(model, d, XfrcRef(model), settle=20)
