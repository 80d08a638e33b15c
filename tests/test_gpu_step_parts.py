"""The two step-kernel parts no other test launches: the G = 8 kernels, without and with the per-env
model parameter reads (build.py STEP_PARTS g8 / g8_prm; every other part has a test that forces its
group, layout, solver or parameters).  Each on the smallest scene that reaches it, 4 envs and 2 steps
against the fp64 oracle, with the bar of the nearest parity test of the scene's family: qpos / qvel
within 1e-5 x max(1, |ref|) (test_gpu_parity.py test_rollout_parity on the reference 2-DoF scene;
test_gpu_model_params.py test_gains_and_damping on the 2-dof arm, each step from the batch's own state)."""
import numpy as np
import pytest

import binding
import model_param_scenes as mp
from conftest import REF_SCENE
from mujoco_ros2_simulation_amd import sim, synth

pytestmark = pytest.mark.gpu
N = 4


def _force_group8(monkeypatch):
    for k in ("MRS_G16_WPB", "MRS_RAY_HELPERS", "MRS_SPREAD", "MRS_NO_FUSE_IH"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MRS_GROUP", "8")


def _close(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    err, scale = float(np.max(np.abs(got - want))), max(1.0, float(np.max(np.abs(want))))
    print(f"{name:6s} max |err| {err:.2e}  scale {scale:.3g}  rel {err / scale:.2e}")
    assert err <= 1e-5 * scale, (name, err, scale)


def test_group8_matches_oracle(monkeypatch):
    _force_group8(monkeypatch)
    model = sim.Model.load(REF_SCENE)
    envs = np.arange(N)
    qpos0 = synth.initial_qpos(model, envs)
    ctrl = synth.ctrl_table(model, envs, 1, 10)[0]
    b = sim.Batch(model, N)
    assert b.layout()["group"] == 8, b.layout()
    b.set(sim.FIELD_QPOS, qpos0)
    b.set(sim.FIELD_CTRL, ctrl)
    b.step(2)
    ref = []
    for e in range(N):
        d = binding.OracleData(model)
        d.qpos[:] = qpos0[e]
        d.ctrl[:] = ctrl[e]
        d.step(2)
        ref.append(d)
    _close("qpos", b.get(sim.FIELD_QPOS), [d.qpos for d in ref])
    _close("qvel", b.get(sim.FIELD_QVEL), [d.qvel for d in ref])
    b.close()


def test_group8_params_match_oracle(monkeypatch):
    _force_group8(monkeypatch)
    values = mp.arm_values(N, 2)
    model = mp.model_of(mp.arm_scene, mp.ARM_BASE)
    qpos, qvel, ctrl = mp.arm_state(N, 2)
    b = sim.Batch(model, N)
    assert b.layout()["group"] == 8, b.layout()
    b.set(sim.FIELD_QPOS, qpos)
    b.set(sim.FIELD_QVEL, qvel)
    b.set(sim.FIELD_CTRL, ctrl)
    mp.set_all(b, mp.env_rows(mp.arm_scene, values))
    for _ in range(2):
        q, v, w = b.get(sim.FIELD_QPOS), b.get(sim.FIELD_QVEL), b.get(sim.FIELD_QACC_WARMSTART)
        b.step(1)
        ref = []
        for e in range(N):
            d = mp.oracle(mp.arm_scene, values[e], q[e], v[e], ctrl[e], w[e])
            d.step(1)
            ref.append(d)
        _close("qpos", b.get(sim.FIELD_QPOS), [d.qpos for d in ref])
        _close("qvel", b.get(sim.FIELD_QVEL), [d.qvel for d in ref])
    b.close()
