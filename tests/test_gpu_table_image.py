"""The launch prologue's table image on the device (step.hip stage_table_image; DevModel::shr_image): a
batch that copies the packed image into LDS computes exactly what a batch created under
MRS_NO_TABLE_IMAGE=1 computes, which stages table by table (stage_tables, the former prologue).  The LDS
contents are the same floats either way, and nothing in the step loop differs, so every output is compared
bit for bit; no case needs the oracle (the rest of the GPU suite compares the default mode with it)."""
from pathlib import Path

import numpy as np
import pytest

from mujoco_ros2_simulation_amd import sim
from test_table_image import ODD_NV, chain_xml

ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu

FIELDS = {"qpos": sim.FIELD_QPOS, "qvel": sim.FIELD_QVEL, "qacc": sim.FIELD_QACC,
          "qacc_warmstart": sim.FIELD_QACC_WARMSTART, "sensordata": sim.FIELD_SENSORDATA,
          "ncon": sim.FIELD_NCON, "niter": sim.FIELD_SOLVER_NITER, "warning": sim.FIELD_WARNING}
SWITCHES = ["MRS_GROUP", "MRS_G16_WPB", "MRS_RAY_HELPERS", "MRS_NO_SOLVE_FUSE"]


def rollout(monkeypatch, image: bool, make_model, n: int, launches, env: dict, expect: dict, poke=None):
    """the FIELDS after every launch (launches: steps of each) of a seeded rollout; poke(k, batch) may edit
    the batch before launch k"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if image:
        monkeypatch.delenv("MRS_NO_TABLE_IMAGE", raising=False)
    else:
        monkeypatch.setenv("MRS_NO_TABLE_IMAGE", "1")
    model = make_model()
    b = sim.Batch(model, n)
    lay = b.layout()
    assert lay["table_image"] == int(image), lay
    assert {k: lay[k] for k in expect} == expect, lay
    rng = np.random.default_rng(7)
    qpos = b.get(sim.FIELD_QPOS)
    qpos[:, :] += rng.uniform(-0.02, 0.02, qpos.shape).astype(np.float32)
    b.set(sim.FIELD_QPOS, qpos)
    out = []
    for k, steps in enumerate(launches):
        if model.nu:
            b.set(sim.FIELD_CTRL, rng.uniform(-1, 1, (n, model.nu)).astype(np.float32))
        if poke:
            poke(k, b)
        b.step(steps)
        out.append({name: b.get(f).copy() for name, f in FIELDS.items()})
    b.close()
    return out


def assert_same_bits(monkeypatch, make_model, n, launches, env=None, expect=None, poke=None):
    on = rollout(monkeypatch, True, make_model, n, launches, env or {}, expect or {}, poke)
    off = rollout(monkeypatch, False, make_model, n, launches, env or {}, expect or {}, poke)
    for k, (x, y) in enumerate(zip(on, off)):
        for name in FIELDS:
            u, v = np.asarray(x[name]), np.asarray(y[name])
            assert np.array_equal(u, v, equal_nan=True), (k, name, np.nanmax(np.abs(u.astype(np.float64) - v)))
    return on


def scene(name: str):
    return lambda: sim.Model.load(ROOT / "scenes" / f"{name}.xml")


def test_c3_two_workgroups_the_second_partial(monkeypatch):
    """arm7_lidar at 20 envs on four-wave workgroups (16 envs each); 12 steps as launches of 5 and 7"""
    on = assert_same_bits(monkeypatch, scene("arm7_lidar"), 20, [5, 7], env={"MRS_G16_WPB": "4"},
                          expect={"group": 16, "waves_per_workgroup": 4, "helper_waves": 0, "ray_sweep": 1})
    assert np.any(on[-1]["sensordata"] > 0) and np.all(np.isfinite(on[-1]["qpos"]))


def test_reference_scene_2dof_newton(monkeypatch):
    base = ROOT / "tests" / "golden" / "ref_scenes"
    on = assert_same_bits(monkeypatch, lambda: sim.Model.load(base / "scene.xml"), 5, [5, 7], expect={"group": 16})
    assert np.all(np.isfinite(on[-1]["qpos"]))


def test_mobile_base_on_the_helper_wave_kernels(monkeypatch):
    on = assert_same_bits(monkeypatch, scene("mobile_base"), 8, [5, 7],
                          expect={"group": 16, "waves_per_workgroup": 1, "helper_waves": 1})
    assert np.any(on[-1]["sensordata"] != 0) and not np.any(on[-1]["warning"])


def test_arm_boxes_blocked(monkeypatch):
    on = assert_same_bits(monkeypatch, scene("arm_boxes"), 3, [5, 7], expect={"group": 64, "blocked": 1})
    assert np.all(on[-1]["ncon"] > 0)


def test_image_length_no_multiple_of_four(monkeypatch):
    model = sim.Model.from_string(chain_xml(ODD_NV))
    assert sim.table_image(model, 17, 256)["copied"] % 4 != 0
    on = assert_same_bits(monkeypatch, lambda: sim.Model.from_string(chain_xml(ODD_NV)), 17, [5, 7], expect={"group": 16})
    assert np.all(on[-1]["niter"] >= 1)


def test_set_param_and_set_inertial_between_launches(monkeypatch):
    """per-env parameters and inertias go to their own rows, not to the staged tables: the image stays
    coherent with the tables after them (and the launches take the parameter kernels from then on)"""
    def poke(k, b):
        n, m = b.n, b.model
        if k == 1:
            b.set_model_param(sim.PARAM_DOF_DAMPING, np.linspace(0.2, 1.5, n * m.nv).reshape(n, m.nv))
            b.set_model_param(sim.PARAM_ACT_GAINPRM, np.array([[150.0, 0, 0]] * m.nu), env0=2)
        if k == 2:
            mass, _, arm = b.get_inertial()
            b.set_inertial(mass=mass * np.linspace(0.8, 1.3, n)[:, None], armature=arm * 1.5)

    on = assert_same_bits(monkeypatch, lambda: sim.Model.from_string(chain_xml(5)), 8, [5, 7, 4], expect={"group": 16},
                          poke=poke)
    assert not np.array_equal(on[1]["qvel"][0], on[1]["qvel"][7])
