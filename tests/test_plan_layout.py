"""The launch plan without a device: sim.plan_layout (mrs_debug_plan_layout) builds the model's tables and
chooses the plan on the host (csrc/hip/devtables.h, plan.h), so what the GPU tests pin through
Batch.layout() -- C3 on 16 lanes with four-wave workgroups, C4 on one-wave workgroups with helpers, C5
blocked -- is pinned here on a CPU-only box too, for a device with 256 compute units."""
from pathlib import Path

import pytest

from mujoco_ros2_simulation_amd import sim

ROOT = Path(__file__).resolve().parents[1]
ERR_INVALID, ERR_UNSUPPORTED = -1, -4  # include/mrs.h
SWITCHES = ["MRS_GROUP", "MRS_G16_WPB", "MRS_G16_ONE_WG", "MRS_RAY_HELPERS", "MRS_NO_FUSE_IH", "MRS_NO_RAY_SWEEP",
            "MRS_NO_STATIC_RAYS", "MRS_NO_STATIC_FRAME", "MRS_SENSORS_EVERY_STEP"]


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def models():
    return {s: sim.Model.load(ROOT / "scenes" / f"{s}.xml") for s in ("mobile_base", "arm7_lidar", "arm_boxes")}


@pytest.mark.parametrize("scene,envs,group,wpb,helpers", [
    ("mobile_base", 2048, 16, 1, 1), ("mobile_base", 3072, 16, 1, 0), ("arm7_lidar", 8192, 16, 4, 0)])
def test_plan_of_the_benchmark_batches(models, scene, envs, group, wpb, helpers):
    lay = sim.plan_layout(models[scene], envs, 256)
    assert list(lay) == sim.LAYOUT_KEYS and len(sim.LAYOUT_KEYS) == 16
    assert (lay["group"], lay["waves_per_workgroup"], lay["helper_waves"]) == (group, wpb, helpers), lay


def test_c5_is_blocked(models):
    lay = sim.plan_layout(models["arm_boxes"], 8192, 256)
    assert lay["blocked"] == 1 and lay["group"] == 64 and lay["waves_per_workgroup"] == 0, lay


def test_switches_are_read_at_every_call(models, monkeypatch):
    m = models["mobile_base"]
    first = sim.plan_layout(m, 2048, 256)
    assert (first["group"], first["waves_per_workgroup"], first["helper_waves"]) == (16, 1, 1)
    monkeypatch.setenv("MRS_RAY_HELPERS", "0")
    assert sim.plan_layout(m, 2048, 256)["helper_waves"] == 0
    monkeypatch.setenv("MRS_G16_WPB", "4")
    assert sim.plan_layout(m, 2048, 256)["waves_per_workgroup"] == 4
    monkeypatch.setenv("MRS_GROUP", "32")
    lay = sim.plan_layout(m, 2048, 256)
    assert lay["group"] == 32 and lay["waves_per_workgroup"] == 0, lay
    for k in ("MRS_RAY_HELPERS", "MRS_G16_WPB", "MRS_GROUP"):
        monkeypatch.delenv(k)
    assert sim.plan_layout(m, 2048, 256) == first


def test_unknown_cu_count_keeps_four_wave_workgroups(models, monkeypatch):
    # cu_count <= 0 is a failed device query: no one-wave workgroups (so no helper waves either), and
    # the helper decision's fit test passes, which shows once MRS_G16_WPB asks for one-wave workgroups
    lay = sim.plan_layout(models["mobile_base"], 2048, 0)
    assert lay["waves_per_workgroup"] == 4 and lay["helper_waves"] == 0, lay
    monkeypatch.setenv("MRS_G16_WPB", "1")
    assert sim.plan_layout(models["mobile_base"], 8192, 0)["helper_waves"] == 1
    assert sim.plan_layout(models["mobile_base"], 8192, 256)["helper_waves"] == 0  # (2048 waves > 2 x 256)


def test_unsupported_models_are_refused_without_a_device():
    bodies = "".join(f'<body pos="{i} 0 1"><freejoint/><geom size="0.1"/></body>' for i in range(11))
    m = sim.Model.from_string(f"<mujoco><worldbody>{bodies}</worldbody></mujoco>")
    assert m.nv == 66
    with pytest.raises(sim.MrsError) as e:
        sim.plan_layout(m, 64, 256)
    assert e.value.code == ERR_UNSUPPORTED and "nv > 64" in str(e.value)
    # (a height-field collision pair cannot be loaded from MJCF, which refuses the geom type; the
    # sanitizer driver makes one in a compiled model and checks the same error: tests/sanitize/driver.cc)


def test_bad_arguments(models):
    with pytest.raises(sim.MrsError) as e:
        sim.plan_layout(models["arm7_lidar"], 0, 256)
    assert e.value.code == ERR_INVALID
    assert sim.lib().mrs_debug_plan_layout(None, 64, 256, 0, None, 16) == ERR_INVALID
