"""The packed image of the step kernel's workgroup-shared tables (devtables.h pack_shared_image;
sim.table_image / mrs_debug_table_image, no device): every launch copies it into LDS at DevModel::shr_off, so
it has to be exactly what the table-by-table staging puts there -- each table (sim.staged_table, as the model
block holds it) at its shr_* offset, rfray as floats 0..3 of each ray's 8, the jump table as int bits, the
static ray hits' extent left for the device -- and nothing else but zero padding to a multiple of 4."""
from pathlib import Path

import numpy as np
import pytest

from mujoco_ros2_simulation_amd import sim

ROOT = Path(__file__).resolve().parents[1]
SWITCHES = ["MRS_GROUP", "MRS_G16_WPB", "MRS_G16_ONE_WG", "MRS_RAY_HELPERS", "MRS_NO_FUSE_IH", "MRS_NO_RAY_SWEEP",
            "MRS_NO_STATIC_RAYS", "MRS_NO_STATIC_FRAME", "MRS_NO_TABLE_IMAGE", "MRS_NO_PAIR_PRUNE"]


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def chain_xml(nv: int) -> str:
    """a serial chain of nv hinges with a position actuator and two sensors per joint, no rangefinder"""
    body, close, act, sens = "", "", "", ""
    for j in range(nv):
        axis = "0 0 1" if j % 2 == 0 else "0 1 0"
        body += (f'<body name="l{j}" pos="0 0 0.15"><joint name="j{j}" axis="{axis}" damping="0.5" armature="0.02" '
                 f'frictionloss="0.1"/><geom type="capsule" fromto="0 0 0 0.05 0 0.15" size="0.03" contype="0" '
                 f'conaffinity="0"/>')
        close += "</body>"
        act += f'<position name="a{j}" joint="j{j}" kp="200"/>'
        sens += f'<jointpos joint="j{j}"/><jointvel joint="j{j}"/>'
    return (f'<mujoco model="chain{nv}"><compiler angle="radian" autolimits="true"/>'
            f'<option timestep="0.002" integrator="implicitfast" solver="PGS" iterations="50"/>'
            f'<worldbody>{body}{close}</worldbody><actuator>{act}</actuator><sensor>{sens}</sensor></mujoco>')


ODD_NV = 3  # the chain whose tables end at a float count that is no multiple of 4 (asserted below)


def load(name: str):
    if name == "ref2dof":
        return sim.Model.load(ROOT / "tests" / "golden" / "ref_scenes" / "scene.xml")
    if name == "odd":
        return sim.Model.from_string(chain_xml(ODD_NV))
    return sim.Model.load(ROOT / "scenes" / f"{name}.xml")


def expected_image(model, ti: dict) -> np.ndarray:
    """the tables placed at their offsets the way step.hip's stage_tables stages them"""
    off, n = ti["offsets"], ti["copied"]
    want = np.zeros(len(ti["image"]), dtype=np.float32)
    names = sim.IMAGE_TABLES + ["end"]
    for k, name in enumerate(sim.IMAGE_TABLES):
        lo, hi = off[name], min(off[names[k + 1]], n)
        if name == "rf_static" or hi <= lo:
            continue
        t = sim.staged_table(model, name)
        if name == "rfray":
            i = np.arange(hi - lo)
            want[lo:hi] = t[8 * (i >> 2) + (i & 3)]
        else:
            assert len(t) >= hi - lo, (name, len(t), hi - lo)
            want[lo:hi] = t[:hi - lo]
    return want


def check(model, n_envs: int, cus: int = 256) -> dict:
    ti = sim.table_image(model, n_envs, cus)
    img, off, n = ti["image"], ti["offsets"], ti["copied"]
    assert len(img) == (n + 3) // 4 * 4
    order = [off[t] for t in sim.IMAGE_TABLES] + [off["end"]]
    assert order == sorted(order) and order[0] == 0
    assert n == (off["actrec"] if ti["blocked"] else off["end"])
    assert off["shared_floats"] == sim.plan_layout(model, n_envs, cus)["shared_floats"]
    assert off["shared_floats"] == (off["actrec"] if ti["blocked"] else off["end"] + 4)
    # bit for bit (the int-bit entries are NaN patterns or denormals as floats)
    assert np.array_equal(img.view(np.uint32), expected_image(model, ti).view(np.uint32))
    assert not img[n:].any()
    return ti


@pytest.mark.parametrize("scene,envs", [("arm7_lidar", 8192), ("arm7_lidar", 20), ("ref2dof", 4096), ("mobile_base", 2048)])
def test_image_is_the_tables_at_their_offsets(scene, envs):
    ti = check(load(scene), envs)
    assert not ti["blocked"] and ti["copied"] > 0


def test_c3_image_has_the_ray_table_and_the_static_hits_extent():
    model = load("arm7_lidar")
    ti = check(model, 8192)
    off = ti["offsets"]
    nrf = len(sim.staged_table(model, "rfray")) // 8
    assert nrf > 0 and off["rf_static"] - off["rfray"] == 4 * nrf  # the common-frame ray table, 4 of 8 floats
    assert off["rfblk"] - off["rf_static"] == nrf                  # static ray split: one hit per ray ...
    assert not ti["image"][off["rf_static"]:off["rfblk"]].any()    # ... zero until the device writes them
    # about 12 KB for C3: three 16-byte loads per thread of a 256-thread workgroup
    assert 2048 < ti["copied"] <= 3 * 4 * 256


def test_blocked_image_ends_at_the_actuator_table():
    ti = check(load("arm_boxes"), 8192)
    assert ti["blocked"] == 1 and ti["copied"] == ti["offsets"]["actrec"] < ti["offsets"]["end"]


def test_tail_of_an_image_that_is_no_multiple_of_four():
    ti = check(load("odd"), 17)
    assert ti["copied"] % 4 != 0 and len(ti["image"]) == ti["copied"] + 4 - ti["copied"] % 4


def test_model_without_rangefinders_has_empty_ray_extents():
    ti = check(load("odd"), 17)
    off = ti["offsets"]
    assert off["rfray"] == off["rf_static"] == off["rfblk"] == off["sensrec"]


def test_image_is_packed_whatever_the_switch_says(monkeypatch):
    """MRS_NO_TABLE_IMAGE=1 changes what a batch uploads, not the plan or the packing"""
    model = load("arm7_lidar")
    first = sim.table_image(model, 8192, 256)
    monkeypatch.setenv("MRS_NO_TABLE_IMAGE", "1")
    again = sim.table_image(model, 8192, 256)
    assert first["offsets"] == again["offsets"] and np.array_equal(first["image"].view(np.uint32), again["image"].view(np.uint32))


def test_bad_arguments():
    model = load("ref2dof")
    L = sim.lib()
    assert L.mrs_debug_table_image(None, 8, 256, 0, None, 0, None, 0) == -1
    assert L.mrs_debug_table_image(model.handle, 0, 256, 0, None, 0, None, 0) == -1
    assert L.mrs_debug_table_image(model.handle, 8, 256, 0, None, 4, None, 0) == -1
    assert L.mrs_debug_staged_table(model.handle, 0, 14, None, 0) == -1
    assert L.mrs_debug_staged_table(None, 0, 0, None, 0) == -1
