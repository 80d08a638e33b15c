"""The frame plan without a device: sim.render_plan (mrs_debug_render_plan) reads the render switches and
chooses the depth kernel, its LDS, grid and frame chunk on the host (csrc/hip/renderplan.h), so which
kernel a frame gets -- also on the branches no switch selects -- is pinned on a CPU-only box.  Every
expected value is worked out from the conditions of the frame launch as they stood in batch.hip: the binned
kernel needs mesh geoms within its limits, W <= 2048, H <= 8 * 128, its band of W * 8 keys of 8 bytes within
the device's LDS and neither MRS_DEPTH_V1 nor MRS_DEPTH_V2; else the frame kernel needs at most 64 geoms
and no MRS_DEPTH_V1; else the tile kernel, one workgroup per 16 x 16 pixels.  Frames of the binned kernel
go in chunks of max(1, min(n, budget / per_frame)) with 8 bytes per (geom, triangle) pair per frame and a
budget of max(1, MRS_RAST_BUDGET_MB) MB, 2048 MB when unset."""
from pathlib import Path

import pytest

from mujoco_ros2_simulation_amd import sim

ROOT = Path(__file__).resolve().parents[1]
ERR_INVALID, ERR_UNSUPPORTED = -1, -4  # include/mrs.h
SWITCHES = ["MRS_DEPTH_V1", "MRS_DEPTH_V2", "MRS_RAST_BUDGET_MB"]
MB = 1 << 20
# scenes/arm7_mesh.xml: the statue's 6912 triangles and seven link shells of 1536, 8 bytes per pair
C3M_PER_FRAME = 8 * (6912 + 7 * 1536)


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def models():
    return {s: sim.Model.load(ROOT / "scenes" / f"{s}.xml") for s in ("mobile_base", "arm7_mesh")}


def spheres(count: int, res: str = "100 50") -> sim.Model:
    geoms = "".join(f'<geom size="0.05" pos="{0.2 * i} 0 0"/>' for i in range(count))
    return sim.Model.from_string(f'<mujoco><worldbody><camera pos="0 -3 0" xyaxes="1 0 0 0 0 1" resolution="{res}"/>'
                                 f"{geoms}</worldbody></mujoco>")


def mesh_scene(res: str, mesh: str = "link", count: int = 1) -> sim.Model:
    geoms = "".join(f'<geom type="mesh" mesh="m" pos="{i} 0 0"/>' for i in range(count))
    return sim.Model.from_string(
        f'<mujoco><asset><mesh name="m" file="meshes/{mesh}.obj"/></asset><worldbody>'
        f'<camera pos="0 -3 0" xyaxes="1 0 0 0 0 1" resolution="{res}"/>{geoms}</worldbody></mujoco>',
        basedir=str(ROOT / "scenes"))


def test_c4_takes_the_frame_kernel_without_mesh_code(models):
    m = models["mobile_base"]
    assert m.ngeom <= 64
    p = sim.render_plan(m, 0, 2048, 65536)
    assert (p["kernel"], p["mesh"], p["grid"]) == ("frame", False, (2048, 1)), p
    assert p["chunk"] >= 1


@pytest.mark.parametrize("n", [1, 2048])
def test_c3m_takes_the_binned_kernel(models, n):
    p = sim.render_plan(models["arm7_mesh"], 0, n, 65536)
    assert p["kernel"] == "binned" and p["mesh"] is True, p
    assert p["band_lds"] == 640 * 8 * 8
    assert p["per_frame"] == C3M_PER_FRAME
    assert p["chunk"] == min(n, (2048 * MB) // C3M_PER_FRAME) == n  # (the default budget holds 15196 frames)
    assert p["grid"] == (n, 1)


def test_c3m_under_the_switches(models, monkeypatch):
    m = models["arm7_mesh"]
    monkeypatch.setenv("MRS_DEPTH_V2", "1")
    p = sim.render_plan(m, 0, 64, 65536)
    assert (p["kernel"], p["mesh"], p["grid"]) == ("frame", True, (64, 1)), p
    monkeypatch.delenv("MRS_DEPTH_V2")
    monkeypatch.setenv("MRS_DEPTH_V1", "1")
    p = sim.render_plan(m, 0, 64, 65536)
    assert (p["kernel"], p["grid"]) == ("tile", (-(-640 // 16) * -(-480 // 16), 64)), p
    assert p["grid"][0] == 40 * 30
    monkeypatch.setenv("MRS_DEPTH_V2", "1")  # (both: MRS_DEPTH_V1 wins, as the frame kernel's condition excludes it)
    assert sim.render_plan(m, 0, 64, 65536)["kernel"] == "tile"


def test_more_than_64_geoms_take_the_tile_kernel():
    assert sim.render_plan(spheres(64), 0, 3, 65536)["kernel"] == "frame"
    p = sim.render_plan(spheres(65), 0, 3, 65536)
    assert (p["kernel"], p["mesh"], p["grid"]) == ("tile", False, (7 * 4, 3)), p  # (ceil(100 / 16) x ceil(50 / 16) tiles)
    assert sim.render_plan(spheres(256), 0, 1, 65536)["kernel"] == "tile"


def test_more_than_256_geoms_are_refused():
    with pytest.raises(sim.MrsError) as e:
        sim.render_plan(spheres(257), 0, 1, 65536)
    assert e.value.code == ERR_UNSUPPORTED and str(e.value).endswith("too many geoms for the depth kernel"), e.value


@pytest.mark.parametrize("res,max_lds,kernel", [
    ("2048 480", 163840, "binned"), ("2049 480", 163840, "frame"),           # W <= 2048
    ("640 1024", 65536, "binned"), ("640 1025", 65536, "frame"),             # H <= kBandH * kMaxBands = 8 * 128
    ("640 480", 640 * 64, "binned"), ("640 480", 640 * 64 - 1, "frame"),     # band_lds <= max_lds
    ("2048 480", 2048 * 64, "binned"), ("2048 480", 65536, "frame")])
def test_the_binned_kernel_falls_back_at_its_limits(res, max_lds, kernel):
    p = sim.render_plan(mesh_scene(res), 0, 4, max_lds)
    assert p["kernel"] == kernel and p["mesh"] is True, p
    assert p["band_lds"] == int(res.split()[0]) * 64 and p["per_frame"] == 8 * 1536


@pytest.mark.parametrize("value", ["1", "0", "-5"])
def test_the_budget_is_at_least_one_megabyte(models, monkeypatch, value):
    monkeypatch.setenv("MRS_RAST_BUDGET_MB", value)
    p = sim.render_plan(models["arm7_mesh"], 0, 2048, 65536)
    assert p["kernel"] == "binned" and p["chunk"] == MB // C3M_PER_FRAME == 7 and p["grid"] == (7, 1), p
    assert sim.render_plan(models["arm7_mesh"], 0, 3, 65536)["chunk"] == 3
    monkeypatch.setenv("MRS_RAST_BUDGET_MB", "2")
    assert sim.render_plan(models["arm7_mesh"], 0, 2048, 65536)["chunk"] == 2 * MB // C3M_PER_FRAME == 14


def test_chunk_is_never_below_one(monkeypatch):
    # twenty statues: one frame's list (8 x 20 x 6912 bytes) is larger than a 1 MB budget
    m = mesh_scene("64 48", "statue", 20)
    monkeypatch.setenv("MRS_RAST_BUDGET_MB", "1")
    for n in (1, 2, 2048):
        p = sim.render_plan(m, 0, n, 65536)
        assert p["per_frame"] == 8 * 20 * 6912 > MB
        assert p["kernel"] == "binned" and p["chunk"] == 1 and p["grid"] == (1, 1), p


def test_switches_are_read_at_every_call(models, monkeypatch):
    m = models["arm7_mesh"]
    first = sim.render_plan(m, 0, 2048, 65536)
    assert first["kernel"] == "binned"
    monkeypatch.setenv("MRS_DEPTH_V2", "1")
    second = sim.render_plan(m, 0, 2048, 65536)
    assert second["kernel"] == "frame" and second != first
    monkeypatch.delenv("MRS_DEPTH_V2")
    monkeypatch.setenv("MRS_RAST_BUDGET_MB", "1")
    assert sim.render_plan(m, 0, 2048, 65536)["chunk"] == 7
    monkeypatch.delenv("MRS_RAST_BUDGET_MB")
    assert sim.render_plan(m, 0, 2048, 65536) == first


def test_entry_point_is_declared_and_bound():
    import re
    header = re.sub(r"\s+", " ", (ROOT / "include" / "mrs.h").read_text())
    assert ("int mrs_debug_render_plan(const mrs_model* m, int cam, int n_frames, int max_lds, long long* out, "
            "int n);") in header
    L = sim.lib()
    assert hasattr(L, "mrs_debug_render_plan") and len(L.mrs_debug_render_plan.argtypes) == 6


def test_bad_arguments(models):
    m = models["mobile_base"]
    for cam, n, lds in ((-1, 1, 65536), (m.ncam, 1, 65536), (0, 0, 65536), (0, 1, -1)):
        with pytest.raises(sim.MrsError) as e:
            sim.render_plan(m, cam, n, lds)
        assert e.value.code == ERR_INVALID
    assert sim.lib().mrs_debug_render_plan(None, 0, 1, 65536, None, 7) == ERR_INVALID
