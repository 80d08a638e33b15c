"""The ray-query entry points exist with the documented signatures, sim.py's constants match the header, a
NULL handle is rejected with a message, and the geom list of a filter (mrs_debug_ray_filter: what the
batch uploads for the query kernel) equals a brute-force filter over the model view (CPU: no device is
touched)."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT
from mujoco_ros2_simulation_amd import sim

MRS_ERR_INVALID = -1
HEADER = (ROOT / "include" / "mrs.h").read_text()

# groups 0-5 and two outside them, alpha-0 geoms, world and mocap geoms (both body_weldid == 0), a body
# welded to the world (no joint) and moving bodies
FILTER_SCENE = """<mujoco><worldbody>
  <geom name="floor" type="plane" size="0 0 1" group="0"/>
  <geom name="w1" type="box" size="0.1 0.1 0.1" pos="1 0 0.1" group="1"/>
  <geom name="w2" type="sphere" size="0.1" pos="2 0 0.1" group="2" rgba="1 0 0 0"/>
  <geom name="w6" type="sphere" size="0.1" pos="3 0 0.1" group="6"/>
  <body name="mocap" mocap="true" pos="0 1 0.5">
    <geom name="m3" type="box" size="0.1 0.1 0.1" group="3"/>
    <geom name="m4" type="capsule" size="0.05 0.1" group="4" rgba="0 1 0 0"/>
  </body>
  <body name="welded" pos="0 2 0.5"><geom name="f5" type="cylinder" size="0.1 0.1" group="5"/>
    <body name="child" pos="0 0 0.3"><joint type="hinge" axis="0 1 0"/>
      <geom name="c0" type="capsule" size="0.04 0.1" group="0"/>
      <geom name="c7" type="sphere" size="0.05" pos="0 0 0.2" group="7"/></body></body>
  <body name="free" pos="0 -1 0.5"><freejoint/>
    <geom name="b1" type="ellipsoid" size="0.1 0.05 0.07" group="1"/>
    <geom name="b2" type="box" size="0.05 0.05 0.05" pos="0.2 0 0" group="2"/>
    <geom name="b3" type="sphere" size="0.05" pos="-0.2 0 0" group="3" rgba="0 0 1 0"/>
    <geom name="b4" type="sphere" size="0.05" pos="0 0.2 0" group="4"/>
    <geom name="b5" type="sphere" size="0.05" pos="0 -0.2 0" group="5"/></body>
</worldbody></mujoco>"""


def test_header_declarations():
    squeezed = re.sub(r"\s+", " ", HEADER)
    for decl in ("int mrs_batch_ray_device(mrs_batch* b, const float* d_pnt, const float* d_vec, int n_rays, int flags, "
                 "int frame_type, int frame_id, unsigned group_mask, int bodyexclude, float* d_dist, int* d_geomid);",
                 "int mrs_batch_ray(mrs_batch* b, const double* pnt, const double* vec, int n_rays, int flags, "
                 "int frame_type, int frame_id, unsigned group_mask, int bodyexclude, double* dist, int* geomid, "
                 "int env0, int n);",
                 "int mrs_debug_ray_filter(const mrs_model* m, unsigned group_mask, int flags, int bodyexclude, "
                 "int* out, int max);"):
        assert decl in squeezed, decl


def test_constants_match_header():
    enum = {k: int(v) for k, v in re.findall(r"MRS_RAY_(\w+) = (\d+)", HEADER)}
    assert enum == {"SHARED": sim.RAY_SHARED, "NO_STATIC": sim.RAY_NO_STATIC, "FRAME_WORLD": sim.RAY_FRAME_WORLD,
                    "FRAME_GEOM": sim.RAY_FRAME_GEOM, "FRAME_CAMERA": sim.RAY_FRAME_CAMERA}
    assert (sim.RAY_SHARED, sim.RAY_NO_STATIC) == (1, 2)
    assert (sim.RAY_FRAME_WORLD, sim.RAY_FRAME_GEOM, sim.RAY_FRAME_CAMERA) == (0, 1, 2)


def test_entry_points_and_null_handle():
    L = sim.lib()
    for name in ("mrs_batch_ray_device", "mrs_batch_ray", "mrs_debug_ray_filter"):
        assert hasattr(L, name), name
    assert len(L.mrs_batch_ray_device.argtypes) == 11
    assert len(L.mrs_batch_ray.argtypes) == 13
    assert len(L.mrs_debug_ray_filter.argtypes) == 6
    buf = (C.c_double * 3)()
    out = (C.c_double * 1)()
    ids = (C.c_int * 4)()
    assert L.mrs_batch_ray(None, buf, buf, 1, 0, 0, 0, 0, -1, out, ids, 0, 1) == MRS_ERR_INVALID
    assert L.mrs_last_error().decode() == "null batch"
    assert L.mrs_last_status() == MRS_ERR_INVALID
    assert L.mrs_batch_ray_device(None, None, None, 1, 0, 0, 0, 0, -1, None, None) == MRS_ERR_INVALID
    assert L.mrs_last_error().decode() == "null batch"
    assert L.mrs_debug_ray_filter(None, 0, 0, -1, ids, 4) == MRS_ERR_INVALID
    assert L.mrs_last_error().decode() == "null model"


def test_batch_methods():
    for name in ("ray", "ray_device"):
        assert callable(getattr(sim.Batch, name)), name


def _brute(m, mask, no_static, bodyexclude):
    keep = []
    for g in range(m.ngeom):
        body = m.geom_bodyid[g]
        if body == bodyexclude or m.geom_rgba[g, 3] == 0:
            continue
        if mask and not (0 <= m.geom_group[g] < 6 and (mask >> m.geom_group[g]) & 1):
            continue
        if no_static and m.body_weldid[body] == 0:
            continue
        keep.append(g)
    return keep


@pytest.fixture(scope="module")
def filter_model(built):
    return sim.Model.from_string(FILTER_SCENE)


def test_filter_scene_covers_the_cases(filter_model):
    m = filter_model
    assert set(m.geom_group.tolist()) == set(range(8))
    assert np.sum(m.geom_rgba[:, 3] == 0) == 3
    mocap = m.name2id(sim.OBJ_BODY, "mocap")
    assert m.body_weldid[0] == 0 and m.body_weldid[mocap] == 0 and m.body_mocapid[mocap] == 0
    assert m.body_weldid[m.name2id(sim.OBJ_BODY, "welded")] == 0  # (no joint: welded to the world)
    assert m.body_weldid[m.name2id(sim.OBJ_BODY, "child")] != 0 and m.body_weldid[m.name2id(sim.OBJ_BODY, "free")] != 0


@pytest.mark.parametrize("no_static", [False, True])
def test_filter_matches_brute_force(filter_model, no_static):
    m = filter_model
    masks = [0] + [1 << g for g in range(6)] + [0b000110, 0b111111, 1 << 6, (1 << 7) | 1]
    seen = set()
    for mask in masks:
        for body in range(-1, m.nbody):
            got = sim.ray_filter(m, mask, not no_static, body).tolist()
            assert got == _brute(m, mask, no_static, body), (mask, no_static, body)
            seen.add(tuple(got))
    assert len(seen) > 10  # (the triples do select different lists)
    everything = sim.ray_filter(m, 0, True, -1).tolist()
    assert everything == [g for g in range(m.ngeom) if m.geom_rgba[g, 3] != 0]


def test_filter_count_beyond_capacity_and_bad_arguments(filter_model):
    L, m = sim.lib(), filter_model
    full = sim.ray_filter(m)
    ids = (C.c_int * 2)(-7, -7)
    assert L.mrs_debug_ray_filter(m.handle, 0, 0, -1, ids, 1) == len(full)  # the count, one id written
    assert list(ids) == [int(full[0]), -7]
    assert L.mrs_debug_ray_filter(m.handle, 0, 0, -1, None, 0) == len(full)
    assert L.mrs_debug_ray_filter(m.handle, 0, sim.RAY_SHARED | sim.RAY_NO_STATIC, -1, None, 0) == \
        len(sim.ray_filter(m, include_static=False))
    for flags, body, msg in ((4, -1, "unknown ray flag"), (0, -2, "bodyexclude out of range"),
                             (0, m.nbody, "bodyexclude out of range")):
        assert L.mrs_debug_ray_filter(m.handle, 0, flags, body, ids, 2) == MRS_ERR_INVALID
        assert L.mrs_last_error().decode() == msg
    assert L.mrs_debug_ray_filter(m.handle, 0, 0, -1, None, 2) == MRS_ERR_INVALID
    assert L.mrs_debug_ray_filter(m.handle, 0, 0, -1, ids, -1) == MRS_ERR_INVALID
