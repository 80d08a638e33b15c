"""The scenes, poses and rays of tests/test_gpu_ray_query.py are fit for the rule of tests/ray_ref.py (CPU:
the fp64 oracle only).  The oracle at the tests' fp32-rounded inputs is compared, under ray_ref.check,
with the oracle at the same inputs perturbed by up to one fp32 rounding (every qpos and ray component
times 1 +- 6e-8): a scene or seed that puts many rays on a silhouette would leave the caps here, before any
device result is looked at.  It also guards what the GPU cases count on: which geoms the rays reach."""
import numpy as np
import pytest

import ray_ref
import test_gpu_ray_query as cases
from mujoco_ros2_simulation_amd import sim


def _jig(rng, a):
    return a * (1 + rng.uniform(-6e-8, 6e-8, size=np.shape(a)))


def _self_check(name, model, q, pnt, vec, bodyexclude=-1):
    """(dist, geomid) of the oracle at the perturbed inputs, checked against the oracle at the given ones"""
    rng = np.random.default_rng(1)
    ods = cases._oracles(model, q)
    moved = cases._oracles(model, _jig(rng, q))
    got = [ray_ref.oracle_rays(moved[e], _jig(rng, pnt[e]), _jig(rng, vec[e]), bodyexclude) for e in range(len(q))]
    d, g = np.stack([x[0] for x in got]), np.stack([x[1] for x in got])
    outliers = ray_ref.check(name, ods, pnt, vec, d, g, bodyexclude=bodyexclude)
    assert outliers == 0, f"{name}: {outliers} rays graze at the fp32 level: choose another seed"
    return d, g


def _framed(ods, poses, pnt, vec):
    world = [ray_ref.to_world(*poses(od), pnt, vec) for od in ods]
    return np.stack([w[0] for w in world]), np.stack([w[1] for w in world])


def test_primitive_rays():
    model, q, pnt, vec = cases._prim_case()
    d, g = _self_check("primitives", model, q, pnt, vec)
    assert set(g[g >= 0].tolist()) == set(range(model.ngeom))
    for n_rays in (63, 64, 65, cases.TILE):  # every prefix the GPU case casts reaches every geom, too
        assert set(g[:, :n_rays][g[:, :n_rays] >= 0].tolist()) == set(range(model.ngeom)), n_rays


def test_shared_grid_rays():
    model, q, g7, pnt, vec = cases._arm_case()
    wp, wv = _framed(cases._oracles(model, q), lambda od: (od.kinematics()[2][g7], od.kinematics()[3][g7]), pnt, vec)
    d, g = _self_check("arm7 geom frame", model, q, wp, wv)
    assert np.mean(d >= 0) > 0.3 and len(set(g[g >= 0].tolist())) >= 3
    model, q, cam, pnt, vec = cases._mobile_case()
    wp, wv = _framed(cases._oracles(model, q), lambda od: cases._cam_world(model, od, cam), pnt, vec)
    d, g = _self_check("mobile base camera frame", model, q, wp, wv)
    assert np.mean(d >= 0) > 0.3 and len(set(g[g >= 0].tolist())) >= 3


@pytest.mark.parametrize("kwargs", [dict(group_mask=1 << 1), dict(group_mask=(1 << 0) | (1 << 2)),
                                    dict(include_static=False), dict()])
def test_filter_rays(kwargs):
    model, q, pnt, vec = cases._filter_case()
    reduced = sim.Model.from_string(cases._filter_xml(cases._removed_by(model, **kwargs)))
    d, _ = _self_check(f"filter {kwargs}", reduced, q, pnt, vec)
    assert np.sum(d >= 0) >= 20


def test_bodyexclude_rays():
    model, q, pnt, vec = cases._filter_case()
    for body in ("mover", "arm"):
        _self_check(f"bodyexclude {body}", model, q, pnt, vec, bodyexclude=model.name2id(sim.OBJ_BODY, body))


def test_chunk_and_mesh_rays():
    model, q, pnt, vec, n_sph = cases._chunk_case()
    d, g = _self_check("chunking", model, q, pnt, vec)
    assert np.all(g[:, 0] == n_sph - 1) and np.all(g[:, 1] == n_sph) and np.mean(g >= 0) > 0.8
    model, q, pnt, vec = cases._mesh_case()
    d, g = _self_check("mesh robot", model, q, pnt, vec)
    shells = np.isin(g, [model.name2id(sim.OBJ_GEOM, f"g{k}_shell") for k in range(1, 8)])
    assert shells.sum() > 40 and np.sum(g == model.name2id(sim.OBJ_GEOM, "statue")) > 40
