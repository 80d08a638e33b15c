"""Per-env model parameters on the GPU: actuator gainprm / biasprm, dof damping and geom sliding friction
in the batched step, against the fp64 oracle on per-env variants of each scene (model_param_scenes.py:
the variant is compiled with the env's attributes in the XML).

Bar: worst |gpu - ref| <= 1e-5 x max(1, largest |ref|) per quantity; the round-trip, fused-launch, reset
and unused-path checks are bit for bit.  5 envs, so the last wave is partial and env spread is active."""
import numpy as np
import pytest

import model_param_scenes as mp
from mujoco_ros2_simulation_amd import sim

pytestmark = pytest.mark.gpu
N = 5
P = mp.PARAMS


def _close(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    err, scale = float(np.max(np.abs(got - want))), max(1.0, float(np.max(np.abs(want))))
    print(f"{name:14s} max |err| {err:.2e}  scale {scale:.3g}  rel {err / scale:.2e}")
    assert err <= 1e-5 * scale, (name, err, scale)


def _clean_env(monkeypatch, group=None):
    for k in ("MRS_GROUP", "MRS_G16_WPB", "MRS_RAY_HELPERS", "MRS_SPREAD", "MRS_NO_FUSE_IH"):
        monkeypatch.delenv(k, raising=False)
    if group:
        monkeypatch.setenv("MRS_GROUP", str(group))


def _arm_batch(values, seed, **kw):
    """the arm compiled with the base values, the envs' parameters and a state written to the batch"""
    model = mp.model_of(mp.arm_scene, mp.ARM_BASE, **kw)
    qpos, qvel, ctrl = mp.arm_state(N, seed)
    b = sim.Batch(model, N)
    b.set(sim.FIELD_QPOS, qpos)
    b.set(sim.FIELD_QVEL, qvel)
    b.set(sim.FIELD_CTRL, ctrl)
    mp.set_all(b, mp.env_rows(mp.arm_scene, values, **kw))
    return model, b, qpos, qvel, ctrl


def _arm_forward_and_steps(values, seed, steps=10, **kw):
    """forward: qacc and qfrc_actuator; then `steps` single steps, each against the oracle variant's step
    from the batch's own state before it (warmstart included)"""
    model, b, qpos, qvel, ctrl = _arm_batch(values, seed, **kw)
    lay = b.layout()
    b.forward()
    ref = []
    for e in range(N):
        d = mp.oracle(mp.arm_scene, values[e], qpos[e], qvel[e], ctrl[e], **kw)
        d.forward()
        ref.append(d)
    _close("qacc", b.get(sim.FIELD_QACC), [d.qacc for d in ref])
    _close("qfrc_actuator", b.get(sim.FIELD_QFRC_ACTUATOR), [d.qfrc_actuator for d in ref])
    worst = {"qpos": 0.0, "qvel": 0.0}
    for step in range(steps):
        q, v, w = b.get(sim.FIELD_QPOS), b.get(sim.FIELD_QVEL), b.get(sim.FIELD_QACC_WARMSTART)
        b.step(1)
        ref = []
        for e in range(N):
            d = mp.oracle(mp.arm_scene, values[e], q[e], v[e], ctrl[e], w[e], **kw)
            d.step(1)
            ref.append(d)
        for name, got, want in (("qpos", b.get(sim.FIELD_QPOS), [d.qpos for d in ref]),
                                ("qvel", b.get(sim.FIELD_QVEL), [d.qvel for d in ref])):
            err, scale = np.max(np.abs(got - np.array(want))), max(1.0, np.max(np.abs(want)))
            worst[name] = max(worst[name], err / scale)
            assert err <= 1e-5 * scale, (step, name, err, scale)
    print("worst rel over the steps", worst)
    b.close()
    return lay


# ---- 1: round trip and defaults
def test_round_trip_and_defaults(monkeypatch):
    _clean_env(monkeypatch)
    model = mp.model_of(mp.arm_scene, mp.ARM_BASE)
    own = mp.model_rows(model)
    b = sim.Batch(model, N)
    lib, h = sim.lib(), b._h
    assert [lib.mrs_batch_param_dim(h, p) for p in P] == [3 * model.nu, 3 * model.nu, model.nv, model.ngeom]
    assert lib.mrs_batch_param_dim(h, 4) == -1 and lib.mrs_batch_param_dim(h, -1) == -1
    for p in P:  # before any set: the model's arrays for every env
        got = b.get_model_param(p)
        assert got.shape == (N,) + own[p].shape
        assert np.array_equal(got, np.tile(mp.f32(own[p]), (N,) + (1,) * own[p].ndim)), p
    rng = np.random.default_rng(1)
    for p in P:
        rows = rng.uniform(0.1, 3.0, (3,) + own[p].shape)  # (fp64 values that fp32 rounds)
        b.set_model_param(p, rows, env0=1)
        got = b.get_model_param(p)
        assert np.array_equal(got[1:4], mp.f32(rows)), p
        assert np.array_equal(got[[0, 4]], np.tile(mp.f32(own[p]), (2,) + (1,) * own[p].ndim)), p
        assert np.array_equal(b.get_model_param(p, env0=2, n=2), mp.f32(rows[1:3])), p
        # one row broadcasts over the envs from env0 on
        b.set_model_param(p, rows[0], env0=3)
        assert np.array_equal(b.get_model_param(p, env0=3), mp.f32(np.stack([rows[0], rows[0]]))), p
        assert b.model_param_device_ptr(p) != 0
    # rejected writes leave the values as they are
    before = [b.get_model_param(p) for p in P]
    bad = np.ones((1, model.nv))
    for p, val in ((sim.PARAM_DOF_DAMPING, -0.5), (sim.PARAM_DOF_DAMPING, np.nan), (sim.PARAM_DOF_DAMPING, np.inf)):
        row = bad.copy()
        row[0, 1] = val
        assert lib.mrs_batch_set_param(h, p, row.ctypes.data, 0, 1) == -1, (p, val)
    fr = np.ones((1, model.ngeom))
    fr[0, 0] = -1e-3
    assert lib.mrs_batch_set_param(h, sim.PARAM_GEOM_FRICTION, fr.ctypes.data, 0, 1) == -1
    gp = np.ones((1, model.nu, 3))
    gp[0, 0, 2] = np.nan
    assert lib.mrs_batch_set_param(h, sim.PARAM_ACT_GAINPRM, gp.ctypes.data, 0, 1) == -1
    gp[0, 0, 2] = -2.0  # (a negative gain or bias is a value like any other)
    assert lib.mrs_batch_set_param(h, sim.PARAM_ACT_BIASPRM, gp.ctypes.data, 4, 1) == 0
    before[1][4] = gp[0]
    rows = np.ones((N + 1, model.nv))
    for env0, n in ((-1, 1), (N, 1), (3, 3), (0, N + 1), (0, -1)):
        assert lib.mrs_batch_set_param(h, sim.PARAM_DOF_DAMPING, rows.ctypes.data, env0, n) == -1, (env0, n)
        assert lib.mrs_batch_get_param(h, sim.PARAM_DOF_DAMPING, rows.ctypes.data, env0, n) == -1, (env0, n)
    assert lib.mrs_batch_set_param(h, 4, rows.ctypes.data, 0, 1) == -1
    assert lib.mrs_batch_get_param(h, 4, rows.ctypes.data, 0, 1) == -1
    assert not lib.mrs_batch_param_device_ptr(h, 4)
    with pytest.raises(sim.MrsError):
        b.set_model_param(sim.PARAM_DOF_DAMPING, [[-1.0, 1.0]])
    for p, want in zip(P, before):
        assert np.array_equal(b.get_model_param(p), want), p
    b.close()


# ---- 2: gains and damping at every group width
@pytest.mark.parametrize("group", [16, 32, 64])
def test_gains_and_damping(group, monkeypatch):
    _clean_env(monkeypatch, group)
    values = mp.arm_values(N, 2)
    # (every env's values are far from the model's: an env that used the shared table would miss the bar)
    assert np.all(np.abs(values / np.array(mp.ARM_BASE) - 1) > 0.02) and np.ptp(values / np.array(mp.ARM_BASE)) > 1.0
    lay = _arm_forward_and_steps(values, 2)
    assert lay["group"] == group and lay["blocked"] == (1 if group == 64 else 0), lay


# ---- 3: every integrator, and the three routes of the integrator's factor
ROUTES = {
    "inline": dict(env={"MRS_NO_FUSE_IH": "1"}, lidar=False, flags={"fused_integrator_factor": 0, "helper_waves": 0}),
    "fused": dict(env={}, lidar=False, flags={"fused_integrator_factor": 1, "helper_waves": 0}),
    "helper": dict(env={"MRS_G16_WPB": "1", "MRS_RAY_HELPERS": "1"}, lidar=True,
                   flags={"fused_integrator_factor": 0, "helper_waves": 1}),
}
CASES = [("Euler", "inline"), ("implicitfast", "inline"), ("implicit", "inline"), ("RK4", "inline"),
         ("implicitfast", "fused"), ("Euler", "helper"), ("implicitfast", "helper")]


@pytest.mark.parametrize("integrator, route", CASES, ids=[f"{i}-{r}" for i, r in CASES])
def test_integrators(integrator, route, monkeypatch):
    _clean_env(monkeypatch, 16)
    r = ROUTES[route]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    # kv and damping drawn up to 30x the base values: the integrator's matrix M + h D is far from the
    # shared model's
    values = mp.arm_values(N, 3, lo=10.0, hi=30.0)
    if integrator == "RK4":  # no integrator matrix, and explicit: values it integrates stably (h kv / I < 1)
        values = mp.arm_values(N, 3, lo=0.3, hi=1.0)
    else:
        qpos, qvel, ctrl = mp.arm_state(N, 3)
        for e in range(N):
            restated, gap = mp.integrator_matrix_gap(values[e], mp.ARM_BASE, qpos[e], qvel[e], ctrl[e], integrator)
            scale = max(1.0, float(np.max(np.abs(qvel))))
            assert restated <= 1e-9 * scale, (e, restated)  # the restatement is the oracle's step
            assert gap > 100 * 1e-5 * scale, (e, gap)       # and the shared D in it misses the bar 100 times over
    lay = _arm_forward_and_steps(values, 3, steps=5, integrator=integrator, lidar=r["lidar"])
    assert lay["group"] == 16, lay
    for k, v in r["flags"].items():
        assert lay[k] == v, (k, lay)


# ---- 4: friction
def _box(values, seed, **kw):
    model = mp.model_of(mp.box_scene, mp.BOX_BASE, **kw)
    qpos, qvel = mp.box_state(N, seed)
    b = sim.Batch(model, N)
    b.set(sim.FIELD_QPOS, qpos)
    b.set(sim.FIELD_QVEL, qvel)
    mp.set_all(b, mp.env_rows(mp.box_scene, values, **kw))
    return model, b, qpos, qvel


BOX_CASES = [("PGS", "pyramidal", None, False), ("Newton", "pyramidal", None, False), ("PGS", "elliptic", None, False),
             ("Newton", "elliptic", None, False), ("PGS", "pyramidal", 64, False), ("PGS", "pyramidal", None, True),
             ("Newton", "elliptic", None, True), ("PGS", "pyramidal", "helper", False)]


@pytest.mark.parametrize("solver, cone, group, pair", BOX_CASES,
                         ids=[f"{s}-{c}-{ {None: 'auto', 64: 'g64'}.get(g, g)}{'-pair' if p else ''}" for s, c, g, p in BOX_CASES])
def test_friction(solver, cone, group, pair, monkeypatch):
    helper = group == "helper"  # the helper wave runs the collision pass and builds the rows
    _clean_env(monkeypatch, 16 if helper else group)
    if helper:
        monkeypatch.setenv("MRS_G16_WPB", "1")
        monkeypatch.setenv("MRS_RAY_HELPERS", "1")
    kw = dict(solver=solver, cone=cone, pair=pair, lidar=helper)
    values = mp.box_values(N, 4)
    assert values[0, 1] > values[0, 0] and values[1, 0] > values[1, 1]  # the max rule matters both ways
    model, b, qpos, qvel = _box(values, 4, **kw)
    if helper:
        assert b.layout()["group"] == 16 and b.layout()["helper_waves"] == 1, b.layout()
    elif group:
        assert b.layout()["group"] == 64 and b.layout()["blocked"] == 1, b.layout()
    floor, cube = model.name2id(sim.OBJ_GEOM, "floor"), model.name2id(sim.OBJ_GEOM, "cube")
    rows = b.get_model_param(sim.PARAM_GEOM_FRICTION)
    assert np.array_equal(rows[:, floor], values[:, 0]) and np.array_equal(rows[:, cube], values[:, 1])
    b.forward()
    fwd = []
    for e in range(N):
        d = mp.oracle(mp.box_scene, values[e], qpos[e], qvel[e], **kw)
        d.forward()
        fwd.append(d)
        g, want = b.contacts(e)[0], d.contacts()[0]
        assert len(want) == (8 if pair else 4) and np.array_equal(g, want), (e, g, want)
    _close("qacc", b.get(sim.FIELD_QACC), [d.qacc for d in fwd])
    b.set(sim.FIELD_QACC_WARMSTART, np.zeros((N, 6)))
    b.step(1)
    ref = []
    for e in range(N):
        d = mp.oracle(mp.box_scene, values[e], qpos[e], qvel[e], warm=np.zeros(6), **kw)
        d.step(1)
        ref.append(d)
    _close("qpos", b.get(sim.FIELD_QPOS), [d.qpos for d in ref])
    _close("qvel", b.get(sim.FIELD_QVEL), [d.qvel for d in ref])
    # friction matters here: the envs' tangential accelerations differ far beyond the bar
    assert np.ptp([d.qacc[1] for d in fwd]) > 1e-2
    b.close()


# ---- 5: fused launches and the device pointer
class _DeviceView:
    """a device buffer as torch.as_tensor takes it (the CUDA array interface)"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2}


def test_fused_launch_and_device_pointer(monkeypatch):
    import torch
    _clean_env(monkeypatch)
    values = mp.arm_values(N, 5)
    runs = []
    for fused in (True, False):
        model, b, qpos, qvel, ctrl = _arm_batch(values, 5, integrator="implicitfast")
        for _ in range(1 if fused else 10):
            b.step(10 if fused else 1)
        runs.append([b.get(sim.FIELD_QPOS), b.get(sim.FIELD_QVEL), b.get(sim.FIELD_QACC), b.get(sim.FIELD_QFRC_ACTUATOR)])
        if fused:
            b.close()
    for name, u, v in zip(("qpos", "qvel", "qacc", "qfrc_actuator"), *runs):
        assert np.array_equal(u, v), (name, np.abs(u - v).max())
    # other values through the device pointers between launches: the next launch reads them
    new = np.roll(values, 2, axis=0)
    rows = mp.env_rows(mp.arm_scene, new, integrator="implicitfast")
    b.sync()
    for p in (sim.PARAM_ACT_GAINPRM, sim.PARAM_ACT_BIASPRM, sim.PARAM_DOF_DAMPING):
        flat = rows[p].reshape(N, -1)
        view = torch.as_tensor(_DeviceView(b.model_param_device_ptr(p), flat.shape), device="cuda")
        view.copy_(torch.tensor(flat, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert np.array_equal(b.get_model_param(sim.PARAM_DOF_DAMPING), rows[sim.PARAM_DOF_DAMPING])
    q, v, w = b.get(sim.FIELD_QPOS), b.get(sim.FIELD_QVEL), b.get(sim.FIELD_QACC_WARMSTART)
    b.step(1)
    ref = []
    for e in range(N):
        d = mp.oracle(mp.arm_scene, new[e], q[e], v[e], ctrl[e], w[e], integrator="implicitfast")
        d.step(1)
        ref.append(d)
    _close("qpos", b.get(sim.FIELD_QPOS), [d.qpos for d in ref])
    _close("qvel", b.get(sim.FIELD_QVEL), [d.qvel for d in ref])
    _close("qfrc_actuator", b.get(sim.FIELD_QFRC_ACTUATOR), [d.qfrc_actuator for d in ref])
    b.close()


# ---- 6: resets keep them
def test_resets_keep_the_parameters(monkeypatch):
    _clean_env(monkeypatch)
    values = mp.arm_values(N, 6)
    model, b, qpos, qvel, ctrl = _arm_batch(values, 6)
    want = [b.get_model_param(p) for p in P]

    def unchanged(tag):
        for p, w in zip(P, want):
            assert np.array_equal(b.get_model_param(p), w), (tag, p)

    def next_step_matches(tag):
        b.set(sim.FIELD_QPOS, qpos)
        b.set(sim.FIELD_QVEL, qvel)
        b.set(sim.FIELD_CTRL, ctrl)
        b.set(sim.FIELD_QACC_WARMSTART, np.zeros((N, model.nv)))
        b.step(1)
        ref = []
        for e in range(N):
            d = mp.oracle(mp.arm_scene, values[e], qpos[e], qvel[e], ctrl[e], np.zeros(model.nv))
            d.step(1)
            ref.append(d)
        _close(tag + " qpos", b.get(sim.FIELD_QPOS), [d.qpos for d in ref])
        _close(tag + " qvel", b.get(sim.FIELD_QVEL), [d.qvel for d in ref])

    b.step(3)
    b.reset()
    unchanged("reset")
    next_step_matches("reset")
    b.reset_where(np.array([1, 0, 1, 0, 1], dtype=bool))
    unchanged("reset_where")
    next_step_matches("masked")
    # a NaN in qpos written by the host: the env auto-resets, its parameters stay
    q = b.get(sim.FIELD_QPOS)
    q[3, 0] = np.nan
    b.set(sim.FIELD_QPOS, q)
    b.step(1)
    assert b.get(sim.FIELD_WARNING)[3, 0] == 1 and np.all(np.isfinite(b.get(sim.FIELD_QPOS)))
    unchanged("auto-reset")
    next_step_matches("auto-reset")
    b.close()


# ---- 7: unused means unchanged
@pytest.mark.parametrize("integrator", ["Euler", "implicitfast"])
def test_unused_means_unchanged(integrator, monkeypatch):
    _clean_env(monkeypatch)
    model = mp.model_of(mp.arm_scene, mp.ARM_BASE, integrator=integrator)
    qpos, qvel, ctrl = mp.arm_state(N, 7)
    out, lays = [], []
    for use in (False, True):
        b = sim.Batch(model, N)
        b.set(sim.FIELD_QPOS, qpos)
        b.set(sim.FIELD_QVEL, qvel)
        b.set(sim.FIELD_CTRL, ctrl)
        if use:  # every parameter set to the model's own values
            mp.set_all(b, {p: np.tile(r, (N,) + (1,) * r.ndim) for p, r in mp.model_rows(model).items()})
        lays.append(b.layout())
        b.step(10)
        out.append([b.get(sim.FIELD_QPOS), b.get(sim.FIELD_QVEL), b.get(sim.FIELD_QACC), b.get(sim.FIELD_QFRC_ACTUATOR)])
        b.close()
    for name, u, v in zip(("qpos", "qvel", "qacc", "qfrc_actuator"), *out):
        assert np.array_equal(u, v), (name, np.abs(u - v).max())
    # the layout of a batch that sets nothing is what it was before the feature: per env the arm's LDS
    # working set and scratch region (floats), recorded on the commit before this one
    assert lays[0] == lays[1]
    assert (lays[0]["group"], lays[0]["lds_floats"], lays[0]["scratch_floats"]) == PARENT_LAYOUT[integrator], lays[0]


# (group, LDS floats per env, scratch floats per env) of the arm scene on the parent commit
PARENT_LAYOUT = {"Euler": (16, 308, 72), "implicitfast": (16, 312, 72)}
