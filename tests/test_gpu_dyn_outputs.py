"""The dynamics outputs (MRS_DYNOUT_*: qfrc_bias, the dense mass matrix, site Jacobians and poses) of the
batched step against the fp64 references of tests/dyn_ref.py.

The bar is the project's own: the absolute error of each output is at most
1e-5 * max(1, largest |ref| of that output in that env); no env and no element is excluded.  States are
random (re-seeded per test): qpos within the joint ranges, qvel in +-2, so the Coriolis terms count."""
import numpy as np
import pytest

import binding
import dyn_ref
import inertial_scenes as ins
from conftest import ARM7, REF_SCENE
from mujoco_ros2_simulation_amd import sim
from sensor_scenes import FLOAT, bare

pytestmark = pytest.mark.gpu
ARM_BOXES = ARM7.parent / "arm_boxes.xml"
MOBILE = ARM7.parent / "mobile_base.xml"
ALL = (sim.DYNOUT_QFRC_BIAS, sim.DYNOUT_MASS_MATRIX, sim.DYNOUT_SITE_JAC, sim.DYNOUT_SITE_POSE)
NAMES = ("qfrc_bias", "mass_matrix", "site_jac", "site_pose")
BAR = 1e-5


def _env(monkeypatch, group=None, helpers=False, every=False):
    for k in ("MRS_GROUP", "MRS_G16_WPB", "MRS_RAY_HELPERS", "MRS_SPREAD", "MRS_SENSORS_EVERY_STEP"):
        monkeypatch.delenv(k, raising=False)
    if group:
        monkeypatch.setenv("MRS_GROUP", str(group))
    if helpers:
        monkeypatch.setenv("MRS_G16_WPB", "1")
        monkeypatch.setenv("MRS_RAY_HELPERS", "1")
    if every:
        monkeypatch.setenv("MRS_SENSORS_EVERY_STEP", "1")


def _states(model, n, seed):
    """qpos within the joint ranges (+-1.5 where a hinge / slide has none; random unit quaternions for ball /
    free, a free body moved up to 0.2 sideways and 0.3 up), qvel in +-2, rounded to fp32"""
    rng = np.random.default_rng(seed)
    qpos = np.tile(np.array(model.qpos0, dtype=np.float64), (n, 1))
    for j in range(model.njnt):
        a, t = model.jnt_qposadr[j], model.jnt_type[j]
        if t in (sim.JNT_HINGE, sim.JNT_SLIDE):
            lo, hi = model.jnt_range[j] if model.jnt_limited[j] else (-1.5, 1.5)
            qpos[:, a] = rng.uniform(lo, hi, n)
            continue
        if t == sim.JNT_FREE:
            qpos[:, a:a + 3] += rng.uniform(-0.2, 0.2, (n, 3)) * [1, 1, 0] + [0, 0, 0.3]
            a += 3
        q = rng.normal(size=(n, 4))
        qpos[:, a:a + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
    qvel = rng.uniform(-2, 2, (n, model.nv))
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    return f32(qpos), f32(qvel)


def _sites(model, names):
    return [model.name2id(sim.OBJ_SITE, s) for s in names]


def _on(b, sites):
    b.set_jac_sites(sites)
    for w in ALL:
        b.dyn(w, n=0)


def _compare(b, model, xml, qpos, qvel, sites, tag, basedir=None, models=None, xmls=None):
    """every output of every env against the references at (qpos[e], qvel[e]); returns the worst relative
    error per output.  models / xmls: per-env variants (per-env inertial values)"""
    got = [b.dyn(w) for w in ALL]
    worst = [0.0] * 4
    for e in range(b.n):
        ref = dyn_ref.refs(models[e] if models else model, xmls[e] if xmls else xml, qpos[e], qvel[e], sites, basedir)
        for w in ALL:
            scale = max(1.0, float(np.max(np.abs(ref[w]))) if ref[w].size else 0.0)
            err = float(np.max(np.abs(got[w][e] - ref[w]))) / scale if ref[w].size else 0.0
            worst[w] = max(worst[w], err)
    print(f"{tag}: worst rel " + ", ".join(f"{NAMES[w]} {worst[w]:.2e}" for w in ALL))
    for w in ALL:
        assert worst[w] <= BAR, (tag, NAMES[w], worst[w])
    return worst


def _batch(model, n, qpos, qvel, sites):
    b = sim.Batch(model, n)
    b.set(sim.FIELD_QPOS, qpos)
    b.set(sim.FIELD_QVEL, qvel)
    _on(b, sites)
    return b


def test_known_answer_two_link(monkeypatch):
    """1: the reference 2-DoF arm (both hinges about z, link 1 of length 1, the ee_link site 1 along link 2):
    the planar Jacobian and the mass matrix tests/test_oracle_kat.py pins, in closed form"""
    _env(monkeypatch)
    model = sim.Model.load(REF_SCENE)
    n = 5
    qpos, qvel = _states(model, n, 1)
    sites = _sites(model, ["ee_link"])
    b = _batch(model, n, qpos, qvel, sites)
    b.forward()
    M, J, P = b.dyn(sim.DYNOUT_MASS_MATRIX), b.dyn(sim.DYNOUT_SITE_JAC), b.dyn(sim.DYNOUT_SITE_POSE)
    b.close()
    for e in range(n):
        q1, q2 = qpos[e]
        c = np.cos(q2)
        Mw = np.array([[0.45 + 27 * (1.25 + c) + 6.75, 0.225 + 27 * (0.25 + 0.5 * c)],
                       [0.225 + 27 * (0.25 + 0.5 * c), 6.975]])
        s1, c1, s12, c12 = np.sin(q1), np.cos(q1), np.sin(q1 + q2), np.cos(q1 + q2)
        Jw = np.zeros((6, 2))
        Jw[0], Jw[1], Jw[5] = [-s1 - s12, -s12], [c1 + c12, c12], [1, 1]
        assert np.max(np.abs(M[e] - Mw)) <= BAR * np.max(np.abs(Mw))
        assert np.max(np.abs(J[e, 0] - Jw)) <= BAR * max(1.0, np.max(np.abs(Jw)))
        assert np.max(np.abs(P[e, 0, :3] - [c1 + c12, s1 + s12, 0])) <= BAR * 2


def test_arm7_g16_forward_and_step(monkeypatch):
    """2: the 7-DoF arm at 16 lanes per env, 21 envs (a full workgroup, a partial wave and idle groups), a site
    on the last link: after forward() and after step(1) the outputs are those of the given state"""
    _env(monkeypatch)
    xml, base = ARM7.read_text(), str(ARM7.parent)
    model = sim.Model.load(ARM7)
    n = 21
    qpos, qvel = _states(model, n, 2)
    sites = _sites(model, ["ee"])
    b = _batch(model, n, qpos, qvel, sites)
    assert b.layout()["group"] == 16
    b.forward()
    _compare(b, model, xml, qpos, qvel, sites, "arm7 forward", base)
    b.step(1)
    _compare(b, model, xml, qpos, qvel, sites, "arm7 step(1)", base)
    b.close()


def test_quaternion_dofs_two_trees(monkeypatch):
    """3: a ball pendulum and a free box, one site on each: ball and free dofs, and the other tree's columns
    are exactly zero"""
    _env(monkeypatch)
    model = sim.Model.from_string(dyn_ref.BALL_FREE)
    n = 6
    qpos, qvel = _states(model, n, 3)
    sites = _sites(model, ["tip", "corner"])
    b = _batch(model, n, qpos, qvel, sites)
    b.forward()
    _compare(b, model, dyn_ref.BALL_FREE, qpos, qvel, sites, "ball + free")
    J, M = b.dyn(sim.DYNOUT_SITE_JAC), b.dyn(sim.DYNOUT_MASS_MATRIX)
    b.close()
    assert np.all(J[:, 0, :, 3:] == 0.0) and np.all(J[:, 1, :, :3] == 0.0)
    assert np.all(M[:, :3, 3:] == 0.0) and np.all(M[:, 3:, :3] == 0.0)


def test_blocked_mode_g64(monkeypatch):
    """4: arm_boxes (nv = 55, one env per wave, M per tree block): the dense matrix with exact zeros between
    the trees, the Jacobian of a site on the arm and of one on a box"""
    _env(monkeypatch)
    xml, base = ARM_BOXES.read_text(), str(ARM_BOXES.parent)
    # (two sites of its own: one on the arm's last link, one on the first box)
    for nm, site in (("link7", '<site name="dyn_a" pos="0.01 0.02 0.1" quat="0.8 0.2 -0.4 0.4"/>'),
                     ("box2", '<site name="dyn_b" pos="0.03 -0.02 0.04" quat="0.6 -0.3 0.5 0.2"/>')):
        i = xml.index(">", xml.index(f'<body name="{nm}"')) + 1
        xml = xml[:i] + site + xml[i:]
    model = sim.Model.from_string(xml, base)
    n = 3
    qpos, qvel = _states(model, n, 4)
    sites = _sites(model, ["dyn_a", "dyn_b"])
    b = _batch(model, n, qpos, qvel, sites)
    lay = b.layout()
    assert lay["group"] == 64 and lay["blocked"] == 1
    b.forward()
    _compare(b, model, xml, qpos, qvel, sites, "arm_boxes blocked", base)
    M = b.dyn(sim.DYNOUT_MASS_MATRIX)
    b.close()
    tree = np.zeros(model.nv, dtype=int)
    for j in range(model.njnt):
        d0 = model.jnt_dofadr[j]
        nd = {sim.JNT_FREE: 6, sim.JNT_BALL: 3}.get(int(model.jnt_type[j]), 1)
        tree[d0:d0 + nd] = model.body_rootid[model.jnt_bodyid[j]]
    off = tree[:, None] != tree[None, :]
    assert off.any() and np.all(M[:, off] == 0.0)


@pytest.mark.parametrize("solver", ["PGS", "Newton"])
def test_helper_waves(solver, monkeypatch):
    """5: the mobile base with its lidar under helper waves: the physics wave writes, the helper is untouched"""
    _env(monkeypatch, 16, helpers=True)
    xml, base = MOBILE.read_text().replace('solver="PGS"', f'solver="{solver}"'), str(MOBILE.parent)
    model = sim.Model.from_string(xml, base)
    n = 8
    qpos, qvel = _states(model, n, 5)
    sites = _sites(model, ["imu"])
    b = _batch(model, n, qpos, qvel, sites)
    assert b.layout()["helper_waves"] == 1
    b.forward()
    _compare(b, model, xml, qpos, qvel, sites, f"helpers {solver} forward", base)
    b.step(1)
    _compare(b, model, xml, qpos, qvel, sites, f"helpers {solver} step(1)", base)
    b.close()


@pytest.mark.parametrize("group", [32, 8])
def test_group_override(group, monkeypatch):
    """6: the arm at 32 and at 8 lanes per env"""
    _env(monkeypatch, group)
    xml, base = ARM7.read_text(), str(ARM7.parent)
    model = sim.Model.load(ARM7)
    n = 5
    qpos, qvel = _states(model, n, 6)
    sites = _sites(model, ["ee"])
    b = _batch(model, n, qpos, qvel, sites)
    assert b.layout()["group"] == group
    b.step(1)
    _compare(b, model, xml, qpos, qvel, sites, f"arm7 G={group}", base)
    b.close()


@pytest.mark.parametrize("integrator", ["Euler", "implicitfast", "implicit", "RK4"])
def test_integrators_state_convention(integrator, monkeypatch):
    """7: the landing box with its flap: after step(3) the outputs are those of the state before the third
    step's integration -- the pass that wrote sensordata (under RK4 the step's first stage)
    -- which a second batch stepped twice provides"""
    _env(monkeypatch)
    xml = bare(FLOAT).replace('integrator="implicitfast"', f'integrator="{integrator}"')
    model = sim.Model.from_string(xml)
    n = 4
    qpos, qvel = _states(model, n, 7)
    sites = _sites(model, ["corner", "tip"])
    b = _batch(model, n, qpos, qvel, sites)
    b.step(3)
    b2 = sim.Batch(model, n)
    b2.set(sim.FIELD_QPOS, qpos)
    b2.set(sim.FIELD_QVEL, qvel)
    b2.step(2)
    q2, v2 = b2.get(sim.FIELD_QPOS), b2.get(sim.FIELD_QVEL)
    b2.close()
    _compare(b, model, xml, q2, v2, sites, f"landing box {integrator}")
    b.close()


STATE = ((sim.FIELD_QPOS, "qpos"), (sim.FIELD_QVEL, "qvel"), (sim.FIELD_QACC, "qacc"),
         (sim.FIELD_QACC_WARMSTART, "qacc_warmstart"), (sim.FIELD_QFRC_ACTUATOR, "qfrc_actuator"),
         (sim.FIELD_SENSORDATA, "sensordata"), (sim.FIELD_TIME, "time"), (sim.FIELD_NCON, "ncon"),
         (sim.FIELD_SOLVER_NITER, "niter"), (sim.FIELD_WARNING, "warning"))


def test_cadence_and_non_interference(monkeypatch):
    """8: the arm at 21 envs: step(10), ten step(1) and MRS_SENSORS_EVERY_STEP=1 leave the same bits in the
    outputs; a batch with all four on and one that never asked have the same state bits"""
    model = sim.Model.load(ARM7)
    n = 21
    qpos, qvel = _states(model, n, 8)
    sites = _sites(model, ["ee"])
    runs = []
    for launches, every, on in ((1, False, True), (10, False, True), (1, True, True), (1, False, False)):
        _env(monkeypatch, every=every)
        b = sim.Batch(model, n)
        b.set(sim.FIELD_QPOS, qpos)
        b.set(sim.FIELD_QVEL, qvel)
        if on:
            _on(b, sites)
        assert b.layout()["sensors_every_step"] == int(every)
        for _ in range(launches):
            b.step(10 // launches)
        runs.append(([b.dyn(w) for w in ALL] if on else None, [b.get(f) for f, _ in STATE], b.layout()["dyn_outputs"]))
        b.close()
    assert [r[2] for r in runs] == [15, 15, 15, 0]
    for k in (1, 2):
        for w in ALL:
            assert np.array_equal(runs[0][0][w], runs[k][0][w]), (k, NAMES[w])
    for (_, name), u, v in zip(STATE, runs[0][1], runs[3][1]):
        assert np.array_equal(u, v), name


def test_per_env_inertial_values(monkeypatch):
    """9: masses, inertias and armatures off by up to +-20 % on half the envs (set_inertial): M and qfrc_bias
    of each env are those of the model compiled with that env's values, the others the base model's"""
    _env(monkeypatch)
    scene = ins.arm_scene
    n = 8
    rng = np.random.default_rng(9)
    fac = np.ones((n, scene.nfactor))
    fac[::2] = rng.uniform(0.8, 1.2, (n // 2, scene.nfactor))
    base = ins.base_of(scene)
    qpos, qvel = _states(base, n, 9)
    mass, inertia, arm = ins.env_rows(scene, fac)
    b = _batch(base, n, qpos, qvel, [])
    b.set_inertial(mass, inertia, arm)
    b.forward()
    xmls = [scene(tuple(float(x) for x in f)) for f in fac]
    _compare(b, base, None, qpos, qvel, [], "per-env inertial", models=[ins.model_of(scene, f) for f in fac], xmls=xmls)
    M = b.dyn(sim.DYNOUT_MASS_MATRIX)
    b.close()
    assert np.max(np.abs(M[0] - M[1])) > 1e-3 * np.max(np.abs(M[1]))  # (the envs do differ)


class _DeviceView:
    """a device buffer as torch.as_tensor takes it (the CUDA array interface)"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2}


def test_interface(monkeypatch):
    """10: switching on, the site selection, resets, the NaN auto-reset and the device pointer"""
    import torch
    _env(monkeypatch)
    xml, base = ARM7.read_text(), str(ARM7.parent)
    model = sim.Model.load(ARM7)
    n, nv = 5, model.nv
    qpos, qvel = _states(model, n, 10)
    b = sim.Batch(model, n)
    b.set(sim.FIELD_QPOS, qpos)
    b.set(sim.FIELD_QVEL, qvel)
    assert b.layout()["dyn_outputs"] == 0
    # no selection: dimension 0, no pointer, nothing copied
    assert b.dyn_dim(sim.DYNOUT_SITE_JAC) == 0 and b.dyn_dim(sim.DYNOUT_SITE_POSE) == 0
    assert b.dyn_device_ptr(sim.DYNOUT_SITE_JAC) is None and b.dyn(sim.DYNOUT_SITE_JAC).shape == (n, 0, 6, nv)
    assert b.layout()["dyn_outputs"] == 0
    # one output on: its bit only; zeros before any launch
    assert not b.dyn(sim.DYNOUT_QFRC_BIAS).any()
    assert b.layout()["dyn_outputs"] == 1 << sim.DYNOUT_QFRC_BIAS
    ee, rf = _sites(model, ["ee"])[0], 0
    b.set_jac_sites(["ee"])
    assert b.dyn_dim(sim.DYNOUT_SITE_JAC) == 6 * nv and b.dyn_dim(sim.DYNOUT_SITE_POSE) == 12
    assert b.layout()["dyn_outputs"] == (1 << sim.DYNOUT_QFRC_BIAS) | (1 << sim.DYNOUT_SITE_JAC)  # (asked for above)
    for bad in ([ee, ee], [model.nsite], [-1], list(range(17))):
        with pytest.raises(sim.MrsError) as err:
            b.set_jac_sites(bad)
        assert err.value.code == -1
    for w in ALL:
        b.dyn(w, n=0)
    assert b.layout()["dyn_outputs"] == 15
    b.forward()
    _compare(b, model, xml, qpos, qvel, [ee], "interface, one site", base)  # (the selection survived the rejected calls)
    # a new selection resizes the buffers, zero-filled
    b.set_jac_sites([rf, ee])
    assert b.dyn_dim(sim.DYNOUT_SITE_JAC) == 12 * nv and not b.dyn(sim.DYNOUT_SITE_JAC).any()
    b.forward()
    _compare(b, model, xml, qpos, qvel, [rf, ee], "interface, two sites", base)
    # the device pointer, read on the batch stream: the batch is put on a torch stream, a forward pass at a
    # new state is queued and not waited for, and copies queued behind it on that stream see its values
    q2, v2 = _states(model, n, 11)
    b.set(sim.FIELD_QPOS, q2)
    b.set(sim.FIELD_QVEL, v2)
    b.sync()
    stream = torch.cuda.Stream()
    b.set_stream(stream.cuda_stream)
    views = [torch.as_tensor(_DeviceView(b.dyn_device_ptr(w), shape), device="cuda")
             for w, shape in zip(ALL, ((n, nv), (n, nv, nv), (n, 2, 6, nv), (n, 2, 12)))]
    b.forward()
    with torch.cuda.stream(stream):
        copies = [v.clone() for v in views]
    stream.synchronize()
    for w in ALL:
        assert np.array_equal(copies[w].cpu().numpy().astype(np.float64), b.dyn(w)), NAMES[w]
    _compare(b, model, xml, q2, v2, [rf, ee], "interface, stream read", base)
    b.sync()
    b.set_stream(None)
    b.set(sim.FIELD_QPOS, qpos)
    b.set(sim.FIELD_QVEL, qvel)
    b.forward()
    # no reset writes the buffers
    before = [b.dyn(w) for w in ALL]
    b.reset()
    mask = np.zeros(n, dtype=bool)
    mask[1::2] = True
    b.reset_where(mask)
    for w in ALL:
        assert np.array_equal(before[w], b.dyn(w)), NAMES[w]
    # a non-finite qvel: the env auto-resets and the re-run writes its row at the reset state
    b.set(sim.FIELD_QPOS, qpos)
    qv = qvel.copy()
    qv[2, 3] = np.nan
    b.set(sim.FIELD_QVEL, qv)
    b.step(1)
    assert b.get(sim.FIELD_WARNING)[2].any()
    got = [b.dyn(w) for w in ALL]
    assert all(np.isfinite(g).all() for g in got)
    ref = dyn_ref.refs(model, xml, np.array(model.qpos0), np.zeros(nv), [rf, ee], base)
    for w in ALL:
        assert np.max(np.abs(got[w][2] - ref[w])) <= BAR * max(1.0, np.max(np.abs(ref[w]))), NAMES[w]
    b.set_jac_sites([])
    assert b.layout()["dyn_outputs"] == 3 and b.dyn_device_ptr(sim.DYNOUT_SITE_POSE) is None
    b.close()


def test_gravity_compensation_end_to_end(monkeypatch):
    """11: a use.  The 7-DoF arm with motor actuators (gear 1: ctrl is the joint torque), no joint damping and
    no friction loss, gravity on, posed and at rest.  Each control period qfrc_bias is read on the device,
    copied into the bound ctrl tensor, and the batch steps once; everything is queued on one stream.

    The drift bound, from the state convention.  The bias read before step k belongs to the forward pass of
    step k - 1, i.e. to (q_{k-1}, v_{k-1}): it is one step old.  With tau = bias_{k-1} the arm obeys
        M vdot = bias_{k-1} - bias_k + delta,   bias_k - bias_{k-1} = h G v + O(h^2, h |v| |vdot|),
    G = d qfrc_bias / d qpos at rest (the gravity term's gradient), delta the error of the torque itself.  In
    2-norms |vdot| <= lam |v| + a with
        lam = h |G| / lmin(M),    a = sqrt(nv) eps_tau / lmin(M),    eps_tau = 1e-5 max(1, max |bias|),
    eps_tau being the bar this file holds every element of qfrc_bias to.  From rest, v(t) <= a (e^{lam t} - 1)
    / lam and the drift |q(T) - q(0)| <= a (e^{lam T} - 1 - lam T) / lam^2, T = 200 h.  M, G and max |bias| are
    the fp64 oracle's at the start pose; their change along the drift and the velocity part of the bias are of
    second order in the drift, and a factor 2 on the bound covers them.  (From exact rest the kernel's own bias
    cancels the torque bit for bit, so the measured drift may be exactly zero; the bound does not rely on it.)
    Without the compensation the same arm falls by more than ten times the bound."""
    import torch
    _env(monkeypatch)
    xml, base = ARM7.read_text(), str(ARM7.parent)
    joint = '<joint damping="0.5" armature="0.02" frictionloss="0.1" range="-2.9 2.9"/>'
    assert joint in xml and xml.count("<position name=") == 7
    xml = xml.replace(joint, '<joint armature="0.02" range="-2.9 2.9"/>').replace("<position name=", "<motor name=")
    model = sim.Model.from_string(xml, base)
    n, nv, steps = 4, model.nv, 200
    h = model.view.timestep
    rng = np.random.default_rng(11)
    qpos = rng.uniform(-1.0, 1.0, (n, nv))
    qpos[:, 1] = rng.uniform(0.8, 1.2, n)  # (the shoulder bent: gravity torques of tens of N m)
    qpos = qpos.astype(np.float32).astype(np.float64)
    bounds = []
    for e in range(n):
        d = binding.OracleData(model)
        d.qpos[:] = qpos[e]
        lmin = float(np.linalg.eigvalsh(d.mass_matrix())[0])
        G = np.zeros((nv, nv))
        for j in range(nv):
            dq = np.zeros(nv)
            dq[j] = 1e-4
            G[:, j] = (dyn_ref.bias_ref(xml, qpos[e] + dq, np.zeros(nv), base)
                       - dyn_ref.bias_ref(xml, qpos[e] - dq, np.zeros(nv), base)) / 2e-4
        gmax = float(np.max(np.abs(dyn_ref.bias_ref(xml, qpos[e], np.zeros(nv), base))))
        lam = h * np.linalg.norm(G, 2) / lmin
        a = np.sqrt(nv) * BAR * max(1.0, gmax) / lmin
        T = steps * h
        bounds.append(2 * a * (np.exp(lam * T) - 1 - lam * T) / lam ** 2)
        print(f"env {e}: lmin(M) {lmin:.3g}, |G| {np.linalg.norm(G, 2):.3g}, max |bias| {gmax:.3g}, "
              f"lam {lam:.3g} /s, bound {bounds[-1]:.3g} rad")
    drift = {}
    for comp in (True, False):
        b = sim.Batch(model, n)
        b.set(sim.FIELD_QPOS, qpos)
        b.sync()
        stream = torch.cuda.Stream()
        b.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            ctrl = torch.zeros((n, model.nu), dtype=torch.float32, device="cuda")
        stream.synchronize()
        b.bind_ctrl_device(ctrl.data_ptr())
        if comp:
            bias = torch.as_tensor(_DeviceView(b.dyn_device_ptr(sim.DYNOUT_QFRC_BIAS), (n, nv)), device="cuda")
            b.forward()  # (the bias of the start state for the first period)
        for _ in range(steps):
            if comp:
                with torch.cuda.stream(stream):
                    ctrl.copy_(bias)
            b.step(1)
        b.sync()
        drift[comp] = np.linalg.norm(b.get(sim.FIELD_QPOS) - qpos, axis=1)
        b.bind_ctrl_device(None)
        b.set_stream(None)
        b.close()
    for e in range(n):
        print(f"env {e}: drift compensated {drift[True][e]:.3g} rad, uncompensated {drift[False][e]:.3g} rad, bound {bounds[e]:.3g}")
    for e in range(n):
        assert drift[True][e] <= bounds[e], (e, drift[True][e], bounds[e])
        assert drift[False][e] > 10 * bounds[e], (e, drift[False][e], bounds[e])
