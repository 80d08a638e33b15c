"""fp64 reference for per-body Cartesian wrenches (mjData.xfrc_applied), without asking the oracle for
them: the oracle (oracle/oracle.c) has no such input, so the wrenches are turned into what it does take.

  equivalent joint force   Q = sum_b Jp_b' f_b + Jr_b' tau_b, the Jacobians of each body's centre of mass
                           (xipos) by central differences of kinematics() along every unit velocity:
                           Jp[:, j] = (p(q + h e_j) - p(q - h e_j)) / 2h, q + h e_j being mj_integratePos,
                           Jr[:, j] = vee(R+ R-' - R- R+') / 4h; h = 1e-6 as tests/sensor_ref.py.  With
                           qfrc_applied += Q the oracle has MuJoCo's qacc and next state under xfrc_applied.
  force / torque sensors   equal qacc gives equal cacc and cvel, so only cfrc_ext differs: MuJoCo counts a
                           Cartesian wrench as external, and the sensor of site s on body b reads
                           oracle(with Q) - R_s' W, W = sum of f_k over b's subtree for force and
                           sum of tau_k + (xipos_k - p_s) x f_k for torque.
  every other sensor       the oracle's own value under Q.
  RK4                      MuJoCo holds the wrenches over the four stages but evaluates the Jacobians at each
                           stage's state, which a constant qfrc_applied does not: rk4_step restates
                           mj_RungeKutta over the oracle's forward(), with Q of each stage's qpos.

Test infrastructure only."""
import numpy as np

import binding
from mujoco_ros2_simulation_amd import sim, synth
from sensor_ref import H, integrate_pos, quat2mat, quat_mul, subtree_bodies

G = 9.81


class XfrcRef:
    def __init__(self, model):
        self.model = model
        self._d = binding.OracleData(model)
        self._sub = [subtree_bodies(model, b) for b in range(model.nbody)]

    def frames(self, qpos):
        """(xipos [nbody, 3], R [nbody, 3, 3], xpos, xquat) at qpos"""
        m = self.model
        self._d.qpos[:] = qpos
        xpos, xquat, _, _ = self._d.kinematics()
        R = np.array([quat2mat(q) for q in xquat])
        xipos = np.array([xpos[b] + R[b] @ m.body_ipos[b] for b in range(m.nbody)])
        return xipos, R, xpos, xquat

    def jacobians(self, qpos):
        """translational (at xipos) and rotational Jacobians of every body, [nbody, 3, nv] each"""
        m = self.model
        qpos = np.array(qpos, dtype=np.float64)
        Jp, Jr = np.zeros((m.nbody, 3, m.nv)), np.zeros((m.nbody, 3, m.nv))
        for j in range(m.nv):
            e = np.zeros(m.nv)
            e[j] = 1.0
            pp, Rp, _, _ = self.frames(integrate_pos(m, qpos, e, H))
            pm, Rm, _, _ = self.frames(integrate_pos(m, qpos, e, -H))
            Jp[:, :, j] = (pp - pm) / (2 * H)
            for b in range(m.nbody):
                S = Rp[b] @ Rm[b].T - Rm[b] @ Rp[b].T
                Jr[b, :, j] = np.array([S[2, 1], S[0, 2], S[1, 0]]) / (4 * H)
        return Jp, Jr

    def qfrc(self, qpos, xfrc):
        """the joint-space force equivalent to the wrenches xfrc [nbody, 6] (row 0, the world, ignored)"""
        Jp, Jr = self.jacobians(qpos)
        x = np.asarray(xfrc, dtype=np.float64).reshape(self.model.nbody, 6)
        Q = np.zeros(self.model.nv)
        for b in range(1, self.model.nbody):
            Q += Jp[b].T @ x[b, :3] + Jr[b].T @ x[b, 3:]
        return Q

    def correct_ft(self, sensordata, qpos, xfrc):
        """sensordata of the oracle under qfrc_applied = qfrc(qpos, xfrc), with its force / torque sensors
        moved to what they read when the same wrenches are Cartesian (external)"""
        m = self.model
        x = np.asarray(xfrc, dtype=np.float64).reshape(m.nbody, 6)
        out = np.array(sensordata, dtype=np.float64)
        xipos, R, xpos, xquat = self.frames(qpos)
        for i in range(m.nsensor):
            t = m.sensor_type[i]
            if t not in (sim.SENS_FORCE, sim.SENS_TORQUE):
                continue
            s = m.sensor_objid[i]
            b = m.site_bodyid[s]
            ps = xpos[b] + R[b] @ m.site_pos[s]
            Rs = quat2mat(quat_mul(xquat[b], m.site_quat[s]))
            ks = [k for k in self._sub[b] if k != 0]
            if t == sim.SENS_FORCE:
                W = x[ks, :3].sum(axis=0)
            else:
                W = sum((x[k, 3:] + np.cross(xipos[k] - ps, x[k, :3]) for k in ks), np.zeros(3))
            v = out[m.sensor_adr[i]:m.sensor_adr[i] + 3] - Rs.T @ W
            cut = m.sensor_cutoff[i]
            out[m.sensor_adr[i]:m.sensor_adr[i] + 3] = np.clip(v, -cut, cut) if cut > 0 else v
        return out


def draw_wrenches(model, e, t):
    """wrenches [nbody, 6] of env e at step t, rounded to fp32 (Philox uniforms of the env id, as
    synth.initial_qpos): per body a force in a random direction of up to 3 x the body's weight and a torque
    of up to 1 N m.  Two bodies are left at exactly zero -- two of the moving ones, rotating with the env,
    where there are at least three; otherwise the world and (except in every third env) one other."""
    nb = model.nbody
    u = synth.uniforms(np.array([e]), 8 * nb, 3 + t)[0, :, 0].reshape(nb, 8)
    x = np.zeros((nb, 6))
    for b in range(1, nb):
        f, tq = u[b, 0:3] - 0.5, u[b, 4:7] - 0.5
        x[b, :3] = f / max(np.linalg.norm(f), 1e-9) * u[b, 3] * 3 * model.body_mass[b] * G
        x[b, 3:] = tq / max(np.linalg.norm(tq), 1e-9) * u[b, 7]
    if nb - 1 >= 3:
        zero = [1 + e % (nb - 1), 1 + (e + 1 + t % (nb - 2)) % (nb - 1)]
        if zero[0] == zero[1]:
            zero[1] = 1 + (zero[0] % (nb - 1))
    else:
        zero = [0] if e % 3 == 2 else [0, 1 + e % (nb - 1)]
    x[zero] = 0
    return x.astype(np.float32).astype(np.float64)


def rk4_step(model, d, xr, xfrc):
    """mj_RungeKutta(4) under the wrenches xfrc: d is an OracleData after forward() at the step's start
    state with qfrc_applied = xr.qfrc(qpos, xfrc).  Each further stage's forward() gets the Q of its own
    qpos.  Returns the next (qpos, qvel); d is left at the last stage."""
    h = model.view.timestep
    A, B = (0.5, 0.5, 1.0), (1 / 6, 1 / 3, 1 / 3, 1 / 6)
    q0, v0 = d.qpos.copy(), d.qvel.copy()
    v, a = v0.copy(), d.qacc.copy()
    sv, sa = B[0] * v, B[0] * a
    for i in range(1, 4):
        qi, vi = integrate_pos(model, q0, A[i - 1] * v, h), v0 + h * A[i - 1] * a
        d.qpos[:], d.qvel[:] = qi, vi
        d.qfrc_applied[:] = xr.qfrc(qi, xfrc)
        d.forward()
        v, a = vi, d.qacc.copy()
        sv, sa = sv + B[i] * v, sa + B[i] * a
    return integrate_pos(model, q0, sv, h), v0 + h * sa
