"""fp64 reference for the per-contact forces (mj_contactForce) and the net contact wrench per body, from
oracle quantities that are pinned elsewhere: OracleData.contacts(), the contact rows of efc() in contact
order (paired as tests/sensor_ref.py::_touch_at pairs them), and kinematics() plus the model's body_ipos
for the bodies' centres of mass (xfrc_ref.XfrcRef.frames).

  contact-frame force   condim 1: the row's force; elliptic cone: the block's three rows as they are;
                        pyramidal cone (mju_decodePyramid): normal = sum of the four edge forces, tangent k =
                        (f[2k] - f[2k+1]) * mu, mu the pair's sliding friction -- max of the two geoms', or
                        the explicit <contact><pair>'s own.
  world force           F = frame' lf (frame rows: normal, tangent 1, tangent 2; the normal points from geom1
                        to geom2) acts on geom2's body at the contact point, -F on geom1's.
  wrench of body b      [0:3] the sum of those forces, [3:6] their torque about xipos_b (the world, b = 0:
                        about the origin) -- xfrc_applied's layout and reference point.

Test infrastructure only."""
import numpy as np

from sensor_ref import EFC_CONTACT


def pair_params(model, g1, g2, friction=None):
    """(condim, sliding friction) of the contact pair (g1, g2); friction: the geoms' sliding friction
    [ngeom] in place of the model's (a per-env MRS_PARAM_GEOM_FRICTION row), which an explicit pair ignores"""
    for q in range(getattr(model, "nexpair", 0)):
        if {int(model.expair_geom1[q]), int(model.expair_geom2[q])} == {int(g1), int(g2)}:
            return int(model.expair_dim[q]), float(model.expair_friction[q][0])
    f = model.geom_friction[:, 0] if friction is None else np.asarray(friction, dtype=np.float64)
    return int(max(model.geom_condim[g1], model.geom_condim[g2])), float(max(f[g1], f[g2]))


def contact_forces(model, d, friction=None):
    """[ncon, 6] contact-frame forces of the oracle's last forward pass (normal, tangent 1, tangent 2, then
    three zeros: condim 1 and 3 carry no torque), in contacts()' order"""
    geoms = d.contacts()[0]
    efc = d.efc()
    rows = np.flatnonzero(efc["type"] == EFC_CONTACT)
    out = np.zeros((len(geoms), 6))
    r = 0
    for c, (g1, g2) in enumerate(geoms):
        dim, mu = pair_params(model, g1, g2, friction)
        assert dim in (1, 3), "condim 4 and 6 are not part of the project"
        nr = 1 if dim == 1 else (3 if model.view.cone == 1 else 4)
        f = efc["force"][rows[r:r + nr]]
        r += nr
        if dim == 1:
            out[c, 0] = f[0]
        elif model.view.cone == 1:
            out[c, :3] = f
        else:
            out[c, :3] = [f.sum(), (f[0] - f[1]) * mu, (f[2] - f[3]) * mu]
    assert r == len(rows), "contact rows do not match the contacts"
    return out


def wrenches(model, geoms, pos, frame, forces, xipos):
    """[nbody, 6] net contact wrench per body from contacts (geoms [n, 2], pos [n, 3], frame [n, 9]), their
    contact-frame forces [n, 6] and the bodies' centres of mass xipos [nbody, 3]"""
    W = np.zeros((model.nbody, 6))
    ref = np.array(xipos, dtype=np.float64)
    ref[0] = 0
    for c, (g1, g2) in enumerate(geoms):
        F = np.asarray(frame[c], dtype=np.float64).reshape(3, 3).T @ forces[c, :3]
        for b, sg in ((model.geom_bodyid[g2], 1.0), (model.geom_bodyid[g1], -1.0)):
            W[b, :3] += sg * F
            W[b, 3:] += sg * np.cross(pos[c] - ref[b], F)
    return W


def contact_wrench(model, d, xipos, friction=None):
    """(per-contact contact-frame forces [ncon, 6], wrenches [nbody, 6]) of the oracle's last forward
    pass; xipos [nbody, 3] at that pass's qpos (XfrcRef.frames(qpos)[0])"""
    geoms, _, pos, frame = d.contacts()
    forces = contact_forces(model, d, friction)
    return forces, wrenches(model, geoms, pos, frame, forces, xipos)


# ---- the known-answer scene of the reference's own test and of the GPU test: a free sphere dropped onto
# the floor with a tangential velocity and a spin.  The contact is the only force besides gravity, so the
# sphere's row is m (a_lin + g) and, the inertia being isotropic, its torque I R alpha (R: the body's
# rotation; a free joint's angular acceleration is in the body frame), both from qacc
SPHERE_R, SPHERE_M = 0.1, 0.8
SPHERE = f"""
<mujoco model="drop_sphere">
  <option timestep="0.002"%(option)s/>
  <worldbody>
    <geom name="floor" type="plane" size="0 0 0.05"/>
    <body name="ball" pos="0 0 {SPHERE_R + 0.001}">
      <freejoint name="ball_free"/>
      <geom name="ball_g" type="sphere" size="{SPHERE_R}" mass="{SPHERE_M}" friction="0.7 0.005 0.0001"/>
    </body>
  </worldbody>
</mujoco>
"""


def sphere_start(model, e):
    """env e: 1 mm above the floor, falling at 0.2 m/s, sliding and spinning, each env differently"""
    qpos = np.array(model.qpos0, dtype=np.float64)
    qvel = np.zeros(model.nv)
    qvel[0:3] = [0.5 + 0.1 * e, -0.3 + 0.05 * e, -0.2]
    qvel[3:6] = [1.0, 2.0 - 0.3 * e, -0.5]
    return qpos, qvel


def sphere_known(qpos, qacc, g=9.81):
    """the sphere's wrench [6] from qacc at qpos: m (a_lin + g), then I R alpha"""
    from sensor_ref import quat2mat
    R = quat2mat(np.asarray(qpos[3:7], dtype=np.float64) / np.linalg.norm(qpos[3:7]))
    inertia = 0.4 * SPHERE_M * SPHERE_R ** 2
    return np.concatenate([SPHERE_M * (np.asarray(qacc[0:3]) + [0, 0, g]), inertia * (R @ np.asarray(qacc[3:6]))])
