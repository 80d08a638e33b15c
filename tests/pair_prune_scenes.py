"""Scenes and the reach bound of the pair-pruning tests (test_pair_prune.py, test_gpu_pair_prune.py).

The bound is restated here in numpy from its definition, independently of devtables.h: every geom gets a
ball (centre fixed in the world, radius rho) that holds its centre at every qpos -- its own position
for a geom welded to the world; the first joint's anchor and rho = sum |a_i - a_(i-1)| + |x_g - a_k| for
a geom below hinge / ball joints only, one per body -- and an automatic pair is pruned when the balls,
the bounding spheres and the margin leave a gap (with the slack for the device's fp32 poses)."""
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
C3 = (ROOT / "scenes" / "arm7_lidar.xml").read_text()
BOX_N = '<geom name="box_n" class="env" type="box" pos="0.2 2.4 0.5" size="0.5 0.3 0.5"/>'
JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = 0, 1, 2, 3
GEOM_PLANE = 0


def c3_box_n_at(y: float) -> str:
    """C3 with box_n's centre moved to (0.2, y, 0.5)"""
    assert BOX_N in C3
    return C3.replace(BOX_N, BOX_N.replace('pos="0.2 2.4 0.5"', f'pos="0.2 {y} 0.5"'))


def c3_slide_root() -> str:
    """C3 with the arm's base on a slide joint: every arm geom is unbounded"""
    old = '<body name="base" pos="0 0 0">'
    assert old in C3
    return C3.replace(old, old + '\n      <joint name="rail" type="slide" axis="1 0 0" damping="5"/>')


def c3_free_body() -> str:
    """C3 with a free ball far from everything: unbounded, so its pairs stay however far it starts"""
    old = '<body name="lidar_post"'
    assert old in C3
    return C3.replace(old, '<body name="stray" pos="40 40 1"><freejoint/>'
                      '<geom name="stray" type="sphere" size="0.1" contype="3" conaffinity="3"/></body>\n    ' + old, 1)


def c3_mocap() -> str:
    """C3 with a mocap body far from the arm that carries a box the arm may collide with, and a welded
    child of it: both follow per-env mocap poses, so neither is bounded"""
    old = '<body name="lidar_post"'
    assert old in C3
    return C3.replace(old, '<body name="hand" mocap="true" pos="30 0 1">'
                      '<geom name="hand" class="env" type="box" size="0.1 0.1 0.1"/>'
                      '<body name="finger" pos="0 0 0.3"><geom name="finger" class="env" type="sphere" size="0.05"/></body>'
                      '</body>\n    ' + old, 1)


def c3_explicit() -> str:
    """C3 with explicit pairs between the last link and two boxes: both are out of reach and stay"""
    old = '<actuator>'
    assert old in C3
    return C3.replace(old, '<contact>\n    <pair geom1="g7" geom2="box_e" condim="3"/>\n'
                      '    <pair geom1="box_s" geom2="g6" condim="1" margin="0.01"/>\n  </contact>\n\n  ' + old, 1)


# a branched hinge tree on a welded, rotated stand: a jointless body inside the chain, a ball joint, joints
# away from their bodies' origins, a second plane below everything, boxes in and out of reach
TREE = """
<mujoco model="tree">
  <compiler angle="radian"/>
  <option timestep="0.002"/>
  <default>
    <geom contype="2" conaffinity="1" condim="3"/>
    <default class="env"><geom contype="1" conaffinity="2"/></default>
  </default>
  <worldbody>
    <geom name="floor" class="env" type="plane" size="0 0 0.05"/>
    <geom name="pit" class="env" type="plane" pos="0 0 -3" size="0 0 0.05"/>
    <geom name="tilted" class="env" type="plane" pos="-1.5 0 0" euler="0 0.9 0" size="0 0 0.05"/>
    <geom name="near" class="env" type="box" pos="0.9 0.2 1.1" size="0.1 0.2 0.1"/>
    <geom name="mid" class="env" type="box" pos="0.2 1.25 1.0" size="0.15 0.15 0.3" euler="0 0 0.5"/>
    <geom name="far" class="env" type="sphere" pos="-2.5 -1 1.5" size="0.3" margin="0.02"/>
    <body name="stand" pos="0.1 -0.2 0" euler="0 0 0.7">
      <geom name="stand" type="cylinder" size="0.08 0.4" pos="0 0 0.4" contype="0" conaffinity="0"/>
      <body name="trunk" pos="0 0 0.8" euler="0.2 0 0">
        <joint name="t1" type="hinge" axis="0 0 1" pos="0.02 0 0.05"/>
        <geom name="trunk" type="capsule" fromto="0 0 0 0 0 0.4" size="0.05"/>
        <body name="fork" pos="0 0 0.4" euler="0 0.3 0">
          <geom name="fork" type="sphere" size="0.07" pos="0.01 0 0"/>
          <body name="left" pos="0 0.1 0.05">
            <joint name="l1" type="hinge" axis="1 0 0" pos="0 -0.03 0"/>
            <geom name="left" type="capsule" fromto="0 0 0 0 0.3 0.1" size="0.04"/>
            <body name="left2" pos="0 0.3 0.1">
              <joint name="l2" type="ball"/>
              <geom name="left2" type="box" size="0.03 0.1 0.03" pos="0 0.1 0"/>
            </body>
          </body>
          <body name="right" pos="0 -0.1 0.05">
            <joint name="r1" type="hinge" axis="0 1 1"/>
            <geom name="right" type="capsule" fromto="0 0 0 0.05 -0.25 0" size="0.04"/>
            <body name="right2" pos="0.05 -0.25 0">
              <joint name="r2" type="hinge" axis="0 0 1" pos="0 0 0.02"/>
              <geom name="right2" type="ellipsoid" size="0.03 0.08 0.03" pos="0 -0.08 0"/>
            </body>
          </body>
        </body>
      </body>
    </body>
  </worldbody>
</mujoco>
"""


# perturbations within +-1.5 rad that fold the arm over onto the floor (joints 2 and 4 bend the same way:
# the links past joint 4, 0.7 m of them, point down from 0.64 m).  Uniform draws alone do not get there:
# none of 480 drawn envs touched the floor within 30 steps of the fp64 oracle
C3_FOLDS = [(0, 1.5, 0, 1.5, 0, 0, 0), (0.7, 1.4, 0, 1.5, 0, 0.2, 0), (-1.0, -1.5, 0, -1.5, 0, 0, 0),
            (1.5, 1.3, 0, 1.4, 0, 0.4, 0)]


def c3_start_qpos(model, n, seed):
    """synth.initial_qpos perturbed by +-1.5 rad: the first envs by C3_FOLDS, the others uniformly"""
    from mujoco_ros2_simulation_amd import synth
    rng = np.random.default_rng(seed)
    base = synth.initial_qpos(model, np.arange(n))
    dq = rng.uniform(-1.5, 1.5, base.shape)
    dq[:len(C3_FOLDS)] = C3_FOLDS
    assert np.all(np.abs(dq) <= 1.5)
    return base + dq, rng


def _rot(q, v):
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R @ np.asarray(v, dtype=np.float64)


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def reach_balls(m):
    """per geom (bounded, centre [3], rho), and per body its world frame (pos, quat) with every joint
    at its reference, where the distances that no joint changes are measured"""
    pos, quat = [np.zeros(3)], [np.array([1.0, 0, 0, 0])]
    for b in range(1, m.nbody):
        p = m.body_parentid[b]
        pos.append(pos[p] + _rot(quat[p], m.body_pos[b]))
        quat.append(_qmul(quat[p], m.body_quat[b] / np.linalg.norm(m.body_quat[b])))
    mocap = getattr(m, "body_mocapid", np.full(m.nbody, -1))
    body = [dict(bounded=True, fixed=True, c=np.zeros(3), last=np.zeros(3), rho=0.0)]
    for b in range(1, m.nbody):
        r = dict(body[m.body_parentid[b]])
        if mocap[b] >= 0 or m.body_jntnum[b] > 1:
            r["bounded"] = False
        if r["bounded"] and m.body_jntnum[b] == 1:
            j = m.body_jntadr[b]
            if m.jnt_type[j] not in (JNT_HINGE, JNT_BALL):
                r["bounded"] = False
            else:
                a = pos[b] + _rot(quat[b], m.jnt_pos[j])
                if r["fixed"]:
                    r["c"] = a
                else:
                    r["rho"] = r["rho"] + np.linalg.norm(a - r["last"])
                r["last"], r["fixed"] = a, False
        body.append(r)
    out = []
    for g in range(m.ngeom):
        b = m.geom_bodyid[g]
        r = body[b]
        x = pos[b] + _rot(quat[b], m.geom_pos[g])
        if not r["bounded"]:
            out.append((False, None, None))
        elif r["fixed"]:
            out.append((True, x, 0.0))
        else:
            out.append((True, r["c"], r["rho"] + np.linalg.norm(x - r["last"])))
    return out, pos, quat


def welded_to_world(m, b) -> bool:
    mocap = getattr(m, "body_mocapid", np.full(m.nbody, -1))
    while b != 0:
        if m.body_jntnum[b] > 0 or mocap[b] >= 0:
            return False
        b = m.body_parentid[b]
    return True


def expected_pruned(m, pairs, nexplicit) -> list:
    """indices into `pairs` ([k, 2] geom ids: the explicit pairs, then the automatic ones) that the bound
    proves apart"""
    balls, pos, quat = reach_balls(m)
    slack = lambda r: r * (1 + 1e-4) + 1e-4  # noqa: E731
    out = []
    for q, (ga, gb) in enumerate(pairs):
        if q < nexplicit:
            continue
        margin = float(np.float32(max(m.geom_margin[ga], m.geom_margin[gb])))
        pa, pb = m.geom_type[ga] == GEOM_PLANE, m.geom_type[gb] == GEOM_PLANE
        if pa and pb:
            continue
        if pa or pb:
            pl, g = (ga, gb) if pa else (gb, ga)
            if not welded_to_world(m, m.geom_bodyid[pl]) or not balls[g][0]:
                continue
            b = m.geom_bodyid[pl]
            n = _rot(_qmul(quat[b], m.geom_quat[pl] / np.linalg.norm(m.geom_quat[pl])), [0, 0, 1])
            o = pos[b] + _rot(quat[b], m.geom_pos[pl])
            if n @ (balls[g][1] - o) > slack(balls[g][2] + m.geom_rbound[g] + margin):
                out.append(q)
            continue
        if not balls[ga][0] or not balls[gb][0]:
            continue
        d = np.linalg.norm(balls[ga][1] - balls[gb][1])
        if d > slack(balls[ga][2] + balls[gb][2] + m.geom_rbound[ga] + m.geom_rbound[gb] + margin):
            out.append(q)
    return out
