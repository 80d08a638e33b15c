"""The two scenes of the velocimeter / frame / subtree / touch sensor tests, without their <sensor>
sections (tests/sensor_ref.py builds a companion model with probe sensors from the same string), and the
sections themselves: the new sensors and the known ones that stay in the scene."""
import numpy as np

from mujoco_ros2_simulation_amd import synth

# A: fixed-base arm, hinge / hinge / slide; sites off their body origins with their own rotations, plus
# plain sites at body and geom origins (the accelerometer probes of framelinacc on bodies and geoms)
ARM = """
<mujoco model="arm_sensors">
  <compiler angle="radian"/>
  <option timestep="0.002" integrator="implicitfast"/>
  <worldbody>
    <geom name="floor" type="plane" size="0 0 0.05" contype="1" conaffinity="1"/>
    <body name="post" pos="-0.3 0 0.8">
      <geom name="post_g" type="box" size="0.03 0.03 0.03" contype="0" conaffinity="0"/>
      %(lidar)s
    </body>
    <body name="l1" pos="0 0 1.2">
      <joint name="j1" type="hinge" axis="0 1 0" damping="0.2"/>
      <geom name="g1" type="capsule" fromto="0 0 0 0.4 0 0" size="0.04" mass="1" contype="0" conaffinity="0"/>
      <site name="s1" pos="0.1 0.02 0.03" quat="0.9238795 0.3826834 0 0"/>
      <site name="s1o" pos="0 0 0"/>
      <body name="l2" pos="0.4 0 0">
        <joint name="j2" type="hinge" axis="0 0 1" damping="0.2"/>
        <geom name="g2" type="box" pos="0.15 0.01 0" quat="0.9659258 0 0.258819 0" size="0.15 0.03 0.03" mass="0.6"
              contype="0" conaffinity="0"/>
        <site name="s2" pos="0.15 0 0.03" quat="0.9659258 0 0 0.258819"/>
        <site name="s2g" pos="0.15 0.01 0"/>
        <site name="s2o" pos="0 0 0"/>
        <body name="l3" pos="0.3 0 0">
          <joint name="j3" type="slide" axis="1 0 0" damping="1"/>
          <geom name="g3" type="sphere" size="0.05" mass="0.5" contype="0" conaffinity="0"/>
          <site name="s3" pos="0.02 0.03 -0.01" quat="0.7071068 0 0.7071068 0"/>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator>
    <motor name="m1" joint="j1"/>
    <motor name="m2" joint="j2"/>
    <motor name="m3" joint="j3" gear="5"/>
  </actuator>
</mujoco>
"""
ARM_LIDAR_SITES = "".join(f'<site name="ray{k}" pos="0 0 0" euler="0 1.5707963 {0.2 * k - 0.7:.4f}"/>' for k in range(8))
ARM_LIDAR = "".join(f'<rangefinder name="ray{k}" site="ray{k}"/>' for k in range(8))


def _frames(tag, objs):
    return "".join(f'<{tag} name="{tag}_{n}" objtype="{t}" objname="{n}"/>' for t, n in objs)


_OBJS = [("site", "s2"), ("body", "l2"), ("geom", "g2")]
# 25 new sensors: more than one per lane of a 16-lane group
ARM_SENSORS = (
    '<velocimeter name="vel_s1" site="s1"/><velocimeter name="vel_s3" site="s3"/>'
    + _frames("framelinvel", _OBJS + [("site", "s3")]) + _frames("frameangvel", _OBJS + [("site", "s3")])
    + _frames("framelinacc", [("site", "s2"), ("body", "l2"), ("geom", "g2"), ("site", "s3")])
    + _frames("framexaxis", _OBJS) + _frames("frameyaxis", _OBJS) + _frames("framezaxis", _OBJS)
    + '<subtreecom name="com_l1" body="l1"/><subtreecom name="com_l2" body="l2"/>'
    + '<subtreelinvel name="cvel_l1" body="l1"/><subtreelinvel name="cvel_l2" body="l2"/>')
ARM_KNOWN = ('<framequat name="imu_quat" objtype="site" objname="s2"/><gyro name="imu_gyro" site="s2"/>'
             '<accelerometer name="imu_accel" site="s2"/><framepos name="pos_s3" objtype="site" objname="s3"/>'
             '<jointpos name="q3" joint="j3"/>')

# B: the free box with a hinged child of scenes/imu_ft.xml landing on the floor; a pad enclosing the
# box's underside and a small one inside the box that no contact normal ray meets
FLOAT = """
<mujoco model="float_sensors">
  <compiler angle="radian"/>
  <option timestep="0.002" integrator="implicitfast"%(option)s/>
  <worldbody>
    <geom name="floor" type="plane" size="0 0 0.05" contype="1" conaffinity="1"/>
    <body name="box" pos="0 0 0.13">
      <freejoint name="box_free"/>
      <geom name="box_g" type="box" size="0.1 0.1 0.1" mass="1.5" contype="1" conaffinity="1"/>
      <site name="box_site" pos="0 0 0"/>
      <site name="corner" pos="0.08 -0.05 0.06" quat="0.8 0.2 -0.4 0.4"/>
      <site name="under" type="box" size="0.13 0.13 0.03" pos="0 0 -0.1"/>
      <site name="miss" type="sphere" size="0.01" pos="0.3 0 0.05"/>
      <body name="flap" pos="0.1 0 0.1">
        <joint name="flap_j" type="hinge" axis="0 1 0" damping="0.05"/>
        <geom name="flap_g" type="capsule" fromto="0 0 0 0.15 0 0" size="0.02" mass="0.3" contype="0" conaffinity="0"/>
        <site name="tip" pos="0.15 0 0" quat="0.9238795 0 0.3826834 0"/>
      </body>
    </body>
  </worldbody>
</mujoco>
"""
FLOAT_SENSORS = ('<touch name="under" site="under"/><touch name="miss" site="miss"/>'
                 '<velocimeter name="vel_corner" site="corner"/><velocimeter name="vel_tip" site="tip"/>'
                 '<framelinvel name="lv_corner" objtype="site" objname="corner"/>'
                 '<framelinvel name="lv_box" objtype="body" objname="box"/>'
                 '<framelinacc name="la_box" objtype="site" objname="box_site"/>'
                 '<framelinacc name="la_tip" objtype="site" objname="tip"/>'
                 '<frameangvel name="av_tip" objtype="site" objname="tip"/>'
                 '<subtreecom name="com_box" body="box"/><subtreelinvel name="cvel_box" body="box"/>'
                 '<subtreelinvel name="cvel_flap" body="flap"/>')
FLOAT_KNOWN = ('<accelerometer name="box_accel" site="box_site"/><gyro name="box_gyro" site="corner"/>'
               '<framequat name="box_quat" objtype="site" objname="corner"/>')
FLOAT_OPTIONS = {"pgs_pyramidal": ' solver="PGS" iterations="100"', "newton_pyramidal": ' solver="Newton"',
                 "pgs_elliptic": ' solver="PGS" iterations="100" cone="elliptic"',
                 "newton_elliptic": ' solver="Newton" cone="elliptic"'}


def with_sensors(scene, sensors, lidar=False, option=""):
    xml = scene % {"lidar": ARM_LIDAR_SITES if lidar else "", "option": option}
    return xml.replace("</mujoco>", f"<sensor>{sensors}{ARM_LIDAR if lidar else ''}</sensor></mujoco>")


def bare(scene, lidar=False, option=""):
    return scene % {"lidar": ARM_LIDAR_SITES if lidar else "", "option": option}


def float_start(model, e):
    """env e of the floating scene: the box 3 cm above the floor, tilted a little and moving, each env
    differently (Philox uniforms of the env id, as synth.initial_qpos)"""
    u = synth.uniforms(np.array([e]), 12, 2)[0, :, 0]
    qpos = np.array(model.qpos0, dtype=np.float64)
    qvel = np.zeros(model.nv)
    ax = 0.1 * (u[0:3] - 0.5)
    qpos[3:7] = np.concatenate([[1.0], 0.5 * ax])
    qpos[3:7] /= np.linalg.norm(qpos[3:7])
    qpos[2] += 0.02 * u[3]
    qpos[7] = 0.4 * (u[4] - 0.5)
    qvel[0:3] = [0.3 * (u[5] - 0.5), 0.3 * (u[6] - 0.5), -0.2 * u[7]]
    qvel[3:6] = 1.0 * (u[8:11] - 0.5)
    qvel[6] = 2.0 * (u[11] - 0.5)
    return qpos, qvel
