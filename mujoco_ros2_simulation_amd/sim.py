"""ctypes binding of the C ABI (include/mrs.h) — the host-side mirror used by tests, bench and the
plugin harness.  The product path is libmrs.so (HIP kernels for gfx950); there is no CPU fallback:
if the library or a GPU is missing, the calls raise.

Reference mapping (reference repo paths):
  Model.load        -> mj_loadXML            src/mujoco_system_interface.cpp:318
  Model.from_string -> mj_parseXMLString+mj_compile  :398-399
  Model.name2id     -> mj_name2id            :1193,1213,1496-1497,1527-1529
  Batch             -> N x mjData             mj_makeData :686-687
  Batch.step        -> mj_step               :1691,1731
  Batch.forward     -> mj_forward            :741,1771
  Batch.render_depth-> mjr_render+mjr_readPixels+linearise  src/mujoco_cameras.cpp:211-240
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["MRS_LIB"]) if os.environ.get("MRS_LIB") else _PKG / "libmrs.so"

# enums mirrored from include/mrs_model.h / include/mrs.h
GEOM_PLANE, GEOM_HFIELD, GEOM_SPHERE, GEOM_CAPSULE, GEOM_ELLIPSOID, GEOM_CYLINDER, GEOM_BOX, GEOM_MESH = range(8)
JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = range(4)
OBJ_BODY, OBJ_JOINT, OBJ_GEOM, OBJ_SITE, OBJ_CAMERA, OBJ_ACTUATOR, OBJ_SENSOR = 1, 3, 5, 6, 7, 19, 20
OBJ_TENDON = 18
SENS_ACCELEROMETER, SENS_GYRO, SENS_FORCE, SENS_TORQUE, SENS_RANGEFINDER = 1, 3, 4, 5, 7
SENS_JOINTPOS, SENS_JOINTVEL, SENS_ACTUATORFRC, SENS_FRAMEPOS, SENS_FRAMEQUAT = 9, 10, 15, 25, 26
SENS_TOUCH, SENS_VELOCIMETER, SENS_FRAMEXAXIS, SENS_FRAMEYAXIS, SENS_FRAMEZAXIS = 0, 2, 27, 28, 29
SENS_FRAMELINVEL, SENS_FRAMEANGVEL, SENS_FRAMELINACC, SENS_SUBTREECOM, SENS_SUBTREELINVEL = 30, 31, 32, 34, 35
SENS_TENDONPOS, SENS_TENDONVEL = 11, 12
BIAS_NONE, BIAS_AFFINE = 0, 1
RESTATE_NEWTON_REFINE, RESTATE_PGS_ELLIPTIC_BLOCK, RESTATE_NO_MPR_POLISH, RESTATE_NO_MULTICCD = 1, 2, 4, 8
(FIELD_QPOS, FIELD_QVEL, FIELD_CTRL, FIELD_QFRC_APPLIED, FIELD_QACC_WARMSTART, FIELD_QACC,
 FIELD_QFRC_ACTUATOR, FIELD_SENSORDATA, FIELD_TIME, FIELD_WARNING, FIELD_NCON, FIELD_SOLVER_NITER,
 FIELD_XFRC_APPLIED) = range(13)
# per-env body mass / inertia / dof armature (MRS_INERTIAL_*; Batch.get_inertial / set_inertial)
INERTIAL_BODY_MASS, INERTIAL_BODY_INERTIA, INERTIAL_DOF_ARMATURE, INERTIAL_COUNT = 0, 1, 2, 3
# per-env model parameters (MRS_PARAM_*; Batch.get_model_param / set_model_param)
PARAM_ACT_GAINPRM, PARAM_ACT_BIASPRM, PARAM_DOF_DAMPING, PARAM_GEOM_FRICTION = range(4)
# the dynamics outputs (MRS_DYNOUT_*; Batch.dyn / dyn_device_ptr / set_jac_sites).  Not DYN_*: those are
# the actuator dyntypes below
DYNOUT_QFRC_BIAS, DYNOUT_MASS_MATRIX, DYNOUT_SITE_JAC, DYNOUT_SITE_POSE, DYNOUT_COUNT = 0, 1, 2, 3, 4
MAX_JAC_SITES = 16
# ray queries (MRS_RAY_*; Batch.ray / ray_device): flags, then frame types
RAY_SHARED, RAY_NO_STATIC = 1, 2
RAY_FRAME_WORLD, RAY_FRAME_GEOM, RAY_FRAME_CAMERA = 0, 1, 2
_RAY_FRAMES = {"world": RAY_FRAME_WORLD, "geom": RAY_FRAME_GEOM, "camera": RAY_FRAME_CAMERA}
# ActuatorType (include/mujoco_ros2_control/data.hpp:43-51 numbering)
ACT_UNKNOWN, ACT_MOTOR, ACT_POSITION, ACT_VELOCITY, ACT_CUSTOM = range(5)

MRS_OK = 0
ERRORS = {-1: "invalid argument", -2: "load error", -3: "device error", -4: "unsupported"}


class MrsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


# (name, kind, size-expression) in exactly the order of struct mrs_model_view
_SIZES = ["nq", "nv", "nu", "na", "nbody", "njnt", "ngeom", "nsite", "ncam", "nsensor", "nsensordata", "nkey",
          "nM", "max_depth", "npair"]
_ARRAYS = [
    ("body_parentid", "i", "nbody", 1), ("body_rootid", "i", "nbody", 1), ("body_weldid", "i", "nbody", 1),
    ("body_jntnum", "i", "nbody", 1), ("body_jntadr", "i", "nbody", 1), ("body_dofnum", "i", "nbody", 1),
    ("body_dofadr", "i", "nbody", 1), ("body_geomnum", "i", "nbody", 1), ("body_geomadr", "i", "nbody", 1),
    ("body_depth", "i", "nbody", 1),
    ("body_pos", "d", "nbody", 3), ("body_quat", "d", "nbody", 4), ("body_ipos", "d", "nbody", 3),
    ("body_iquat", "d", "nbody", 4), ("body_mass", "d", "nbody", 1), ("body_subtreemass", "d", "nbody", 1),
    ("body_inertia", "d", "nbody", 3), ("body_invweight0", "d", "nbody", 2), ("body_gravcomp", "d", "nbody", 1),
    ("jnt_type", "i", "njnt", 1), ("jnt_qposadr", "i", "njnt", 1), ("jnt_dofadr", "i", "njnt", 1),
    ("jnt_bodyid", "i", "njnt", 1), ("jnt_limited", "i", "njnt", 1), ("jnt_actfrclimited", "i", "njnt", 1),
    ("jnt_pos", "d", "njnt", 3), ("jnt_axis", "d", "njnt", 3), ("jnt_stiffness", "d", "njnt", 1),
    ("jnt_range", "d", "njnt", 2), ("jnt_actfrcrange", "d", "njnt", 2), ("jnt_margin", "d", "njnt", 1),
    ("jnt_solref", "d", "njnt", 2), ("jnt_solimp", "d", "njnt", 5),
    ("dof_bodyid", "i", "nv", 1), ("dof_jntid", "i", "nv", 1), ("dof_parentid", "i", "nv", 1),
    ("dof_armature", "d", "nv", 1), ("dof_damping", "d", "nv", 1), ("dof_frictionloss", "d", "nv", 1),
    ("dof_solref", "d", "nv", 2), ("dof_solimp", "d", "nv", 5), ("dof_invweight0", "d", "nv", 1),
    ("dof_M0", "d", "nv", 1),
    ("geom_type", "i", "ngeom", 1), ("geom_contype", "i", "ngeom", 1), ("geom_conaffinity", "i", "ngeom", 1),
    ("geom_condim", "i", "ngeom", 1), ("geom_bodyid", "i", "ngeom", 1), ("geom_group", "i", "ngeom", 1),
    ("geom_priority", "i", "ngeom", 1),
    ("geom_size", "d", "ngeom", 3), ("geom_pos", "d", "ngeom", 3), ("geom_quat", "d", "ngeom", 4),
    ("geom_rbound", "d", "ngeom", 1), ("geom_friction", "d", "ngeom", 3), ("geom_margin", "d", "ngeom", 1),
    ("geom_gap", "d", "ngeom", 1), ("geom_solmix", "d", "ngeom", 1), ("geom_solref", "d", "ngeom", 2),
    ("geom_solimp", "d", "ngeom", 5), ("geom_rgba", "d", "ngeom", 4),
    ("site_bodyid", "i", "nsite", 1), ("site_pos", "d", "nsite", 3), ("site_quat", "d", "nsite", 4),
    ("cam_bodyid", "i", "ncam", 1), ("cam_resolution", "i", "ncam", 2), ("cam_pos", "d", "ncam", 3),
    ("cam_quat", "d", "ncam", 4), ("cam_fovy", "d", "ncam", 1),
    ("actuator_trntype", "i", "nu", 1), ("actuator_dyntype", "i", "nu", 1), ("actuator_gaintype", "i", "nu", 1),
    ("actuator_biastype", "i", "nu", 1), ("actuator_trnid", "i", "nu", 2), ("actuator_ctrllimited", "i", "nu", 1),
    ("actuator_forcelimited", "i", "nu", 1),
    ("actuator_gear", "d", "nu", 6), ("actuator_gainprm", "d", "nu", 10), ("actuator_biasprm", "d", "nu", 10),
    ("actuator_ctrlrange", "d", "nu", 2), ("actuator_forcerange", "d", "nu", 2),
    ("sensor_type", "i", "nsensor", 1), ("sensor_objtype", "i", "nsensor", 1), ("sensor_objid", "i", "nsensor", 1),
    ("sensor_dim", "i", "nsensor", 1), ("sensor_adr", "i", "nsensor", 1), ("sensor_cutoff", "d", "nsensor", 1),
    ("qpos0", "d", "nq", 1), ("qpos_spring", "d", "nq", 1),
    ("key_time", "d", "nkey", 1), ("key_qpos", "d", "nkey", "nq"), ("key_qvel", "d", "nkey", "nv"),
    ("key_ctrl", "d", "nkey", "nu"),
    ("pair_geom1", "i", "npair", 1), ("pair_geom2", "i", "npair", 1),
]
# mesh block (after the arrays above in struct mrs_model_view)
_MESH_SIZES = ["nmesh", "nmeshvert", "nmeshface", "nmeshhull"]
_MESH_ARRAYS = [
    ("geom_dataid", "i", "ngeom", 1), ("mesh_vertadr", "i", "nmesh", 1), ("mesh_vertnum", "i", "nmesh", 1),
    ("mesh_faceadr", "i", "nmesh", 1), ("mesh_facenum", "i", "nmesh", 1), ("mesh_hulladr", "i", "nmesh", 1),
    ("mesh_hullnum", "i", "nmesh", 1), ("mesh_face", "i", "nmeshface", 3), ("mesh_hull", "i", "nmeshhull", 1),
    ("mesh_vert", "d", "nmeshvert", 3),
]
# explicit contact pairs and excluded body pairs (after the mesh block)
_CONTACT_SIZES = ["nexpair", "nexclude"]
_CONTACT_ARRAYS = [
    ("expair_geom1", "i", "nexpair", 1), ("expair_geom2", "i", "nexpair", 1), ("expair_dim", "i", "nexpair", 1),
    ("exclude_body1", "i", "nexclude", 1), ("exclude_body2", "i", "nexclude", 1),
    ("expair_friction", "d", "nexpair", 5), ("expair_solref", "d", "nexpair", 2), ("expair_solimp", "d", "nexpair", 5),
    ("expair_margin", "d", "nexpair", 1), ("expair_gap", "d", "nexpair", 1),
]
# equality constraints (after the contact block)
_EQ_SIZES = ["neq"]
_EQ_ARRAYS = [
    ("eq_type", "i", "neq", 1), ("eq_obj1id", "i", "neq", 1), ("eq_obj2id", "i", "neq", 1), ("eq_active0", "i", "neq", 1),
    ("eq_solref", "d", "neq", 2), ("eq_solimp", "d", "neq", 5), ("eq_data", "d", "neq", 11),
]
EQ_CONNECT, EQ_WELD, EQ_JOINT = 0, 1, 2
# rendering (after the equality block; vis_headlight is a fixed double[10] before the sizes)
_REND_SIZES = ["nlight", "ntex", "nmat"]
_REND_ARRAYS = [
    ("light_directional", "i", "nlight", 1), ("light_castshadow", "i", "nlight", 1), ("light_active", "i", "nlight", 1),
    ("tex_type", "i", "ntex", 1), ("tex_builtin", "i", "ntex", 1), ("tex_mark", "i", "ntex", 1),
    ("tex_width", "i", "ntex", 1), ("tex_height", "i", "ntex", 1), ("mat_texid", "i", "nmat", 1),
    ("mat_texuniform", "i", "nmat", 1), ("geom_matid", "i", "ngeom", 1),
    ("light_pos", "d", "nlight", 3), ("light_dir", "d", "nlight", 3), ("light_ambient", "d", "nlight", 3),
    ("light_diffuse", "d", "nlight", 3), ("light_specular", "d", "nlight", 3), ("light_attenuation", "d", "nlight", 3),
    ("light_cutoff", "d", "nlight", 1), ("light_exponent", "d", "nlight", 1), ("tex_rgb1", "d", "ntex", 3),
    ("tex_rgb2", "d", "ntex", 3), ("tex_markrgb", "d", "ntex", 3), ("mat_rgba", "d", "nmat", 4),
    ("mat_texrepeat", "d", "nmat", 2), ("mat_specular", "d", "nmat", 1), ("mat_shininess", "d", "nmat", 1),
    ("mat_emission", "d", "nmat", 1),
]
TEX_2D, TEX_CUBE, TEX_SKYBOX = 0, 1, 2
# fixed tendons (after the rendering block)
_TEN_SIZES = ["ntendon", "nwrap"]
_TEN_ARRAYS = [
    ("tendon_adr", "i", "ntendon", 1), ("tendon_num", "i", "ntendon", 1), ("tendon_limited", "i", "ntendon", 1),
    ("wrap_objid", "i", "nwrap", 1), ("wrap_prm", "d", "nwrap", 1), ("tendon_range", "d", "ntendon", 2),
    ("tendon_margin", "d", "ntendon", 1), ("tendon_solref_lim", "d", "ntendon", 2),
    ("tendon_solimp_lim", "d", "ntendon", 5), ("tendon_frictionloss", "d", "ntendon", 1),
    ("tendon_solref_fri", "d", "ntendon", 2), ("tendon_solimp_fri", "d", "ntendon", 5),
    ("tendon_stiffness", "d", "ntendon", 1), ("tendon_damping", "d", "ntendon", 1),
    ("tendon_lengthspring", "d", "ntendon", 2), ("tendon_invweight0", "d", "ntendon", 1),
    ("tendon_length0", "d", "ntendon", 1),
]
TRN_JOINT, TRN_TENDON, TRN_SITE = 0, 3, 4
# mesh hull polygons (after the tendon block)
_POLY_SIZES = ["nmeshpoly", "nmeshpolyvert"]
_POLY_ARRAYS = [
    ("mesh_polyadr", "i", "nmesh", 1), ("mesh_polynum", "i", "nmesh", 1), ("mesh_polyvertadr", "i", "nmeshpoly", 1),
    ("mesh_polyvertnum", "i", "nmeshpoly", 1), ("mesh_polyvert", "i", "nmeshpolyvert", 1),
    ("mesh_polynormal", "d", "nmeshpoly", 3),
]
# site shapes (after the polygon block)
_SITE_ARRAYS = [("site_type", "i", "nsite", 1), ("site_size", "d", "nsite", 3)]
# activation state (after the site shapes): na stateful actuators, one activation each
_ACT_ARRAYS = [
    ("actuator_actadr", "i", "nu", 1), ("actuator_actnum", "i", "nu", 1), ("actuator_actlimited", "i", "nu", 1),
    ("actuator_actearly", "i", "nu", 1), ("actuator_dynprm", "d", "nu", 3), ("actuator_actrange", "d", "nu", 2),
    ("key_act", "d", "nkey", "na"),
]
DYN_NONE, DYN_INTEGRATOR, DYN_FILTER, DYN_FILTEREXACT = range(4)
# mocap bodies (after the activation block): nmocap, then body_mocapid and the keyframes' poses; a
# width (name, k) is k times that size
_MOCAP_SIZES = ["nmocap"]
_MOCAP_ARRAYS = [("body_mocapid", "i", "nbody", 1), ("key_mpos", "d", "nkey", ("nmocap", 3)),
                 ("key_mquat", "d", "nkey", ("nmocap", 4))]
# tendon paths (after the mocap block): each wrap's type, each tendon's kind.  A fixed tendon's wraps are
# joints (wrap_prm the coefficient), a spatial one's sites and pulleys (wrap_prm the divisor)
_PATH_ARRAYS = [("wrap_type", "i", "nwrap", 1), ("tendon_kind", "i", "ntendon", 1)]
WRAP_NONE, WRAP_JOINT, WRAP_PULLEY, WRAP_SITE = range(4)
TENDON_FIXED, TENDON_SPATIAL = 0, 1


class ModelView(C.Structure):
    _fields_ = ([(n, C.c_int) for n in _SIZES] +
                [("timestep", C.c_double), ("gravity", C.c_double * 3), ("tolerance", C.c_double),
                 ("impratio", C.c_double), ("ls_tolerance", C.c_double),
                 ("integrator", C.c_int), ("solver", C.c_int), ("iterations", C.c_int), ("disableflags", C.c_int),
                 ("cone", C.c_int), ("ls_iterations", C.c_int), ("restate", C.c_int),
                 ("stat_extent", C.c_double), ("stat_center", C.c_double * 3), ("stat_meaninertia", C.c_double),
                 ("vis_znear", C.c_double), ("vis_zfar", C.c_double)] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _ARRAYS] +
                [(n, C.c_int) for n in _MESH_SIZES] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _MESH_ARRAYS] +
                [(n, C.c_int) for n in _CONTACT_SIZES] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _CONTACT_ARRAYS] +
                [(n, C.c_int) for n in _EQ_SIZES] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _EQ_ARRAYS] +
                [("vis_headlight", C.c_double * 10)] + [(n, C.c_int) for n in _REND_SIZES] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _REND_ARRAYS] +
                [(n, C.c_int) for n in _TEN_SIZES] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _TEN_ARRAYS] +
                [(n, C.c_int) for n in _POLY_SIZES] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _POLY_ARRAYS] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _SITE_ARRAYS] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _ACT_ARRAYS] +
                [(n, C.c_int) for n in _MOCAP_SIZES] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _MOCAP_ARRAYS] +
                [(n, C.POINTER(C.c_int) if k == "i" else C.POINTER(C.c_double)) for n, k, _, _ in _PATH_ARRAYS])


_lib = None


def lib() -> C.CDLL:
    """Load libmrs.so (built in-tree by build.py); raises if it is missing."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise MrsError(-3, f"{LIB_PATH} not built; run `python -m mujoco_ros2_simulation_amd.build`")
        L = C.CDLL(str(LIB_PATH))
        L.mrs_last_error.restype = C.c_char_p
        L.mrs_last_status.restype = C.c_int
        L.mrs_model_load_xml.restype = C.c_void_p
        L.mrs_model_load_xml.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.mrs_model_load_xml_string.restype = C.c_void_p
        L.mrs_model_load_xml_string.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        L.mrs_model_free.argtypes = [C.c_void_p]
        L.mrs_model_view_get.argtypes = [C.c_void_p, C.POINTER(ModelView)]
        L.mrs_model_set_restate.argtypes = [C.c_void_p, C.c_int]
        L.mrs_name2id.argtypes = [C.c_void_p, C.c_int, C.c_char_p]
        L.mrs_id2name.restype = C.c_char_p
        L.mrs_id2name.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mrs_actuator_type.argtypes = [C.c_void_p, C.c_int]
        L.mrs_batch_create.restype = C.c_void_p
        L.mrs_batch_create.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mrs_batch_free.argtypes = [C.c_void_p]
        L.mrs_batch_num_envs.argtypes = [C.c_void_p]
        L.mrs_batch_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.mrs_batch_reset.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.mrs_batch_set_start_states.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.mrs_batch_set_start_states_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.mrs_batch_num_start_states.argtypes = [C.c_void_p]
        L.mrs_batch_reset_masked_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.mrs_batch_reset_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.mrs_batch_set_field.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.mrs_batch_get_field.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.mrs_batch_device_ptr.restype = C.c_void_p
        L.mrs_batch_device_ptr.argtypes = [C.c_void_p, C.c_int]
        L.mrs_batch_set_act.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.mrs_batch_get_act.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.mrs_batch_act_device_ptr.restype = C.c_void_p
        L.mrs_batch_act_device_ptr.argtypes = [C.c_void_p]
        L.mrs_batch_set_mocap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.mrs_batch_get_mocap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.mrs_batch_mocap_pos_device_ptr.restype = C.c_void_p
        L.mrs_batch_mocap_pos_device_ptr.argtypes = [C.c_void_p]
        L.mrs_batch_mocap_quat_device_ptr.restype = C.c_void_p
        L.mrs_batch_mocap_quat_device_ptr.argtypes = [C.c_void_p]
        L.mrs_batch_param_dim.argtypes = [C.c_void_p, C.c_int]
        L.mrs_batch_set_param.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.mrs_batch_get_param.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.mrs_batch_param_device_ptr.restype = C.c_void_p
        L.mrs_batch_param_device_ptr.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "mrs_batch_set_inertial"):  # (an A/B library named by MRS_LIB may predate the family)
            L.mrs_model_derive_inertial.argtypes = [C.c_void_p] + [C.c_void_p] * 8
            L.mrs_batch_inertial_dim.argtypes = [C.c_void_p, C.c_int]
            L.mrs_batch_set_inertial.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            L.mrs_batch_get_inertial.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            L.mrs_batch_get_inertial_derived.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mrs_batch_set_ctrl_device.argtypes = [C.c_void_p, C.c_void_p]
        L.mrs_batch_bind_ctrl_device.argtypes = [C.c_void_p, C.c_void_p]
        L.mrs_batch_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.mrs_batch_step.argtypes = [C.c_void_p, C.c_int]
        L.mrs_batch_forward.argtypes = [C.c_void_p]
        L.mrs_batch_render_depth.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.mrs_batch_render_depth_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.mrs_batch_render_rgbd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.mrs_batch_render_rgbd_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.mrs_batch_render_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.mrs_batch_render_wait.argtypes = [C.c_void_p]
        L.mrs_batch_sync.argtypes = [C.c_void_p]
        L.mrs_batch_get_contacts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
        L.mrs_batch_get_efc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
        if hasattr(L, "mrs_batch_get_contact_wrench"):  # (an A/B library named by MRS_LIB may predate them)
            L.mrs_batch_get_contact_forces.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            L.mrs_batch_contact_wrench_device_ptr.restype = C.c_void_p
            L.mrs_batch_contact_wrench_device_ptr.argtypes = [C.c_void_p]
            L.mrs_batch_get_contact_wrench.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        if hasattr(L, "mrs_batch_get_dyn"):  # (likewise)
            L.mrs_batch_set_jac_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            L.mrs_batch_dyn_dim.argtypes = [C.c_void_p, C.c_int]
            L.mrs_batch_dyn_device_ptr.restype = C.c_void_p
            L.mrs_batch_dyn_device_ptr.argtypes = [C.c_void_p, C.c_int]
            L.mrs_batch_get_dyn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        if hasattr(L, "mrs_batch_ray"):  # (likewise)
            L.mrs_batch_ray_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_uint, C.c_int, C.c_void_p, C.c_void_p]
            L.mrs_batch_ray.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            L.mrs_debug_ray_filter.argtypes = [C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.mrs_batch_get_field_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.mrs_batch_last_kernel_ms.restype = C.c_double
        L.mrs_batch_last_kernel_ms.argtypes = [C.c_void_p, C.c_int]
        L.mrs_debug_phase_cycles.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mrs_debug_batch_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.mrs_debug_plan_layout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        if hasattr(L, "mrs_debug_render_plan"):  # (an A/B library named by MRS_LIB may predate it)
            L.mrs_debug_render_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        if hasattr(L, "mrs_debug_pairs"):  # (likewise)
            L.mrs_debug_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        if hasattr(L, "mrs_debug_table_image"):  # (likewise)
            L.mrs_debug_table_image.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            L.mrs_debug_staged_table.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        _lib = L
    return _lib


PHASES = ["kinematics", "com_pos", "make_M", "cholesky", "com_vel", "rne", "smooth_forces", "collision",
          "constraints", "sensors", "integrate", "checks", "sensors.level1", "sensors.setup", "sensors.geoms",
          "constraints.rows", "constraints.records", "constraints.warmstart", "constraints.pgs",
          "collision.narrow", "collision.out", "constraints.delassus", "records.jac", "records.solve",
          "records.rows"]


def phase_cycles(reset: bool = False) -> dict | None:
    """per-phase wave-cycle totals of the step kernel (profiling builds, -DMRS_PHASE_TIMING)"""
    out = np.zeros(len(PHASES))
    n = lib().mrs_debug_phase_cycles(out.ctypes.data_as(C.c_void_p), len(PHASES), int(reset))
    if n <= 0:
        return None
    return dict(zip(PHASES, out[:n].tolist()))


def _check(rc: int) -> None:
    if rc != MRS_OK:
        raise MrsError(rc, lib().mrs_last_error().decode())


class Model:
    """Compiled MJCF model (mjModel analogue).  Arrays are exposed as read-only numpy views."""

    def __init__(self, handle: int):
        self._h = handle
        self.view = ModelView()
        _check(lib().mrs_model_view_get(self._h, C.byref(self.view)))
        v = self.view
        for n in _SIZES + _MESH_SIZES + _CONTACT_SIZES + _EQ_SIZES + _REND_SIZES + _TEN_SIZES + _POLY_SIZES + _MOCAP_SIZES:
            setattr(self, n, getattr(v, n))
        for n in ["timestep", "tolerance", "impratio", "ls_tolerance", "ls_iterations", "restate", "integrator", "solver",
                  "iterations", "disableflags",
                  "stat_extent", "stat_meaninertia", "vis_znear", "vis_zfar"]:
            setattr(self, n, getattr(v, n))
        self.gravity = np.array(v.gravity[:])
        self.vis_headlight = np.array(v.vis_headlight[:])
        for name, kind, count, width in (_ARRAYS + _MESH_ARRAYS + _CONTACT_ARRAYS + _EQ_ARRAYS + _REND_ARRAYS +
                                         _TEN_ARRAYS + _POLY_ARRAYS + _SITE_ARRAYS + _ACT_ARRAYS +
                                         _MOCAP_ARRAYS + _PATH_ARRAYS):
            n = getattr(v, count)
            if isinstance(width, tuple):
                w = getattr(v, width[0]) * width[1]
            else:
                w = getattr(v, width) if isinstance(width, str) else width
            ptr = getattr(v, name)
            size = n * w
            if size == 0 or not ptr:
                arr = np.zeros((n, w) if (w > 1 or not isinstance(width, int)) else (n,),
                               dtype=np.int32 if kind == "i" else np.float64)
            else:
                arr = np.ctypeslib.as_array(ptr, shape=(size,)).copy()
                if w > 1 or not isinstance(width, int):
                    arr = arr.reshape(n, w)
            setattr(self, name, arr)

    @classmethod
    def load(cls, path: str | os.PathLike) -> "Model":
        err = C.create_string_buffer(1024)
        h = lib().mrs_model_load_xml(str(path).encode(), err, 1024)
        if not h:
            raise MrsError(lib().mrs_last_status() or -2, err.value.decode())
        return cls(h)

    @classmethod
    def from_string(cls, xml: str, basedir: str | None = None) -> "Model":
        err = C.create_string_buffer(1024)
        h = lib().mrs_model_load_xml_string(xml.encode(), (basedir or ".").encode(), err, 1024)
        if not h:
            raise MrsError(lib().mrs_last_status() or -2, err.value.decode())
        return cls(h)

    def set_restate(self, flags: int) -> None:
        """opt into this restatement's own solver variants (RESTATE_* bits; 0 = upstream rules);
        batches and oracle data created afterwards use them"""
        _check(lib().mrs_model_set_restate(self._h, int(flags)))
        _check(lib().mrs_model_view_get(self._h, C.byref(self.view)))
        self.restate = self.view.restate

    def derive_inertial(self, body_mass=None, body_inertia=None, dof_armature=None) -> dict:
        """the constants mj_setConst derives at qpos0 from body_mass [nbody], body_inertia [nbody, 3] and
        dof_armature [nv] (None: the model's own), by the compiler's own function: body_subtreemass,
        dof_M0, dof_invweight0, body_invweight0 [nbody, 2] and meaninertia.  No GPU needed"""
        def arg(v, shape):
            if v is None:
                return None
            a = np.ascontiguousarray(v, dtype=np.float64)
            if a.shape != shape:
                raise ValueError(f"expected shape {shape}, got {a.shape}")
            return a
        ins = [arg(body_mass, (self.nbody,)), arg(body_inertia, (self.nbody, 3)), arg(dof_armature, (self.nv,))]
        out = {"body_subtreemass": np.zeros(self.nbody), "dof_M0": np.zeros(self.nv), "dof_invweight0": np.zeros(self.nv),
               "body_invweight0": np.zeros((self.nbody, 2)), "meaninertia": np.zeros(1)}
        _check(lib().mrs_model_derive_inertial(self._h, *(None if a is None else a.ctypes.data for a in ins),
                                               *(o.ctypes.data for o in out.values())))
        out["meaninertia"] = float(out["meaninertia"][0])
        return out

    def name2id(self, objtype: int, name: str) -> int:
        return lib().mrs_name2id(self._h, objtype, name.encode())

    def id2name(self, objtype: int, i: int) -> str | None:
        r = lib().mrs_id2name(self._h, objtype, i)
        return r.decode() if r else None

    def actuator_type(self, i: int) -> int:
        return lib().mrs_actuator_type(self._h, i)

    @property
    def handle(self) -> int:
        return self._h

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mrs_model_free(self._h)
            self._h = None


# floats per env of a field: a fixed count times a model size (None: 1)
_FIELD_DIM = {
    FIELD_QPOS: (1, "nq"), FIELD_QVEL: (1, "nv"), FIELD_CTRL: (1, "nu"), FIELD_QFRC_APPLIED: (1, "nv"),
    FIELD_QACC_WARMSTART: (1, "nv"), FIELD_QACC: (1, "nv"), FIELD_QFRC_ACTUATOR: (1, "nv"),
    FIELD_SENSORDATA: (1, "nsensordata"), FIELD_TIME: (1, None), FIELD_WARNING: (4, None), FIELD_NCON: (1, None),
    FIELD_SOLVER_NITER: (1, None), FIELD_XFRC_APPLIED: (6, "nbody"),
}


# Batch.layout(): the values of mrs_debug_batch_layout, in order (sensors_every_step: 1 under
# MRS_SENSORS_EVERY_STEP=1, else a fused launch evaluates sensors on its last step only)
LAYOUT_KEYS = ["group", "lds_floats", "scratch_floats", "blocked", "pipe_w", "max_efc", "max_con", "ntree",
               "shared_floats", "rf_common", "one_workgroup_per_cu", "waves_per_workgroup", "helper_waves",
               "fused_integrator_factor", "ray_sweep", "sensors_every_step"]
# the values after them: the batch's optional outputs, 1 once asked for (contact_wrench: the net contact
# wrench per body, Batch.contact_wrench)
LAYOUT_OUTPUT_KEYS = ["contact_wrench"]
# and after those: the dynamics outputs that are on, a bit mask (1 << DYNOUT_*)
LAYOUT_DYN_KEYS = ["dyn_outputs"]
# and last: 1 when the 16-lane solves are fused (0 otherwise, and under MRS_NO_SOLVE_FUSE=1)
LAYOUT_SOLVE_KEYS = ["solve_fuse"]
# then the collision pairs the step walks, and the admissible pairs pruned from them (walked_pairs)
LAYOUT_PAIR_KEYS = ["pairs", "pairs_pruned"]
# and: 1 when the launches stage the workgroup-shared tables from one packed image (0 under
# MRS_NO_TABLE_IMAGE=1: table by table)
LAYOUT_IMAGE_KEYS = ["table_image"]


def plan_layout(model: "Model", n_envs: int, cu_count: int, max_contacts: int = 0) -> dict:
    """the LAYOUT_KEYS part of Batch.layout() as a batch of n_envs on a device with cu_count compute
    units (0: unknown) would have it, chosen on the host: needs no GPU"""
    out = np.zeros(len(LAYOUT_KEYS), dtype=np.int32)
    k = lib().mrs_debug_plan_layout(model.handle, n_envs, cu_count, max_contacts, out.ctypes.data, len(out))
    if k < 0:
        raise MrsError(k, lib().mrs_last_error().decode())
    return dict(zip(LAYOUT_KEYS[:k], out[:k].tolist()))


def walked_pairs(model: "Model") -> tuple[np.ndarray, int]:
    """the collision pairs a batch of this model walks each step, [k][2] geom ids in contact order, and
    the number of statically admissible pairs pruned from them because their geoms can never touch
    (mrs_debug_pairs; MRS_NO_PAIR_PRUNE=1 keeps every pair).  Needs no GPU"""
    pruned = C.c_int(0)
    k = lib().mrs_debug_pairs(model.handle, None, 0, C.byref(pruned))
    if k < 0:
        raise MrsError(k, lib().mrs_last_error().decode())
    out = np.zeros((k, 2), dtype=np.int32)
    lib().mrs_debug_pairs(model.handle, out.ctypes.data if k else None, k, None)
    return out, pruned.value


# the tables of the packed image in offset order (table_image), and their ids for staged_table
IMAGE_TABLES = ["rgeom", "rfray", "rf_static", "rfblk", "sensrec", "fricrec", "limrec", "actrec", "dofrec", "bodytab",
                "mpairtab", "jump", "kinbody", "kinjnt", "kingeom"]
STAGED_TABLE_IDS = {name: k for k, name in enumerate(t for t in IMAGE_TABLES if t != "rf_static")}


def table_image(model: "Model", n_envs: int, cu_count: int, max_contacts: int = 0) -> dict:
    """the packed image of the step kernel's workgroup-shared tables as a batch of this plan uploads it
    (mrs_debug_table_image): "image" (fp32, zero-padded to a multiple of 4), "offsets" (table name -> first
    float, in IMAGE_TABLES order, plus "end" and "shared_floats"), "blocked" and "copied" (the floats a
    launch copies).  Needs no GPU"""
    off = np.zeros(18, dtype=np.int32)
    k = lib().mrs_debug_table_image(model.handle, n_envs, cu_count, max_contacts, None, 0, off.ctypes.data, len(off))
    if k < 0:
        raise MrsError(k, lib().mrs_last_error().decode())
    img = np.zeros(k, dtype=np.float32)
    lib().mrs_debug_table_image(model.handle, n_envs, cu_count, max_contacts, img.ctypes.data if k else None, k, None, 0)
    offsets = dict(zip(IMAGE_TABLES + ["end", "shared_floats"], [0] + off[:16].tolist()))
    return {"image": img, "offsets": offsets, "blocked": int(off[16]), "copied": int(off[17])}


def staged_table(model: "Model", name: str, max_contacts: int = 0) -> np.ndarray:
    """one of the tables the image holds, as the model block holds it (mrs_debug_staged_table): fp32; the
    jump table's ints as bits.  Needs no GPU"""
    which = STAGED_TABLE_IDS[name]
    k = lib().mrs_debug_staged_table(model.handle, max_contacts, which, None, 0)
    if k < 0:
        raise MrsError(k, lib().mrs_last_error().decode())
    out = np.zeros(k, dtype=np.float32)
    lib().mrs_debug_staged_table(model.handle, max_contacts, which, out.ctypes.data if k else None, k)
    return out


RENDER_KERNELS = ["binned", "frame", "tile"]  # depth_kernel_mesh, depth_kernel_v2, depth_kernel


def render_plan(model: "Model", cam: int, n_frames: int, max_lds: int) -> dict:
    """how n_frames frames of camera `cam` would be rendered on a device with max_lds bytes of LDS per
    workgroup (mrs_debug_render_plan; the render switches are read at the call): the kernel, the frame
    kernel's mesh flag, the binned kernel's band LDS bytes, frames per launch and list bytes per frame, and
    the grid.  Needs no GPU"""
    out = np.zeros(7, dtype=np.int64)
    k = lib().mrs_debug_render_plan(model.handle, cam, n_frames, max_lds, out.ctypes.data, len(out))
    if k < 0:
        raise MrsError(k, lib().mrs_last_error().decode())
    v = out.tolist()
    return {"kernel": RENDER_KERNELS[v[0]], "mesh": bool(v[1]), "band_lds": v[2], "chunk": v[3], "per_frame": v[4],
            "grid": (v[5], v[6])}


def ray_filter(model: "Model", group_mask: int = 0, include_static: bool = True, bodyexclude: int = -1) -> np.ndarray:
    """the ids of the geoms a ray query with these filters may hit, in geom order (mrs_debug_ray_filter):
    needs no GPU"""
    out = np.zeros(max(1, model.ngeom), dtype=np.int32)
    k = lib().mrs_debug_ray_filter(model.handle, group_mask, 0 if include_static else RAY_NO_STATIC, bodyexclude,
                                   out.ctypes.data, model.ngeom)
    if k < 0:
        raise MrsError(k, lib().mrs_last_error().decode())
    return out[:k].copy()


def _ray_args(frame, shared: bool, include_static: bool) -> tuple[int, int, int]:
    """(flags, frame_type, frame_id) of Batch.ray's keyword arguments"""
    kind, fid = frame
    if kind not in _RAY_FRAMES:
        raise ValueError(f"frame must be one of {sorted(_RAY_FRAMES)}, not {kind!r}")
    return (RAY_SHARED if shared else 0) | (0 if include_static else RAY_NO_STATIC), _RAY_FRAMES[kind], int(fid)


class Batch:
    """N independent environments of one model on one GPU (N x mjData analogue)."""

    def __init__(self, model: Model, n_envs: int, device: int = 0):
        self.model = model
        self.n = n_envs
        h = lib().mrs_batch_create(model.handle, n_envs, device)
        if not h:
            raise MrsError(lib().mrs_last_status() or -3, lib().mrs_last_error().decode())
        self._h = h

    def _dim(self, field: int) -> int:
        k, size = _FIELD_DIM[field]
        return k * getattr(self.model, size) if size else k

    def _get_rows(self, fn, ids: tuple, shapes: list, env0: int, n: int | None, clamp: bool = False) -> list:
        """fn(handle, *ids, one fp64 out [n, *shape] per shape, env0, n); n None: the envs from env0 on"""
        n = self.n - env0 if n is None else n
        outs = [np.empty((max(n, 0) if clamp else n,) + s, dtype=np.float64) for s in shapes]
        _check(fn(self._h, *ids, *(o.ctypes.data for o in outs), env0, n))
        return outs

    def _set_rows(self, fn, ids: tuple, shapes: list, values: list, env0: int) -> None:
        """fn(handle, *ids, one pointer per value as fp64 rows [n, *shape] or None for None, env0, n);
        a shape without elements (e.g. ctrl of a model without actuators) or only None values: no call"""
        if any(0 in s for s in shapes) or all(v is None for v in values):
            return
        rows = [None if v is None else np.ascontiguousarray(v, dtype=np.float64).reshape((-1,) + s)
                for v, s in zip(values, shapes)]
        ns = {r.shape[0] for r in rows if r is not None}
        if len(ns) > 1:  # (two values: the mocap poses)
            raise ValueError("pos and quat cover different numbers of envs")
        _check(fn(self._h, *ids, *(None if r is None else r.ctypes.data for r in rows), env0, ns.pop()))

    def get(self, field: int, env0: int = 0, n: int | None = None) -> np.ndarray:
        out, = self._get_rows(lib().mrs_batch_get_field, (field,), [(self._dim(field),)], env0, n)
        if field == FIELD_XFRC_APPLIED:  # per body: world-frame force, then torque
            return out.reshape(out.shape[0], self.model.nbody, 6)
        return out

    def set(self, field: int, values, env0: int = 0) -> None:
        self._set_rows(lib().mrs_batch_set_field, (field,), [(self._dim(field),)], [values], env0)

    def get_act(self, env0: int = 0, n: int | None = None) -> np.ndarray:
        """mjData.act [n, na]: the activations of the stateful actuators, by actuator_actadr"""
        return self._get_rows(lib().mrs_batch_get_act, (), [(self.model.na,)], env0, n)[0]

    def set_act(self, values, env0: int = 0) -> None:
        self._set_rows(lib().mrs_batch_set_act, (), [(self.model.na,)], [values], env0)

    def act_device_ptr(self) -> int:
        """the activations on the device, fp32 [n, na], ordered on the batch stream (0 when na == 0)"""
        return lib().mrs_batch_act_device_ptr(self._h) or 0

    def get_mocap(self, env0: int = 0, n: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """mjData.mocap_pos [n, nmocap, 3] and mocap_quat [n, nmocap, 4] as the caller wrote them (the
        kernel normalises the quaternion it reads); rows by body_mocapid"""
        nm = self.model.nmocap
        return tuple(self._get_rows(lib().mrs_batch_get_mocap, (), [(nm, 3), (nm, 4)], env0, n))

    def set_mocap(self, pos=None, quat=None, env0: int = 0) -> None:
        """write the mocap poses of envs [env0, env0 + n); a part given as None is left as it is"""
        nm = self.model.nmocap
        self._set_rows(lib().mrs_batch_set_mocap, (), [(nm, 3), (nm, 4)], [pos, quat], env0)

    def mocap_pos_device_ptr(self) -> int:
        """mocap_pos on the device, fp32 [n, nmocap, 3], ordered on the batch stream (0 when nmocap == 0)"""
        return lib().mrs_batch_mocap_pos_device_ptr(self._h) or 0

    def mocap_quat_device_ptr(self) -> int:
        """mocap_quat on the device, fp32 [n, nmocap, 4] (0 when nmocap == 0)"""
        return lib().mrs_batch_mocap_quat_device_ptr(self._h) or 0

    def _param_shape(self, param: int) -> tuple:
        dim = lib().mrs_batch_param_dim(self._h, param)
        if dim < 0:
            raise MrsError(dim, lib().mrs_last_error().decode())
        return (dim // 3, 3) if param in (PARAM_ACT_GAINPRM, PARAM_ACT_BIASPRM) else (dim,)

    def get_model_param(self, param: int, env0: int = 0, n: int | None = None) -> np.ndarray:
        """per-env model parameter PARAM_*: actuator gainprm / biasprm [0:3] as [n, nu, 3], dof damping
        [n, nv], geom sliding friction [n, ngeom]; the model's own values until the parameter is set"""
        # (clamp: a negative n is the library's to reject)
        return self._get_rows(lib().mrs_batch_get_param, (param,), [self._param_shape(param)], env0, n, clamp=True)[0]

    def set_model_param(self, param: int, values, env0: int = 0) -> None:
        """write a model parameter of envs [env0, env0 + n); one row of values broadcasts over the envs
        from env0 on.  Takes effect at the next step / forward launch; resets keep it"""
        shape = self._param_shape(param)
        a = np.asarray(values, dtype=np.float64)
        if a.ndim == len(shape):
            a = np.broadcast_to(a, (self.n - env0,) + shape)
        if a.size == 0:
            return
        self._set_rows(lib().mrs_batch_set_param, (param,), [shape], [a], env0)

    def model_param_device_ptr(self, param: int) -> int:
        """the parameter's buffer on the device, fp32 [n_envs, dim], ordered on the batch stream (made on
        first use; 0 when the model has none of it)"""
        return lib().mrs_batch_param_device_ptr(self._h, param) or 0

    def _inertial_shapes(self) -> list:
        return [(self.model.nbody,), (self.model.nbody, 3), (self.model.nv,)]

    def get_inertial(self, env0: int = 0, n: int | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """per-env body_mass [n, nbody], body_inertia [n, nbody, 3] and dof_armature [n, nv]; the model's own
        values until set_inertial"""
        return tuple(self._get_rows(lib().mrs_batch_get_inertial, (), self._inertial_shapes(), env0, n, clamp=True))

    def set_inertial(self, mass=None, inertia=None, armature=None, env0: int = 0) -> None:
        """write body mass / principal inertia / dof armature of envs [env0, env0 + n), as "set the mjModel
        arrays, then mj_setConst": the envs' derived constants are re-derived on the host.  A quantity given
        as None is left as it is; one row broadcasts over the envs from env0 on.  Resets keep the values"""
        rows = []
        for v, shape in zip([mass, inertia, armature], self._inertial_shapes()):
            if v is None:
                rows.append(None)
                continue
            a = np.asarray(v, dtype=np.float64)
            if a.ndim == len(shape):
                a = np.broadcast_to(a, (self.n - env0,) + shape)
            rows.append(np.ascontiguousarray(a).reshape((-1,) + shape))
        ns = {r.shape[0] for r in rows if r is not None}
        if not ns:
            return
        if len(ns) > 1:
            raise ValueError("mass, inertia and armature cover different numbers of envs")
        _check(lib().mrs_batch_set_inertial(self._h, *(None if r is None else r.ctypes.data for r in rows), env0, ns.pop()))

    def inertial_derived(self, env: int) -> dict:
        """what the kernels read for env `env` (fp32 on the device, widened): body_subtreemass,
        dof_invweight0, body_invweight0 [nbody, 2] and meaninertia"""
        m = self.model
        out = {"body_subtreemass": np.zeros(m.nbody), "dof_invweight0": np.zeros(m.nv),
               "body_invweight0": np.zeros((m.nbody, 2)), "meaninertia": np.zeros(1)}
        _check(lib().mrs_batch_get_inertial_derived(self._h, env, *(o.ctypes.data for o in out.values())))
        out["meaninertia"] = float(out["meaninertia"][0])
        return out

    def reset(self, key: int = -1, env0: int = 0, n: int | None = None) -> None:
        _check(lib().mrs_batch_reset(self._h, key, env0, self.n - env0 if n is None else n))

    def set_start_states(self, qpos, qvel=None) -> None:
        """replace the pool of start states reset_where addresses as nkey + row: qpos [count, nq] and
        qvel [count, nv] (None: zeros), copied as given; an empty qpos frees the pool"""
        m = self.model
        q = np.ascontiguousarray(qpos, dtype=np.float64)
        count = 0 if q.size == 0 else q.reshape(-1, m.nq).shape[0]
        v = None
        if qvel is not None and count:
            v = np.ascontiguousarray(qvel, dtype=np.float64)
            if v.size != count * m.nv:
                raise ValueError(f"qvel must have shape ({count}, {m.nv})")
        _check(lib().mrs_batch_set_start_states(self._h, q.ctypes.data if count else None,
                                                 v.ctypes.data if v is not None and v.size else None, count))

    def set_start_states_device(self, qpos_ptr: int, qvel_ptr: int | None, count: int) -> None:
        """the same from device fp32 buffers [count, nq] / [count, nv] (qvel_ptr 0 or None: zeros),
        copied device-to-device, asynchronous on the batch stream"""
        _check(lib().mrs_batch_set_start_states_device(self._h, C.c_void_p(qpos_ptr) if qpos_ptr else None,
                                                        C.c_void_p(qvel_ptr) if qvel_ptr else None, count))

    @property
    def num_start_states(self) -> int:
        return lib().mrs_batch_num_start_states(self._h)

    def reset_where(self, mask, keys=None, key: int = -1) -> None:
        """reset the envs with mask[e] set (bool or uint8 [n]), each to the start index keys[e]
        (int32 [n]) or, without keys, to `key`: -1 qpos0, 0 .. nkey-1 a keyframe, nkey + r pool row r.
        Unmasked envs are not written and a bound ctrl buffer stays bound (mrs_batch_reset_masked)"""
        mask = np.asarray(mask)
        if mask.shape != (self.n,):
            raise ValueError(f"mask must have shape ({self.n},), not {mask.shape}")
        if mask.dtype not in (np.bool_, np.uint8):
            raise ValueError(f"mask must be bool or uint8, not {mask.dtype}")
        mask = np.ascontiguousarray(mask).view(np.uint8)
        if keys is not None:
            keys = np.asarray(keys)
            if keys.shape != (self.n,):
                raise ValueError(f"keys must have shape ({self.n},), not {keys.shape}")
            if keys.dtype != np.int32:
                raise ValueError(f"keys must be int32, not {keys.dtype}")
            keys = np.ascontiguousarray(keys)
        _check(lib().mrs_batch_reset_masked(self._h, mask.ctypes.data, keys.ctypes.data if keys is not None else None,
                                             key))

    def reset_where_device(self, mask_ptr: int, keys_ptr: int = 0, key: int = -1) -> None:
        """the same from device buffers (a torch.bool / uint8 mask and an int32 key tensor's data_ptr()):
        one launch on the batch stream, no host synchronisation"""
        _check(lib().mrs_batch_reset_masked_device(self._h, C.c_void_p(mask_ptr) if mask_ptr else None,
                                                    C.c_void_p(keys_ptr) if keys_ptr else None, key))

    def layout(self) -> dict:
        """kernel configuration of this batch (diagnostics): group width, LDS and scratch floats per
        env, blocked mode, pipe width, row and contact capacity, kinematic trees"""
        keys = (LAYOUT_KEYS + LAYOUT_OUTPUT_KEYS + LAYOUT_DYN_KEYS + LAYOUT_SOLVE_KEYS + LAYOUT_PAIR_KEYS +
                LAYOUT_IMAGE_KEYS)
        out = np.zeros(len(keys), dtype=np.int32)
        k = lib().mrs_debug_batch_layout(self._h, out.ctypes.data, len(keys))
        return dict(zip(keys[:k], out[:k].tolist()))

    def step(self, n_steps: int = 1) -> None:
        _check(lib().mrs_batch_step(self._h, n_steps))

    def forward(self) -> None:
        _check(lib().mrs_batch_forward(self._h))

    def sync(self) -> None:
        _check(lib().mrs_batch_sync(self._h))

    def device_ptr(self, field: int) -> int:
        return lib().mrs_batch_device_ptr(self._h, field)

    def set_ctrl_device(self, ptr: int) -> None:
        _check(lib().mrs_batch_set_ctrl_device(self._h, C.c_void_p(ptr)))

    def bind_ctrl_device(self, ptr: int | None) -> None:
        """zero-copy ctrl: the following launches read ctrl from this device buffer [n][nu] fp32
        (None: the batch's own buffer again; set / set_ctrl_device also return to it)"""
        _check(lib().mrs_batch_bind_ctrl_device(self._h, C.c_void_p(ptr) if ptr else None))

    def set_stream(self, stream_ptr: int | None) -> None:
        _check(lib().mrs_batch_set_stream(self._h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def render_depth(self, cam: int, env0: int = 0, n: int = 1) -> np.ndarray:
        W, H = self.model.cam_resolution[cam]
        out = np.empty((n, H, W), dtype=np.float32)
        _check(lib().mrs_batch_render_depth(self._h, cam, env0, n, out.ctypes.data))
        return out

    def render_rgbd(self, cam: int, env0: int = 0, n: int = 1) -> tuple[np.ndarray, np.ndarray]:
        """(depth [n, H, W] fp32, rgb [n, H, W, 3] uint8) in one pass"""
        W, H = self.model.cam_resolution[cam]
        depth = np.empty((n, H, W), dtype=np.float32)
        rgb = np.empty((n, H, W, 3), dtype=np.uint8)
        _check(lib().mrs_batch_render_rgbd(self._h, cam, env0, n, depth.ctypes.data, rgb.ctypes.data))
        return depth, rgb

    def render_rgbd_device(self, cam: int, env0: int, n: int, depth_ptr: int, rgb_ptr: int) -> None:
        _check(lib().mrs_batch_render_rgbd_device(self._h, cam, env0, n, C.c_void_p(depth_ptr), C.c_void_p(rgb_ptr)))

    def render_depth_device(self, cam: int, env0: int, n: int, dptr: int) -> None:
        _check(lib().mrs_batch_render_depth_device(self._h, cam, env0, n, C.c_void_p(dptr)))

    def render_async(self, cam: int, env0: int, n: int, depth_ptr: int, rgb_ptr: int = 0) -> None:
        """snapshot the last step's poses, render from the snapshot concurrently with later steps"""
        _check(lib().mrs_batch_render_async(self._h, cam, env0, n, C.c_void_p(depth_ptr),
                                             C.c_void_p(rgb_ptr) if rgb_ptr else None))

    def render_wait(self) -> None:
        """order the batch stream after the last asynchronous render"""
        _check(lib().mrs_batch_render_wait(self._h))

    def ray(self, pnt, vec, *, shared: bool | None = None, frame=("world", 0), group_mask: int = 0,
            include_static: bool = True, bodyexclude: int = -1, env0: int = 0, n: int | None = None,
            want_geomid: bool = True) -> tuple[np.ndarray, np.ndarray | None]:
        """mj_ray for every ray of envs [env0, env0 + n): pnt / vec [n, n_rays, 3], or one pattern
        [n_rays, 3] for every env (shared; the default when pnt has two dimensions), in the world's frame or
        in frame ("geom" | "camera", id): each env's own pose of it.  Returns (dist [n, n_rays] in units of
        |vec|, -1 on a miss; geomid [n, n_rays] int32, -1 on a miss, or None without want_geomid).  The
        poses are those of the last step / forward: after step() the state before the last step's
        integration; call forward() first for the current qpos.  group_mask bit g keeps group g (0: every
        group), include_static=False drops the geoms of bodies welded to the world, bodyexclude one body's"""
        p = np.ascontiguousarray(pnt, dtype=np.float64)
        v = np.ascontiguousarray(vec, dtype=np.float64)
        if shared is None:
            shared = p.ndim == 2
        n = self.n - env0 if n is None else n
        ok = p.shape == v.shape and p.shape[-1:] == (3,) and (p.ndim == 2 if shared else p.ndim == 3 and p.shape[0] == n)
        if not ok:
            raise ValueError(f"pnt {p.shape} and vec {v.shape} must both be "
                             f"{'[n_rays, 3]' if shared else f'[{n}, n_rays, 3]'}")
        n_rays = p.shape[-2]
        flags, ftype, fid = _ray_args(frame, shared, include_static)
        dist = np.empty((max(n, 0), n_rays), dtype=np.float64)
        gid = np.empty((max(n, 0), n_rays), dtype=np.int32) if want_geomid else None
        _check(lib().mrs_batch_ray(self._h, p.ctypes.data, v.ctypes.data, n_rays, flags, ftype, fid, group_mask,
                                   bodyexclude, dist.ctypes.data, gid.ctypes.data if want_geomid else None, env0, n))
        return dist, gid

    def ray_device(self, pnt_ptr: int, vec_ptr: int, n_rays: int, dist_ptr: int, geomid_ptr: int = 0, *,
                   shared: bool = False, frame=("world", 0), group_mask: int = 0, include_static: bool = True,
                   bodyexclude: int = -1) -> None:
        """the same for every env from device fp32 rays [n_envs, n_rays, 3] (shared: [n_rays, 3]) into device
        buffers dist fp32 and geomid int32 [n_envs, n_rays] (geomid_ptr 0: not wanted) -- torch tensors'
        data_ptr(); one launch on the batch stream, no host synchronisation"""
        flags, ftype, fid = _ray_args(frame, shared, include_static)
        _check(lib().mrs_batch_ray_device(self._h, C.c_void_p(pnt_ptr) if pnt_ptr else None,
                                          C.c_void_p(vec_ptr) if vec_ptr else None, n_rays, flags, ftype, fid,
                                          group_mask, bodyexclude, C.c_void_p(dist_ptr) if dist_ptr else None,
                                          C.c_void_p(geomid_ptr) if geomid_ptr else None))

    def contacts(self, env: int = 0, max_n: int = 256):
        """mjData.contact of `env` after the last step/forward: (geom [n, 2] int32, dist [n],
        pos [n, 3], frame [n, 9]) in mj_collision's order"""
        g = np.zeros((max_n, 2), dtype=np.int32)
        dist, pos, frame = np.zeros(max_n), np.zeros((max_n, 3)), np.zeros((max_n, 9))
        n = lib().mrs_batch_get_contacts(self._h, env, max_n, g.ctypes.data, dist.ctypes.data, pos.ctypes.data,
                                         frame.ctypes.data)
        if n < 0:
            _check(n)
        n = min(n, max_n)
        return g[:n], dist[:n], pos[:n], frame[:n]

    def efc(self, env: int = 0, max_n: int = 1024):
        """mjData.efc_* of `env` after the last step/forward: dict of type [n] (1 friction loss,
        2 limit, 3 contact), J [n, nv], R, aref, force [n]"""
        nv = self.model.nv
        t = np.zeros(max_n, dtype=np.int32)
        J = np.zeros((max_n, max(nv, 1)))
        R, a, f = np.zeros(max_n), np.zeros(max_n), np.zeros(max_n)
        n = lib().mrs_batch_get_efc(self._h, env, max_n, t.ctypes.data, J.ctypes.data, R.ctypes.data, a.ctypes.data,
                                    f.ctypes.data)
        if n < 0:
            _check(n)
        n = min(n, max_n)
        return {"type": t[:n], "J": J[:n, :nv], "R": R[:n], "aref": a[:n], "force": f[:n]}

    def contact_forces(self, env: int = 0, max_n: int = 256) -> np.ndarray:
        """mj_contactForce of every contact of `contacts(env)`, in its order: [ncon, 6] in the contact
        frame (normal, tangent 1, tangent 2, then three zeros); a contact without rows gives zeros"""
        f = np.zeros((max_n, 6))
        n = lib().mrs_batch_get_contact_forces(self._h, env, max_n, f.ctypes.data)
        if n < 0:
            _check(n)
        return f[:min(n, max_n)]

    def contact_wrench(self, env0: int = 0, n: int | None = None) -> np.ndarray:
        """the net contact wrench per body [n, nbody, 6] of the last launch: world-frame force, then
        torque about the body's centre of mass (xfrc_applied's layout; row 0: on the world's geoms, about
        the origin).  The first call (or contact_wrench_device_ptr) turns the output on: zeros until a
        step or forward has been launched after it"""
        return self._get_rows(lib().mrs_batch_get_contact_wrench, (), [(self.model.nbody, 6)], env0, n)[0]

    def contact_wrench_device_ptr(self) -> int:
        """the net contact wrenches on the device, fp32 [n_envs, nbody, 6], ordered on the batch stream;
        turns the output on for all later launches"""
        p = lib().mrs_batch_contact_wrench_device_ptr(self._h)
        if not p:
            raise MrsError(lib().mrs_last_status() or -3, lib().mrs_last_error().decode())
        return p

    def set_jac_sites(self, sites) -> None:
        """the sites (ids or names, at most MAX_JAC_SITES, no duplicates) that DYNOUT_SITE_JAC and
        DYNOUT_SITE_POSE cover, in this order; changing the selection remakes their buffers zero-filled"""
        ids = [self.model.name2id(OBJ_SITE, s) if isinstance(s, str) else int(s) for s in sites]
        arr = np.asarray(ids, dtype=np.int32)
        _check(lib().mrs_batch_set_jac_sites(self._h, arr.ctypes.data if len(ids) else None, len(ids)))

    def dyn_dim(self, which: int) -> int:
        """floats per env of dynamics output `which`"""
        d = lib().mrs_batch_dyn_dim(self._h, which)
        if d < 0:
            _check(d)
        return d

    def dyn(self, which: int, env0: int = 0, n: int | None = None) -> np.ndarray:
        """dynamics output `which` (DYNOUT_*) of the last launch: qfrc_bias [n, nv], the dense mass matrix
        [n, nv, nv], the selected sites' Jacobians [n, nsel, 6, nv] (jacp rows, then jacr, world frame) or
        poses [n, nsel, 12] (site_xpos, then site_xmat row-major).  They belong to the forward pass that
        wrote sensordata: after step() the state before the last step's integration, after forward() the
        current one.  The first call (or dyn_device_ptr) turns the output on: zeros until a step or
        forward has been launched after it"""
        nv = self.model.nv
        dim = self.dyn_dim(which)
        shape = {DYNOUT_QFRC_BIAS: (nv,), DYNOUT_MASS_MATRIX: (nv, nv),
                 DYNOUT_SITE_JAC: (dim // max(1, 6 * nv), 6, nv), DYNOUT_SITE_POSE: (dim // 12, 12)}[which]
        return self._get_rows(lib().mrs_batch_get_dyn, (which,), [shape], env0, n)[0]

    def dyn_device_ptr(self, which: int) -> int | None:
        """dynamics output `which` on the device, fp32 [n_envs, dim], ordered on the batch stream; turns
        the output on for all later launches.  None for a site output while no site is selected"""
        p = lib().mrs_batch_dyn_device_ptr(self._h, which)
        if not p and lib().mrs_last_status() != MRS_OK:
            raise MrsError(lib().mrs_last_status(), lib().mrs_last_error().decode())
        return p

    def get_device(self, field: int, dptr: int, env0: int = 0, n: int | None = None) -> None:
        """fp32 rows of `field` into a device buffer [n, dim], asynchronous on the batch stream"""
        n = self.n - env0 if n is None else n
        _check(lib().mrs_batch_get_field_device(self._h, field, C.c_void_p(dptr), env0, n))

    def set_timing(self, mask: int) -> None:
        """launches bracketed by the batch's own HIP events (bit 0 step, bit 1 frames; default 2)"""
        _check(lib().mrs_batch_set_timing(self._h, mask))

    def last_kernel_ms(self, kind: int = 0) -> float:
        return lib().mrs_batch_last_kernel_ms(self._h, kind)

    def close(self) -> None:
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mrs_batch_free(self._h)
            self._h = None

    def __del__(self):
        self.close()
