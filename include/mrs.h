/*
 * mrs.h — C ABI of the MI355X batched rigid-body simulator (library libmrs.so).
 *
 * This is the boundary the re-implemented `mujoco_ros2_control/MujocoSystemInterface` plugin calls
 * instead of MuJoCo.  Every entry point names the reference call site it replaces (paths relative
 * to the reference repository).  Conventions: opaque handles, int status codes
 * (MRS_OK = 0, negative = error, message via mrs_last_error()), no exceptions across the ABI,
 * caller-owned host buffers in fp64 (mjtNum), one batch handle used by one thread at a time (the
 * plugin serialises with its own mutex, as the reference serialises with sim_mutex_).
 * Environment e of a batch is an independent mjData; the plugin maps ROS-visible state to env 0.
 * Device state is fp32, structure-of-arrays per field, env-major inside a field
 * (qpos[e * nq + i]); host get/set convert.
 */
#ifndef MRS_H
#define MRS_H

#include "mrs_model.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mrs_model mrs_model; /* compiled model (mjModel analogue) */
typedef struct mrs_batch mrs_batch; /* N environments resident on one GPU (N x mjData analogue) */

enum {
  MRS_OK = 0,
  MRS_ERR_INVALID = -1,     /* bad argument / handle / range */
  MRS_ERR_LOAD = -2,        /* model could not be parsed or compiled */
  MRS_ERR_DEVICE = -3,      /* HIP runtime error or no usable GPU */
  MRS_ERR_UNSUPPORTED = -4  /* feature outside the implemented subset */
};

/* batch state fields addressable through mrs_batch_device_ptr / get / set */
enum {
  MRS_FIELD_QPOS = 0,          /* nq,  fp32 */
  MRS_FIELD_QVEL = 1,          /* nv,  fp32 */
  MRS_FIELD_CTRL = 2,          /* nu,  fp32 */
  MRS_FIELD_QFRC_APPLIED = 3,  /* nv,  fp32 */
  MRS_FIELD_QACC_WARMSTART = 4,/* nv,  fp32 */
  MRS_FIELD_QACC = 5,          /* nv,  fp32 (output) */
  MRS_FIELD_QFRC_ACTUATOR = 6, /* nv,  fp32 (output) */
  MRS_FIELD_SENSORDATA = 7,    /* nsensordata, fp32 (output) */
  MRS_FIELD_TIME = 8,          /* 1,   fp64 */
  MRS_FIELD_WARNING = 9,       /* 4,   int32: counts of bad qpos, bad qvel, bad qacc (auto-resets), and of
                                  helper-wave signal timeouts (an internal protocol fault: the step then
                                  built its rows inline; 0 in every correct run) */
  MRS_FIELD_NCON = 10,         /* 1,   int32: contacts found in the last step (output) */
  MRS_FIELD_SOLVER_NITER = 11, /* 1,   int32: constraint solver iterations of the last step (mjData.solver_niter) */
  MRS_FIELD_XFRC_APPLIED = 12, /* 6 * nbody, fp32: mjData.xfrc_applied, per body a world-frame force [0:3] then
                                  torque [3:6] acting at the body's centre of mass (xipos); row 0 (the
                                  world) is ignored.  Added to qfrc_smooth beside qfrc_applied and counted
                                  as external by the force / torque sensors (mj_rnePostConstraint).  Its
                                  buffer is made, zero-filled, on the first set / get_field_device /
                                  device_ptr of the field; reading it before returns zeros */
  MRS_FIELD_COUNT = 13
};

/* last error message of the calling thread ("" if none) */
const char* mrs_last_error(void);
/* status code (MRS_OK or MRS_ERR_*) of the calling thread's last call, for the entry points that
 * return a handle (NULL on failure) rather than a code */
int mrs_last_status(void);

/* ------------------------------------------------------------------ model
 * replaces mj_loadXML (src/mujoco_system_interface.cpp:318).  The reference's other branch, a path
 * ending in ".mjb" loaded by mj_loadModel (:307-310), is not supported: such a path fails with
 * MRS_ERR_UNSUPPORTED (mrs_last_status) and "could not load binary model ..." in `error` */
mrs_model* mrs_model_load_xml(const char* path, char* error, int error_len);
/* replaces mj_parseXMLString + mj_compile (src/mujoco_system_interface.cpp:398-399, model from the
 * /mujoco_robot_description topic); `basedir` resolves <include> (may be NULL) */
mrs_model* mrs_model_load_xml_string(const char* xml, const char* basedir, char* error,
                                     int error_len);
/* replaces mj_deleteModel (src/mujoco_system_interface.cpp:512) */
void mrs_model_free(mrs_model* m);
/* deep copy of a compiled model (mj_copyModel behind get_model, src/mujoco_system_interface.cpp:
 * 1794-1798); NULL on a null argument */
mrs_model* mrs_model_copy(const mrs_model* m);
/* read-only view of the compiled arrays (mjModel field access throughout the plugin, e.g.
 * jnt_qposadr at src/mujoco_system_interface.cpp:1224); valid while `m` lives */
int mrs_model_view_get(const mrs_model* m, mrs_model_view* out);
/* opt into this restatement's own solver variants (MRS_RESTATE_* bits of mrs_model.h; 0, the
 * default, follows the upstream rules); batches created afterwards use them */
int mrs_model_set_restate(mrs_model* m, int flags);
/* the constants mj_setConst derives from mass / inertia / armature at qpos0; any input NULL = the
 * model's own; any output NULL = not wanted.  body_mass [nbody], body_inertia [nbody][3] (principal
 * moments in the body's compiled body_iquat frame), dof_armature [nv]; outputs body_subtreemass [nbody],
 * dof_M0 [nv], dof_invweight0 [nv], body_invweight0 [nbody][2], meaninertia [1].  The function the MJCF
 * compiler itself calls, so the model's own inputs return the model's own constants.  No GPU needed.
 * MRS_ERR_INVALID for a non-finite or negative input or when M(qpos0) is not positive definite;
 * MRS_ERR_UNSUPPORTED for a model with tendons (tendon_invweight0 is not re-derived yet). */
int mrs_model_derive_inertial(const mrs_model* m, const double* body_mass, const double* body_inertia,
                              const double* dof_armature, double* body_subtreemass, double* dof_M0,
                              double* dof_invweight0, double* body_invweight0, double* meaninertia);
/* replaces mj_name2id (src/mujoco_system_interface.cpp:1193,1213,1496-1497,1527-1529);
 * objtype is MRS_OBJ_*; returns -1 if not found */
int mrs_name2id(const mrs_model* m, int objtype, const char* name);
/* replaces mj_id2name (src/mujoco_lidar.cpp:139); NULL if unnamed or out of range */
const char* mrs_id2name(const mrs_model* m, int objtype, int id);
/* replaces getActuatorType (src/mujoco_system_interface.cpp:433-460):
 * 1 MOTOR, 2 POSITION, 3 VELOCITY, 4 CUSTOM, 0 UNKNOWN (same numbering as ActuatorType) */
int mrs_actuator_type(const mrs_model* m, int actuator_id);

/* ------------------------------------------------------------------ batch
 * replaces mj_makeData (src/mujoco_system_interface.cpp:686-687) for n_envs environments on HIP
 * device `device`; all envs start at qpos0 (mj_resetData) */
mrs_batch* mrs_batch_create(const mrs_model* m, int n_envs, int device);
/* replaces mj_deleteData (src/mujoco_system_interface.cpp:504-509) */
void mrs_batch_free(mrs_batch* b);
int mrs_batch_num_envs(const mrs_batch* b);
/* use an external HIP stream (hipStream_t) for all batch work; NULL = the batch's own stream */
int mrs_batch_set_stream(mrs_batch* b, void* hip_stream);
/* mj_resetData / mj_resetDataKeyframe for envs [env0, env0+n): key < 0 resets to qpos0 */
int mrs_batch_reset(mrs_batch* b, int key, int env0, int n);

/* ---- device-side masked reset (no reference counterpart: the reference resets one mjData on the
 * host, mj_resetData / mj_resetDataKeyframe; here episodes end in scattered envs of a batch whose
 * training loop stays on the GPU).
 *
 * A start index k addresses a start state: -1 is qpos0 (zero qvel and ctrl, time 0), 0 .. nkey-1 the
 * model's keyframe k, nkey .. nkey+P-1 row k - nkey of the batch's pool of P runtime start states.
 * The model's keyframes and qpos0 are uploaded to a device table at batch creation and the pool lives
 * in HBM as fp32 in the state fields' layout, so the reset kernel reads everything from device memory.
 *
 * replace the batch's pool of start states: `count` rows, host fp64 qpos [count][nq] and
 * qvel [count][nv] (qvel may be NULL: zeros).  count == 0 frees the pool.  Rows are copied as given,
 * as mj_resetDataKeyframe copies a keyframe (quaternions are not renormalised); a pool row has
 * ctrl = 0 and time = 0.  Returns when the host rows have been read. */
int mrs_batch_set_start_states(mrs_batch* b, const double* qpos, const double* qvel, int count);
/* same from device fp32 buffers, copied device-to-device, asynchronous on the batch stream (the
 * buffers may be reused once that copy has run).  Only a pool that grows past the largest count it has
 * held, or is freed, waits for the queued work that may still read the old rows */
int mrs_batch_set_start_states_device(mrs_batch* b, const float* d_qpos, const float* d_qvel, int count);
/* rows in the pool (P above) */
int mrs_batch_num_start_states(const mrs_batch* b);
/* reset the envs e with d_mask[e] != 0 (uint8 [n_envs], a torch.bool tensor's storage), each to
 * the start index d_key[e] (int32 [n_envs]) or, with d_key == NULL, to `key`.  One launch,
 * asynchronous on the batch stream, no host synchronisation: stream order alone places it after the
 * steps and pool copies queued before and ahead of the steps queued after.  A masked env gets what
 * mrs_batch_reset writes: qpos, qvel, ctrl and time of its start state, qfrc_applied,
 * qacc_warmstart and the four warning counters zeroed, and its xfrc_applied rows zeroed if that
 * buffer exists (it is not made here); the output fields keep their values.  An unmasked env is not
 * written at all.  Unlike mrs_batch_reset this call keeps a ctrl buffer bound by
 * mrs_batch_bind_ctrl_device: while one is bound neither that buffer (the caller's) nor the batch's
 * own ctrl is written, and the launches go on reading the bound buffer -- the call to prefer in a bound
 * loop.  The scalar `key` is checked here (>= nkey + P: MRS_ERR_INVALID); a per-env index cannot be
 * checked without a synchronisation, so an index outside [-1, nkey + P) resets that env to qpos0 (as -1).
 * The mask and the key array are only read. */
int mrs_batch_reset_masked_device(mrs_batch* b, const unsigned char* d_mask, const int* d_key, int key);
/* same with host arrays [n_envs] (staged to the device on the batch stream; returns when they have
 * been read, without waiting for the reset itself); `keys` may be NULL */
int mrs_batch_reset_masked(mrs_batch* b, const unsigned char* mask, const int* keys, int key);

/* host <-> device state copies for envs [env0, env0+n), host layout [n][dim] fp64.
 * set_* replace the control->sim copies mju_copy(ctrl/qfrc_applied) at
 * src/mujoco_system_interface.cpp:1688-1689,1728-1729 and set_initial_pose/keyframe writes
 * (:1611-1614,1617-1626); get_* replace the reads of mj_data_control_ in read()
 * (:1057-1098) and of sensordata in MujocoLidar::update (src/mujoco_lidar.cpp:247-250). */
int mrs_batch_set_field(mrs_batch* b, int field, const double* host, int env0, int n);
int mrs_batch_get_field(mrs_batch* b, int field, double* host, int env0, int n);
/* device pointer of a field (for zero-copy use from torch / RCCL); layout [n_envs][dim] */
void* mrs_batch_device_ptr(mrs_batch* b, int field);
/* copy ctrl for all envs from a device buffer [n_envs][nu] fp32 (device-resident actions) */
int mrs_batch_set_ctrl_device(mrs_batch* b, const float* d_ctrl);
/* zero-copy form of the same write (a policy's output tensor as the sim's ctrl): the following step
 * and forward launches read ctrl from the caller's device buffer [n_envs][nu] fp32, stream-ordered
 * on the batch stream, until another buffer is bound, NULL is bound, or ctrl is set by
 * mrs_batch_set_field / mrs_batch_set_ctrl_device (which return to the batch's own buffer).  Reads
 * of the ctrl field return the bound buffer's values.  The buffer must stay valid while bound. */
int mrs_batch_bind_ctrl_device(mrs_batch* b, const float* d_ctrl);
/* xfrc_applied has no bind call: its own buffer is the one the kernel reads.  A write to
 * mrs_batch_device_ptr(b, MRS_FIELD_XFRC_APPLIED) [n_envs][nbody][6] fp32 that is ordered on the batch
 * stream takes effect at the next step / forward launch; like ctrl / qfrc_applied the wrenches are held
 * over the n steps of a launch (and RK4's stages), mrs_batch_reset zeroes the reset envs' rows, and the
 * NaN auto-reset keeps them. */
/* mjData.act: the activations of the model's na stateful actuators (dyntype integrator, filter or
 * filterexact; mrs_model_view actuator_actadr gives each one's column).  Integrated state like qpos
 * and qvel: a step launch loads it, advances it every step and stores it back; every reset writes it
 * (a keyframe's key_act, else 0) and the NaN auto-reset zeroes it.  Not an MRS_FIELD_* value: host
 * layout [n][na] fp64 for envs [env0, env0+n); with na == 0 set / get succeed and copy nothing. */
int mrs_batch_set_act(mrs_batch* b, const double* host, int env0, int n);
int mrs_batch_get_act(mrs_batch* b, double* host, int env0, int n);
/* device pointer of the activations, [n_envs][na] fp32; accesses ordered on the batch stream see the
 * launches' values.  NULL when na == 0. */
float* mrs_batch_act_device_ptr(mrs_batch* b);
/* mjData.mocap_pos / mocap_quat: the world poses of the model's nmocap mocap bodies (mrs_model_view
 * body_mocapid gives each one's row).  Input state like ctrl: a launch reads them at its start and
 * holds them over its n steps (and RK4's stages); the buffer keeps what the caller wrote and the
 * kinematics normalise the quaternion they read.  They start at the bodies' pos / quat; every reset
 * writes the reset envs' rows (a keyframe's mpos / mquat, else the bodies' pos / quat), the NaN
 * auto-reset too.  Not MRS_FIELD_* values: host layout pos [n][nmocap][3], quat [n][nmocap][4] fp64 for
 * envs [env0, env0+n); either pointer may be NULL (that part is left as it is / not read back); with
 * nmocap == 0 set / get succeed and copy nothing. */
int mrs_batch_set_mocap(mrs_batch* b, const double* pos, const double* quat, int env0, int n);
int mrs_batch_get_mocap(mrs_batch* b, double* pos, double* quat, int env0, int n);
/* device pointers of the poses, [n_envs][nmocap][3] and [n_envs][nmocap][4] fp32; a write ordered on the
 * batch stream takes effect at the next step / forward launch.  NULL when nmocap == 0. */
float* mrs_batch_mocap_pos_device_ptr(mrs_batch* b);
float* mrs_batch_mocap_quat_device_ptr(mrs_batch* b);

/* ---- per-env model parameters (no reference counterpart: the reference steps one mjData of one
 * mjModel; here every env of a batch may carry its own values of the mjModel attributes that domain
 * randomisation draws most and that have no derived constants in the compiled model, so writing them is
 * exactly compiling the scene with those attributes changed).  Not MRS_FIELD_* values. */
enum {
  MRS_PARAM_ACT_GAINPRM = 0,   /* [nu][3]  mjModel.actuator_gainprm[:, 0:3] */
  MRS_PARAM_ACT_BIASPRM = 1,   /* [nu][3]  mjModel.actuator_biasprm[:, 0:3] */
  MRS_PARAM_DOF_DAMPING = 2,   /* [nv] */
  MRS_PARAM_GEOM_FRICTION = 3, /* [ngeom]  sliding coefficient only */
  MRS_PARAM_COUNT = 4
};
/* floats per env of a parameter (3 nu, 3 nu, nv, ngeom), < 0 on error */
int mrs_batch_param_dim(const mrs_batch* b, int param);
/* host rows [n][dim] fp64 for envs [env0, env0+n).  A parameter's buffer is made on the first
 * set_param / param_device_ptr of that parameter, every env filled with the model's own fp32 values;
 * before that get_param returns the model's values for every env and the launches take none of the
 * per-env code for that parameter.  Model values, not data values: mrs_batch_reset, both masked resets
 * and the NaN auto-reset leave them untouched.  The values hold over the n steps of a launch and over
 * RK4's stages.  The actuator's gaintype / biastype stay the model's: a fixed gain ignores
 * gainprm[1:3], bias type none ignores all of biasprm.  A position actuator's kp lives in both
 * gainprm[0] and -biasprm[1] (and kv in -biasprm[2]); as with mjModel, keeping them consistent is the
 * caller's job.  Friction: an automatic pair's sliding friction is max of its two geoms' per-env values
 * (mj_contactParam with equal priorities); explicit <contact><pair> entries keep the pair's own;
 * torsional and rolling friction stay the model's.  The one exception to "a write equals compiling the
 * scene with the attribute changed": an explicit pair written without friction= took max of its geoms'
 * friction when the model was compiled, and keeps that compiled value -- it does not follow the per-env
 * geom values.  set_param rejects a bad param, env0 or n, non-finite
 * values, and negative damping or friction with MRS_ERR_INVALID (nothing is written then). */
int mrs_batch_set_param(mrs_batch* b, int param, const double* host, int env0, int n);
int mrs_batch_get_param(mrs_batch* b, int param, double* host, int env0, int n);
/* device pointer of a parameter's buffer, [n_envs][dim] fp32 (made by this call if need be); a write
 * ordered on the batch stream takes effect at the next step / forward launch.  Writes through it are not
 * checked.  NULL when dim == 0 or on error (mrs_last_status). */
float* mrs_batch_param_device_ptr(mrs_batch* b, int param);

/* ---- per-env body mass, inertia and dof armature (no reference counterpart).  A family of its own, not
 * MRS_PARAM_* values: these have derived constants in the compiled model, and a write is exactly "set
 * those mjModel arrays, then mj_setConst" -- the env then steps as a model whose body_subtreemass,
 * dof_M0, stat_meaninertia, dof_invweight0 and body_invweight0 were derived from the new values at
 * qpos0 (and whose friction-loss rows' regulariser and solver scale follow).  body_ipos / body_iquat
 * stay the model's; body_inertia is the principal moments in the compiled body_iquat frame.  Two
 * exceptions: a kv that the compiler derived from dampratio keeps its compiled value (mj_setConst does
 * not redo it either; MRS_PARAM_ACT_BIASPRM moves it), and a model with tendons is refused with
 * MRS_ERR_UNSUPPORTED (tendon_invweight0 is a follow-up).  Model values: mrs_batch_reset, both masked
 * resets and the NaN auto-reset leave them alone; they hold over the n steps of a launch and RK4's
 * stages.  Row 0 (the world) is ignored on write and reads back the model's.  There is no
 * device-pointer call: a raw device write would leave the derived constants stale. */
enum { MRS_INERTIAL_BODY_MASS = 0, MRS_INERTIAL_BODY_INERTIA = 1, MRS_INERTIAL_DOF_ARMATURE = 2,
       MRS_INERTIAL_COUNT = 3 };
int mrs_batch_inertial_dim(const mrs_batch* b, int which);             /* nbody, 3 nbody, nv */
/* host rows [n][dim] fp64 for envs [env0, env0+n); a NULL pointer leaves that quantity as it is.
 * One re-derivation per env per call (host, fp64, the compiler's own function; the results are rounded
 * to fp32 as the model block is).  The per-env storage is made on the first set; before that
 * get_inertial returns the model's values and no launch takes any per-env code.  MRS_ERR_INVALID for a
 * non-finite or negative value and for a row whose M(qpos0) is not positive definite (for example zero
 * mass and inertia on a moving body with zero armature); a rejected call writes nothing for any env. */
int mrs_batch_set_inertial(mrs_batch* b, const double* mass, const double* inertia,
                           const double* armature, int env0, int n);
int mrs_batch_get_inertial(mrs_batch* b, double* mass, double* inertia, double* armature, int env0, int n);
/* what the kernels read for env `env` (fp32 on the device, widened): for tests and debugging.
 * body_subtreemass [nbody], dof_invweight0 [nv], body_invweight0 [nbody][2], meaninertia [1] (from the
 * stored solver scale 1 / (meaninertia max(1, nv))); any output NULL = not wanted */
int mrs_batch_get_inertial_derived(mrs_batch* b, int env, double* body_subtreemass, double* dof_invweight0,
                                   double* body_invweight0, double* meaninertia);

/* replaces mj_step (src/mujoco_system_interface.cpp:1691,1731): advance every env n_steps times,
 * fused in one launch; ctrl / qfrc_applied are held constant (zero-order hold) across the n steps,
 * exactly as PhysicsLoop holds them between write() calls.  Asynchronous on the batch stream.
 * sensordata afterwards is that of the last step's forward pass, as after n_steps mj_step calls; the
 * steps before the last do not evaluate sensors (nothing can read their values, and sensors feed
 * nothing back into the dynamics).  MRS_SENSORS_EVERY_STEP=1 in the environment at batch creation
 * evaluates them every step instead: the same outputs, for A/B runs. */
int mrs_batch_step(mrs_batch* b, int n_steps);
/* replaces mj_forward (src/mujoco_system_interface.cpp:741,1771): recompute outputs (sensordata,
 * qfrc_actuator, qacc) for the current state without integrating */
int mrs_batch_forward(mrs_batch* b);
/* depth image of camera `cam` for envs [env0, env0+n): host out [n][H][W] fp32, rows already
 * flipped to ROS order and linearised to eye-space z (replaces mjr_render + mjr_readPixels +
 * the linearisation loop of src/mujoco_cameras.cpp:211-240) */
int mrs_batch_render_depth(mrs_batch* b, int cam, int env0, int n, float* host_out);
/* same, into a device buffer [n][H][W] (stays in HBM) */
int mrs_batch_render_depth_device(mrs_batch* b, int cam, int env0, int n, float* d_out);
/* depth and colour in one pass (the RGB8 image of src/mujoco_cameras.cpp:211-240): depth as above,
 * rgb [n][H][W][3] uint8, ROS row order, each pixel's nearest geom shaded by MuJoCo's fixed-function
 * lighting model restated per pixel (headlight and model lights, shadows, materials, builtin
 * textures; the skybox where nothing is hit) -- not an OpenGL raster match */
int mrs_batch_render_rgbd(mrs_batch* b, int cam, int env0, int n, float* host_depth, unsigned char* host_rgb);
/* same, into device buffers */
int mrs_batch_render_rgbd_device(mrs_batch* b, int cam, int env0, int n, float* d_depth, unsigned char* d_rgb);
/* camera pipeline (the reference's rendering thread: mjv_copyData of the live data under the sim
 * mutex, then mjv_updateScene + mjr_render of the copy while PhysicsLoop steps on,
 * src/mujoco_cameras.cpp:204-215): snapshot the poses of the last step on the batch stream, then
 * render depth (and colour when d_rgb is not NULL) from the snapshot on the batch's own render stream,
 * concurrently with the steps queued after this call.  Device buffers as mrs_batch_render_rgbd_device.
 * A later snapshot waits until the previous asynchronous render has read the old one. */
int mrs_batch_render_async(mrs_batch* b, int cam, int env0, int n, float* d_depth, unsigned char* d_rgb);
/* order the batch stream after the last asynchronous render (its frames are complete for any work
 * queued on the batch stream afterwards; mrs_batch_sync also waits for it) */
int mrs_batch_render_wait(mrs_batch* b);

/* ---- batched ray queries against the posed scene: mj_ray / mj_multiRay for every env (the reference's
 * lidar is built on mj_ray, src/mujoco_lidar.cpp).  Height scanners, lidar patterns and line-of-sight
 * tests need no <rangefinder> per ray, and the rays may change from one call to the next. */
enum {
  MRS_RAY_SHARED = 1,    /* flags: pnt / vec are one pattern [n_rays][3] for every env */
  MRS_RAY_NO_STATIC = 2  /* flags: drop the geoms of bodies welded to the world (mj_ray flg_static = 0) */
};
enum {
  MRS_RAY_FRAME_WORLD = 0,  /* pnt / vec are world coordinates; frame_id is ignored */
  MRS_RAY_FRAME_GEOM = 1,   /* in geom frame_id's frame: each env's own pose of that geom */
  MRS_RAY_FRAME_CAMERA = 2  /* in camera frame_id's frame, likewise */
};
/* Rays: d_pnt and d_vec are device fp32 [n_envs][n_rays][3], with MRS_RAY_SHARED [n_rays][3]; outputs
 * d_dist fp32 and d_geomid int32 (may be NULL) are [n_envs][n_rays].  As in mj_ray, vec need not be
 * normalised and dist is in units of |vec|; a miss gives dist -1 and geomid -1.  A zero vec (or one whose
 * squared length is not a positive finite fp32 number) is a miss, never a NaN.  The nearest hit wins; equal
 * distances go to the lower geom id.  n_rays == 0 succeeds without a launch (the pointers are not looked at).
 *
 * Frames are the poses the device already holds: the world, a geom or a camera.  A pattern mounted on a
 * site or body is the caller's to build: read MRS_DYNOUT_SITE_POSE on the device and pass per-env world
 * rays.
 *
 * Filters, with mj_ray's meaning: group_mask bit g (0..5) keeps the geoms of group g, 0 keeps every group
 * (geomgroup == NULL), and with a mask a geom whose group is outside 0..5 is dropped; MRS_RAY_NO_STATIC
 * drops the geoms of bodies with body_weldid == 0 (the world's and those welded to it, mocap bodies
 * included); bodyexclude drops one body's geoms (-1: none); geoms with rgba alpha exactly 0 are always
 * dropped.  Height fields are never hit.
 *
 * Which poses: those of the last mrs_batch_step / mrs_batch_forward, as mj_ray reads mjData.  After
 * mrs_batch_step(b, n) they belong to the last step's forward pass, i.e. the state BEFORE that step's
 * integration; a caller who wants them at the current qpos calls mrs_batch_forward first.  Before any
 * step or forward the call reads the pose buffers as they are, as mrs_batch_render_depth does: batch
 * creation runs one forward, so they hold the poses at qpos0, and a reset or a qpos write does not
 * move them.
 *
 * Asynchronous on the batch stream, no synchronisation: stream order alone places the query after the
 * launches queued before.  The first query with a new (group_mask, NO_STATIC, bodyexclude) triple uploads
 * that filter's geom list (a short synchronising copy); the batch keeps the last few, so a repeated query
 * does no host work beyond the launch.
 * MRS_ERR_INVALID, before any launch, for a null handle, a null d_pnt / d_vec / d_dist, negative n_rays, an
 * unknown flag or frame type, frame_id outside the geoms / cameras, bodyexclude outside [-1, nbody). */
int mrs_batch_ray_device(mrs_batch* b, const float* d_pnt, const float* d_vec, int n_rays, int flags,
                         int frame_type, int frame_id, unsigned group_mask, int bodyexclude,
                         float* d_dist, int* d_geomid);
/* same with host fp64 arrays for envs [env0, env0 + n): pnt / vec [n][n_rays][3] (or [n_rays][3] shared),
 * dist and geomid (may be NULL) [n][n_rays].  Stages the rays (through fp32, as mrs_batch_set_field
 * converts), launches and synchronises.  Also MRS_ERR_INVALID for an env range outside the batch; n == 0
 * succeeds without a launch. */
int mrs_batch_ray(mrs_batch* b, const double* pnt, const double* vec, int n_rays, int flags,
                  int frame_type, int frame_id, unsigned group_mask, int bodyexclude,
                  double* dist, int* geomid, int env0, int n);
/* mjData.contact of env `env` after its last step / forward (the output of mj_collision, SURVEY.md
 * §8a row a2.3): up to `max` contacts in mj_collision's order -- geom [max][2] int32 (geom1, geom2,
 * the lower geom type first), dist [max], pos [max][3], frame [max][9] fp64 (normal = frame[0:3]);
 * any output pointer may be NULL.  Returns ncon (which may exceed `max`) or a negative error code. */
int mrs_batch_get_contacts(mrs_batch* b, int env, int max, int* geom, double* dist, double* pos,
                           double* frame);
/* mj_contactForce of every contact of mrs_batch_get_contacts' list for env `env`, in its order: force
 * [max][6] fp64 in the contact frame -- normal, tangent 1, tangent 2, then three zeros (condim 1 and 3
 * carry no torque).  Decoded on the host from the env's contact records and the solver's row forces
 * (the pyramid's edges as mju_decodePyramid, an elliptic block as it is, condim 1 its one row); a
 * contact whose rows the row cap cut gives zeros.  The pyramidal decode's friction is the pair's as the
 * kernel sees it: per-env MRS_PARAM_GEOM_FRICTION where set (max of the two geoms for automatic pairs;
 * an explicit <contact><pair> keeps its own).  Needs no device output to be on.  Returns ncon (which
 * may exceed `max`) or a negative error code. */
int mrs_batch_get_contact_forces(mrs_batch* b, int env, int max, double* force);
/* The net contact wrench per body, an output of the step: [n_envs][nbody][6] fp32.  Row b sums, in
 * contact order, the step's contacts that involve body b: [0:3] the world-frame force on the body,
 * [3:6] the world-frame torque about the body's centre of mass xipos_b -- MRS_FIELD_XFRC_APPLIED's
 * layout and reference point, so writing a row back as xfrc_applied with contacts disabled reproduces
 * the contacts' effect on that body.  Row 0 holds the wrench on the world's geoms, torque about the
 * world origin; the rows' forces sum to zero.  Signs as mj_contactForce: the contact normal points
 * from geom1 to geom2, the decoded force acts on geom2's body at the contact point, its negative on
 * geom1's.  Zeros with contacts or constraints disabled; not a sensor (MRS_DSBL_SENSOR does not cover
 * it).  The buffer does not exist until one of these two calls, which makes it zero-filled and turns
 * the output on for all later launches; it is then written by the last step of every mrs_batch_step
 * launch and by mrs_batch_forward, and no reset changes it.
 * mrs_batch_contact_wrench_device_ptr: the device buffer; reads ordered on the batch stream see the last
 * launch's values.  NULL on error, the code in mrs_last_status.
 * mrs_batch_get_contact_wrench: host rows [n][nbody][6] fp64 of envs [env0, env0 + n); zeros until a
 * step or forward has been launched after the output was turned on. */
float* mrs_batch_contact_wrench_device_ptr(mrs_batch* b);
int mrs_batch_get_contact_wrench(mrs_batch* b, double* host, int env0, int n);
/* The dynamics outputs: what model-based control is built from (gravity compensation tau = qfrc_bias,
 * computed torque tau = M qdd + qfrc_bias, Cartesian impedance tau = J' F), per env, on the device.
 * (The constants are MRS_DYNOUT_*, not MRS_DYN_*: that prefix is the actuator dyntype's, mrs_model.h.) */
enum {
  MRS_DYNOUT_QFRC_BIAS = 0,   /* [nv]          mjData.qfrc_bias (Coriolis, centrifugal, gravity) */
  MRS_DYNOUT_MASS_MATRIX = 1, /* [nv][nv]      mj_fullM: dense, symmetric, both triangles written, zeros between trees */
  MRS_DYNOUT_SITE_JAC = 2,    /* [nsel][6][nv] mj_jacSite: rows 0..2 jacp, rows 3..5 jacr, world frame */
  MRS_DYNOUT_SITE_POSE = 3,   /* [nsel][12]    mjData.site_xpos [3] then site_xmat [9] row-major */
  MRS_DYNOUT_COUNT = 4
};
#define MRS_MAX_JAC_SITES 16
/* Each output is a device buffer [n_envs][dim] fp32 that does not exist until it is first asked for
 * (mrs_batch_dyn_device_ptr or mrs_batch_get_dyn with that `which`): that call makes it zero-filled and
 * turns the output on for all later launches; a batch with no output on launches the kernels it
 * launched before, which hold none of this code.  They are outputs, not sensors: MRS_DSBL_SENSOR does not cover them.
 *
 * Which state the values belong to: the forward pass whose sensors are in sensordata.  After
 * mrs_batch_step(b, n) that is the last step's forward pass, i.e. the state BEFORE that step's
 * integration -- what mjData holds after mj_step (under RK4 the step's first stage; under
 * MRS_SENSORS_EVERY_STEP=1 the same pass).  After mrs_batch_forward it is the current qpos / qvel.  A
 * controller that wants values consistent with the qpos it reads calls mrs_batch_forward.  No reset
 * writes the buffers (as none writes qacc); the re-run of a step after a NaN auto-reset writes them
 * like any other forward pass.
 *
 * The mass matrix and qfrc_bias are the env's own: copies of what the env's step used, so they carry
 * per-env masses, inertias and armatures (mrs_batch_set_inertial) -- which a host-side model cannot
 * give.  qfrc_bias follows MRS_DSBL_GRAVITY as the step's own does.
 *
 * mrs_batch_set_jac_sites: the sites (ids from mrs_name2id(MRS_OBJ_SITE), n in [0, MRS_MAX_JAC_SITES])
 * that SITE_JAC and SITE_POSE cover, in the given order; nsel = n.  With no selection nsel = 0: the two
 * dimensions are 0, their device pointer is NULL (mrs_last_status MRS_OK) and mrs_batch_get_dyn copies
 * nothing.  Changing the selection synchronises, frees the two buffers and remakes those that have
 * been asked for zero-filled (device pointers obtained before are invalid).  MRS_ERR_INVALID for an id outside
 * [0, nsite), a duplicate, or n > MRS_MAX_JAC_SITES; a rejected call changes nothing.
 * mrs_batch_dyn_dim: floats per env of the output (negative error code for an unknown `which`).
 * mrs_batch_dyn_device_ptr: the device buffer; reads ordered on the batch stream see the last launch's
 * values.  NULL on error, the code in mrs_last_status.
 * mrs_batch_get_dyn: host rows [n][dim] fp64 of envs [env0, env0 + n); zeros until a step or forward
 * has been launched after the output was turned on. */
int mrs_batch_set_jac_sites(mrs_batch* b, const int* site_ids, int n);
int mrs_batch_dyn_dim(const mrs_batch* b, int which);
float* mrs_batch_dyn_device_ptr(mrs_batch* b, int which);
int mrs_batch_get_dyn(mrs_batch* b, int which, double* host, int env0, int n);
/* mjData.efc_* of env `env` after its last step / forward (the rows mj_makeConstraint built and the
 * solver's forces): up to `max` rows in mj_makeConstraint's order --
 * type [max] int32 (1 friction loss, 2 joint limit, 3 contact), J [max][nv], R [max], aref [max],
 * force [max] fp64; any output pointer may be NULL.  Returns nefc (which may exceed `max`), or
 * MRS_ERR_UNSUPPORTED for the layouts that keep no dense rows (the register friction-loss path of
 * models without contacts or active limits, and PGS in blocked mode, whose rows are sparse). */
int mrs_batch_get_efc(mrs_batch* b, int env, int max, int* type, double* J, double* R, double* aref,
                      double* force);
/* fp32 state field rows of envs [env0, env0+n) into a device buffer [n][dim], asynchronous on the
 * batch stream (observations for the end-of-step gather stay in HBM; no reference counterpart: the
 * reference copies mjData on the host, src/mujoco_system_interface.cpp:1759) */
int mrs_batch_get_field_device(mrs_batch* b, int field, float* d_out, int env0, int n);
/* wait for all queued batch work */
int mrs_batch_sync(mrs_batch* b);
/* duration in ms of the last step / render kernel measured with HIP events on the batch stream
 * (kind 0 = step, 1 = depth), -1 if unavailable (no such launch yet, or its kind is not timed) */
double mrs_batch_last_kernel_ms(mrs_batch* b, int kind);
/* which launches the batch brackets with its own HIP events for mrs_batch_last_kernel_ms: bit 0 step
 * launches, bit 1 frames (default 2: frames only).  A timed step launch costs ~10 us (a C3 10-step
 * launch 0.420 vs 0.410 ms), so step launches are timed only when asked for */
int mrs_batch_set_timing(mrs_batch* b, int mask);
/* diagnostics (no reference counterpart): per-phase wave-cycle totals of the step kernel since the
 * last reset, in phase order kinematics, com_pos, make_M, cholesky, com_vel, rne, smooth_forces,
 * collision, constraints, sensors, integrate, checks.  Only a library built with
 * -DMRS_PHASE_TIMING records them; returns the number of phases written (0 otherwise, <0 on error). */
int mrs_debug_phase_cycles(double* out, int n, int reset);
/* diagnostics: the batch's kernel configuration -- out[0] lanes per env (group width), [1] LDS floats
 * per env, [2] scratch floats per env, [3] blocked mode (tree-blocked M + sparse constraint rows),
 * [4] dof slots per constraint row (pipe width), [5] constraint-row capacity, [6] contact capacity,
 * [7] kinematic trees with dofs, [8] workgroup-shared LDS floats, [9] lidar rays read from the
 * workgroup's LDS table (1) or the model block (0), [10] one workgroup per CU (16-lane groups kept for
 * tables past the two-per-CU budget), [11] waves per workgroup of a 16-lane batch (0 otherwise),
 * [12] helper waves (collision, rows, rays and the integrator factor beside the dynamics), [13] the
 * integrator's factor fused into the Cholesky phase, [14] ray sweep of a static planar lidar, [15]
 * sensors evaluated on every step of a fused launch (MRS_SENSORS_EVERY_STEP=1) instead of the last
 * only, [16] the contact-wrench output on (1; mrs_batch_contact_wrench_device_ptr) or not (0), [17]
 * the dynamics outputs that are on, a bit mask (1 << MRS_DYNOUT_*; a site output's bit only while sites
 * are selected), [18] the fused 16-lane solves (1: one reciprocal per lane and solve, qacc_smooth solved
 * with the friction-loss rows; 0: not a 16-lane PGS batch without helper waves, or MRS_NO_SOLVE_FUSE=1 --
 * that switch gives the same bits by the separate solves, run out of line: a reference for results, not
 * for speed), [19] the collision pairs the step walks and [20] the statically admissible pairs left out
 * of them because their geoms can never touch (mrs_debug_pairs), [21] the launches stage the workgroup-
 * shared tables from one packed image (1) or table by table, out of line (0: MRS_NO_TABLE_IMAGE=1 at batch
 * creation, a reference for results, not for speed).
 * Returns the number of values written. */
int mrs_debug_batch_layout(const mrs_batch* b, int* out, int n);
/* diagnostics: the collision pairs a batch of this model walks each step, in contact order: the explicit
 * <contact><pair>s, then the pairs the static filters admit (mrs_model_view pair_geom1/2) without those
 * whose geoms can never touch -- each geom's centre stays in a ball fixed in the world (its own position
 * when its body is welded to the world; about the first joint's anchor when only hinge and ball joints,
 * one per body, lie above it), and the balls, the bounding spheres and the margin leave a gap.  Geoms below
 * a slide or free joint or a mocap body have no such ball and keep their pairs; explicit pairs always
 * stay.  MRS_NO_PAIR_PRUNE=1 (read here and at batch creation) keeps every pair.  Up to `max` pairs are
 * written to geom [max][2] (may be NULL when max == 0) and the number of pruned pairs to *pruned (may be
 * NULL); returns the count of walked pairs, which may exceed `max`, MRS_ERR_INVALID for a null or bad
 * argument, MRS_ERR_UNSUPPORTED for a model mrs_batch_create refuses with it.  No device needed. */
int mrs_debug_pairs(const mrs_model* m, int* geom, int max, int* pruned);
/* diagnostics: values [0] to [15] above as mrs_batch_create would choose them for n_envs environments on
 * a device with cu_count compute units (<= 0: unknown, as when the query fails) and max_contacts (<= 0:
 * from the model), without a device: the environment switches are read, the model's tables built and
 * the plan chosen, nothing else.  Returns the number of values written, MRS_ERR_INVALID for a null or
 * bad argument, MRS_ERR_UNSUPPORTED for a model mrs_batch_create refuses with it. */
int mrs_debug_plan_layout(const mrs_model* m, int n_envs, int cu_count, int max_contacts, int* out, int n);
/* diagnostics: the workgroup-shared tables of the step kernel as the one packed image a batch uploads and
 * every launch copies into LDS (the same arguments as mrs_debug_plan_layout choose the plan): up to `max`
 * floats of it to image (may be NULL when max == 0), and to offsets[0..17] the plan's table offsets in
 * floats -- ray directions, static ray hits, ray blocks, sensor records, friction-loss rows, limit rows,
 * actuator, dof, body, mass-matrix pair, jump, kinematics body / joint / geom tables (the ray-geom records
 * are at 0), the end of the tables, the workgroup's shared floats -- then [16] blocked mode and [17] the
 * floats a launch copies (the tables' end; in blocked mode the actuator table's offset).  Returns the
 * image's length, a multiple of 4 (zero-padded).  No device needed. */
int mrs_debug_table_image(const mrs_model* m, int n_envs, int cu_count, int max_contacts, float* image, int max,
                          int* offsets, int n_off);
/* diagnostics: table `which` of those the image holds, as the model block holds it: 0 ray geoms, 1 rays (8
 * floats each), 2 ray blocks, 3 sensor records, 4 friction-loss rows, 5 limit rows, 6 actuators, 7 dofs,
 * 8 bodies, 9 mass-matrix pairs, 10 the jump table (int bits), 11 / 12 / 13 kinematics bodies / joints /
 * geoms.  Up to `max` floats to out; returns the table's length.  No device needed. */
int mrs_debug_staged_table(const mrs_model* m, int max_contacts, int which, float* out, int max);
/* diagnostics: how mrs_batch_render_depth / mrs_batch_render_async would render n_frames frames of camera
 * `cam` on a device with max_lds bytes of LDS per workgroup, without a device: the render switches
 * (MRS_DEPTH_V1, MRS_DEPTH_V2, MRS_RAST_BUDGET_MB) are read and the plan chosen, nothing else.  Values: [0]
 * the kernel (0: triangle binning, one workgroup per frame; 1: one workgroup per frame; 2: one workgroup
 * per 16 x 16 pixel tile), [1] the frame kernel's mesh code is compiled in, [2] dynamic LDS bytes of the
 * binning kernel's band, [3] frames per launch of the binning kernel, [4] bytes of one frame's triangle
 * list, [5] and [6] the grid (of the first launch).  Returns the number of values written,
 * MRS_ERR_INVALID for a null or bad argument, MRS_ERR_UNSUPPORTED for a model the render calls refuse. */
int mrs_debug_render_plan(const mrs_model* m, int cam, int n_frames, int max_lds, long long* out, int n);
/* diagnostics: the ids of the geoms a ray query with this group_mask, flags (MRS_RAY_NO_STATIC; MRS_RAY_SHARED
 * is accepted and ignored) and bodyexclude may hit, in geom order -- the list the batch uploads for the
 * query kernel.  Up to `max` ids are written to out (may be NULL when max == 0); returns the count, which
 * may exceed `max`, or MRS_ERR_INVALID for a null model, an unknown flag or a bodyexclude outside
 * [-1, nbody).  No device needed. */
int mrs_debug_ray_filter(const mrs_model* m, unsigned group_mask, int flags, int bodyexclude, int* out, int max);

#ifdef __cplusplus
}
#endif
#endif /* MRS_H */
