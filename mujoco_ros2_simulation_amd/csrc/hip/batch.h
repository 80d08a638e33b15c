// Internal C++ interface between the C ABI (capi.cc) and the HIP batch implementation.
#pragma once

#include <stdexcept>
#include <string>

namespace mrs {

struct Model;
struct BatchImpl;

struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };
struct UnsupportedError : std::runtime_error { using std::runtime_error::runtime_error; };

BatchImpl* batch_create(const Model* model, int n_envs, int device, int max_contacts);
void batch_free(BatchImpl* b);
int batch_num_envs(const BatchImpl* b);
int batch_layout(const BatchImpl* b, int* out, int n);  // diagnostics: kernel configuration
// its first 16 values as a batch of n_envs on a device with cu_count CUs would have them (no device)
int plan_layout(const Model& m, int n_envs, int cu_count, int max_contacts, int* out, int n);
// the collision pairs a batch of the model walks, [k][2] geom ids in contact order (up to max written;
// returns k), and how many admissible pairs were pruned from them (no device)
int walked_pairs(const Model& m, int* geom, int max, int* pruned);
// the packed workgroup-shared table image of a plan and its offsets, and one staged table as packed
int table_image(const Model& m, int n_envs, int cu_count, int max_contacts, float* image, int max, int* offsets, int n_off);
int staged_table(const Model& m, int max_contacts, int which, float* out, int max);
void batch_set_stream(BatchImpl* b, void* stream);
void batch_reset(BatchImpl* b, int key, int env0, int n);
// start-state pool (count rows; qvel may be null: zeros; count 0 frees it) and the masked reset
void batch_set_start_states(BatchImpl* b, const double* qpos, const double* qvel, int count);
void batch_set_start_states_device(BatchImpl* b, const float* d_qpos, const float* d_qvel, int count);
int batch_num_start_states(const BatchImpl* b);
void batch_reset_masked_device(BatchImpl* b, const unsigned char* d_mask, const int* d_key, int key);
void batch_reset_masked(BatchImpl* b, const unsigned char* mask, const int* keys, int key);
void batch_set(BatchImpl* b, int field, const double* host, int env0, int n);
void batch_get(BatchImpl* b, int field, double* host, int env0, int n);
void* batch_device_ptr(BatchImpl* b, int field);
// the activations [n][na] (mjData.act; no MRS_FIELD_* value of their own)
void batch_set_act(BatchImpl* b, const double* host, int env0, int n);
void batch_get_act(BatchImpl* b, double* host, int env0, int n);
float* batch_act_device_ptr(BatchImpl* b);  // null when na == 0
// the mocap poses [n][nmocap][3] / [n][nmocap][4] (mjData.mocap_pos / mocap_quat); a null part is skipped
void batch_set_mocap(BatchImpl* b, const double* pos, const double* quat, int env0, int n);
void batch_get_mocap(BatchImpl* b, double* pos, double* quat, int env0, int n);
float* batch_mocap_pos_device_ptr(BatchImpl* b);   // null when nmocap == 0
float* batch_mocap_quat_device_ptr(BatchImpl* b);  // null when nmocap == 0
// per-env model parameters (MRS_PARAM_*): floats per env (throws on a bad param), host rows [n][dim],
// and the device buffer [n_envs][dim], made on the first set / device_ptr (null when dim == 0)
int batch_param_dim(BatchImpl* b, int param);
void batch_set_param(BatchImpl* b, int param, const double* host, int env0, int n);
void batch_get_param(BatchImpl* b, int param, double* host, int env0, int n);
float* batch_param_device_ptr(BatchImpl* b, int param);
// per-env body mass / inertia / dof armature (MRS_INERTIAL_*): host rows [n][dim], a null part is left
// as it is; every set re-derives the env's constants on the host (start_rows.h inertial_row)
int batch_inertial_dim(BatchImpl* b, int which);
void batch_set_inertial(BatchImpl* b, const double* mass, const double* inertia, const double* armature, int env0, int n);
void batch_get_inertial(BatchImpl* b, double* mass, double* inertia, double* armature, int env0, int n);
void batch_get_inertial_derived(BatchImpl* b, int env, double* body_subtreemass, double* dof_invweight0,
                                double* body_invweight0, double* meaninertia);
void batch_set_ctrl_device(BatchImpl* b, const float* d_ctrl);
void batch_bind_ctrl_device(BatchImpl* b, const float* d_ctrl);  // zero-copy ctrl source (null: own buffer)
void batch_set_timing(BatchImpl* b, int mask);  // launches timed for batch_last_kernel_ms (bit 0 step, 1 frames)
void batch_launch(BatchImpl* b, int n_steps, bool forward_only);
// rgb (may be null): n * H * W * 3 bytes, same host/device side as out
void batch_render_depth(BatchImpl* b, int cam, int env0, int n, float* out, bool device_out, unsigned char* rgb = nullptr);
void batch_render_async(BatchImpl* b, int cam, int env0, int n, float* d_out, unsigned char* d_rgb);
void batch_render_wait(BatchImpl* b);
// the plan of n_frames frames of camera `cam` on a device with max_lds bytes of LDS per workgroup (no
// device): kernel kind, kMesh, band LDS bytes, frame chunk, list bytes per frame, grid x and y (renderplan.h)
int render_plan(const Model& m, int cam, int n_frames, int max_lds, long long* out, int n);
// ray queries against the poses of the last step / forward (mrs.h MRS_RAY_*): device rays and outputs for
// every env, asynchronous on the batch stream, and host fp64 rows for envs [env0, env0 + n), synchronised;
// geomid may be null.  Every argument is checked before any launch
void batch_ray_device(BatchImpl* b, const float* d_pnt, const float* d_vec, int n_rays, int flags, int frame_type,
                      int frame_id, unsigned group_mask, int bodyexclude, float* d_dist, int* d_geomid);
void batch_ray(BatchImpl* b, const double* pnt, const double* vec, int n_rays, int flags, int frame_type, int frame_id,
               unsigned group_mask, int bodyexclude, double* dist, int* geomid, int env0, int n);
int batch_get_contacts(BatchImpl* b, int env, int max, int* geom, double* dist, double* pos, double* frame);
int batch_get_efc(BatchImpl* b, int env, int max, int* type, double* J, double* R, double* aref, double* force);
// mj_contactForce per contact of batch_get_contacts' list ([max][6], contact frame; returns ncon), and the
// net contact wrench per body [n_envs][nbody][6]: its device buffer, made on first use, which turns the
// output on for every later launch, and host rows [n][nbody][6]
int batch_get_contact_forces(BatchImpl* b, int env, int max, double* force);
float* batch_contact_wrench_device_ptr(BatchImpl* b);
void batch_get_contact_wrench(BatchImpl* b, double* host, int env0, int n);
// the dynamics outputs (mrs.h MRS_DYNOUT_*): the site selection, floats per env, the device buffer (made on
// first use, which turns the output on for every later launch) and host rows [n][dim]
void batch_set_jac_sites(BatchImpl* b, const int* site_ids, int n);
int batch_dyn_dim(const BatchImpl* b, int which);
float* batch_dyn_device_ptr(BatchImpl* b, int which);
void batch_get_dyn(BatchImpl* b, int which, double* host, int env0, int n);
void batch_get_field_device(BatchImpl* b, int field, float* d_out, int env0, int n);
void batch_sync(BatchImpl* b);
double batch_last_kernel_ms(BatchImpl* b, int kind);
int phase_cycles(double* out, int n, bool reset);  // step_dispatch.hip; step.hip in profiling builds

}  // namespace mrs
