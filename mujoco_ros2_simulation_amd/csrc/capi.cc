// C ABI (include/mrs.h): exception firewall + handle management.  Every entry point catches, stores
// the message in a thread-local buffer (mrs_last_error) and returns an MRS_ERR_* code or NULL.
#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mrs.h"
#include "hip/batch.h"
#include "mjcf/model.h"
#include "hip/rayfilter.h"
#include "hip/start_rows.h"
#include "mjcf/xml.h"

struct mrs_model {
  mrs::Model m;
};
struct mrs_batch {
  mrs::BatchImpl* impl = nullptr;
  const mrs_model* model = nullptr;
};

namespace {

thread_local std::string g_last_error;
thread_local int g_last_code = MRS_OK;

void set_error(const std::string& msg) { g_last_error = msg; }

template <class F>
int guarded_impl(F&& f) {
  try {
    g_last_error.clear();
    f();
    return MRS_OK;
  } catch (const mrs::DeviceError& e) {
    set_error(e.what());
    return MRS_ERR_DEVICE;
  } catch (const mrs::UnsupportedError& e) {
    set_error(e.what());
    return MRS_ERR_UNSUPPORTED;
  } catch (const std::invalid_argument& e) {
    set_error(e.what());
    return MRS_ERR_INVALID;
  } catch (const std::exception& e) {
    set_error(e.what());
    return MRS_ERR_INVALID;
  } catch (...) {
    set_error("unknown error");
    return MRS_ERR_INVALID;
  }
}

template <class F>
int guarded(F&& f) {
  g_last_code = guarded_impl(f);
  return g_last_code;
}

bool ends_with(const std::string& s, const char* suffix) {
  const size_t n = std::strlen(suffix);
  return s.size() > n && s.compare(s.size() - n, n, suffix) == 0;
}

void copy_error(char* error, int error_len) {
  if (error && error_len > 0) {
    std::strncpy(error, g_last_error.c_str(), static_cast<size_t>(error_len) - 1);
    error[error_len - 1] = '\0';
  }
}

}  // namespace

extern "C" {

const char* mrs_last_error(void) { return g_last_error.c_str(); }
int mrs_last_status(void) { return g_last_code; }

mrs_model* mrs_model_load_xml(const char* path, char* error, int error_len) {
  std::unique_ptr<mrs_model> out;
  int rc = guarded([&] {
    if (!path || !*path) throw std::invalid_argument("empty model path");
    // the reference loads a path ending in ".mjb" with mj_loadModel (src/mujoco_system_interface.cpp:
    // 307-310): MuJoCo's binary format is a version-specific dump of mjModel that this compiler does
    // not read -- fail with MRS_ERR_UNSUPPORTED instead of handing binary data to the XML parser
    if (ends_with(path, ".mjb") || ends_with(path, ".MJB"))
      throw mrs::UnsupportedError(std::string("could not load binary model ") + path +
                                  ": MuJoCo .mjb files (mj_loadModel) are not supported, load the MJCF XML");
    out.reset(new mrs_model{mrs::compile_mjcf_file(path)});
  });
  if (rc != MRS_OK) {
    // parse / compile failures report MRS_ERR_LOAD; features outside the subset MRS_ERR_UNSUPPORTED
    if (rc != MRS_ERR_UNSUPPORTED) g_last_code = MRS_ERR_LOAD;
    copy_error(error, error_len);
    return nullptr;
  }
  if (error && error_len > 0) error[0] = '\0';
  return out.release();
}

mrs_model* mrs_model_load_xml_string(const char* xml, const char* basedir, char* error, int error_len) {
  std::unique_ptr<mrs_model> out;
  int rc = guarded([&] {
    if (!xml) throw std::invalid_argument("null XML string");
    out.reset(new mrs_model{mrs::compile_mjcf_string(xml, basedir ? basedir : ".")});
  });
  if (rc != MRS_OK) {
    // parse / compile failures report MRS_ERR_LOAD; features outside the subset MRS_ERR_UNSUPPORTED
    if (rc != MRS_ERR_UNSUPPORTED) g_last_code = MRS_ERR_LOAD;
    copy_error(error, error_len);
    return nullptr;
  }
  if (error && error_len > 0) error[0] = '\0';
  return out.release();
}

void mrs_model_free(mrs_model* m) { delete m; }

mrs_model* mrs_model_copy(const mrs_model* m) {
  std::unique_ptr<mrs_model> out;
  int rc = guarded([&] {
    if (!m) throw std::invalid_argument("null model");
    out.reset(new mrs_model{m->m});
  });
  return rc == MRS_OK ? out.release() : nullptr;
}

int mrs_model_view_get(const mrs_model* m, mrs_model_view* out) {
  return guarded([&] {
    if (!m || !out) throw std::invalid_argument("null argument");
    *out = m->m.view();
  });
}

int mrs_model_derive_inertial(const mrs_model* m, const double* body_mass, const double* body_inertia,
                              const double* dof_armature, double* body_subtreemass, double* dof_M0,
                              double* dof_invweight0, double* body_invweight0, double* meaninertia) {
  return guarded([&] {
    if (!m) throw std::invalid_argument("null model");
    const mrs::Model& mm = m->m;
    if (!mm.tendon_adr.empty()) throw mrs::UnsupportedError("inertial re-derivation of a model with tendons (tendon_invweight0)");
    const double* mass = body_mass ? body_mass : mm.body_mass.data();
    const double* inertia = body_inertia ? body_inertia : mm.body_inertia.data();
    const double* armature = dof_armature ? dof_armature : mm.dof_armature.data();
    mrs::check_inertial_values(mm, mass, inertia, armature);
    mrs::setconst::InertialConst c;
    try {
      mrs::setconst::derive_inertial(mm, mass, inertia, armature, c);
    } catch (const std::runtime_error&) {
      throw std::invalid_argument("M(qpos0) is not positive definite for these inertial values");
    }
    auto put = [](double* dst, const std::vector<double>& v) { if (dst) std::copy(v.begin(), v.end(), dst); };
    put(body_subtreemass, c.body_subtreemass);
    put(dof_M0, c.dof_M0);
    put(dof_invweight0, c.dof_invweight0);
    put(body_invweight0, c.body_invweight0);
    if (meaninertia) *meaninertia = c.meaninertia;
  });
}

int mrs_model_set_restate(mrs_model* m, int flags) {
  return guarded([&] {
    if (!m) throw std::invalid_argument("null model");
    if (flags & ~(MRS_RESTATE_NEWTON_REFINE | MRS_RESTATE_PGS_ELLIPTIC_BLOCK | MRS_RESTATE_NO_MPR_POLISH |
                  MRS_RESTATE_NO_MULTICCD))
      throw std::invalid_argument("unknown restate bits");
    m->m.restate = flags;
  });
}

int mrs_name2id(const mrs_model* m, int objtype, const char* name) {
  if (!m || !name) return -1;
  return m->m.name2id(objtype, name);
}

const char* mrs_id2name(const mrs_model* m, int objtype, int id) {
  if (!m) return nullptr;
  return m->m.id2name(objtype, id);
}

// getActuatorType (src/mujoco_system_interface.cpp:433-460): MOTOR if no bias; POSITION if affine
// bias with biasprm[1] != 0; VELOCITY if affine with biasprm[1] == 0 and biasprm[2] != 0; else CUSTOM
int mrs_actuator_type(const mrs_model* m, int id) {
  if (!m || id < 0 || id >= m->m.nu) return 0;
  const mrs::Model& mm = m->m;
  const int biastype = mm.actuator_biastype[id];
  const double* bp = &mm.actuator_biasprm[static_cast<size_t>(id) * MRS_NBIAS];
  if (biastype == MRS_BIAS_NONE) return 1;
  if (biastype == MRS_BIAS_AFFINE && bp[1] != 0) return 2;
  if (biastype == MRS_BIAS_AFFINE && bp[1] == 0 && bp[2] != 0) return 3;
  return 4;
}

mrs_batch* mrs_batch_create(const mrs_model* m, int n_envs, int device) {
  std::unique_ptr<mrs_batch> b(new mrs_batch());
  int rc = guarded([&] {
    if (!m) throw std::invalid_argument("null model");
    b->model = m;
    b->impl = mrs::batch_create(&m->m, n_envs, device, 0);  // contact capacity from the model
  });
  return rc == MRS_OK ? b.release() : nullptr;
}

void mrs_batch_free(mrs_batch* b) {
  if (!b) return;
  guarded([&] { mrs::batch_free(b->impl); });
  delete b;
}

int mrs_batch_num_envs(const mrs_batch* b) { return b ? mrs::batch_num_envs(b->impl) : 0; }

int mrs_batch_set_stream(mrs_batch* b, void* stream) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_set_stream(b->impl, stream);
  });
}

int mrs_batch_reset(mrs_batch* b, int key, int env0, int n) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_reset(b->impl, key, env0, n);
  });
}

int mrs_batch_set_start_states(mrs_batch* b, const double* qpos, const double* qvel, int count) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_set_start_states(b->impl, qpos, qvel, count);
  });
}

int mrs_batch_set_start_states_device(mrs_batch* b, const float* d_qpos, const float* d_qvel, int count) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_set_start_states_device(b->impl, d_qpos, d_qvel, count);
  });
}

int mrs_batch_num_start_states(const mrs_batch* b) { return b ? mrs::batch_num_start_states(b->impl) : 0; }

int mrs_batch_reset_masked_device(mrs_batch* b, const unsigned char* d_mask, const int* d_key, int key) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_reset_masked_device(b->impl, d_mask, d_key, key);
  });
}

int mrs_batch_reset_masked(mrs_batch* b, const unsigned char* mask, const int* keys, int key) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_reset_masked(b->impl, mask, keys, key);
  });
}

int mrs_batch_set_field(mrs_batch* b, int field, const double* host, int env0, int n) {
  return guarded([&] {
    if (!b || !host) throw std::invalid_argument("null argument");
    mrs::batch_set(b->impl, field, host, env0, n);
  });
}

int mrs_batch_get_field(mrs_batch* b, int field, double* host, int env0, int n) {
  return guarded([&] {
    if (!b || !host) throw std::invalid_argument("null argument");
    mrs::batch_get(b->impl, field, host, env0, n);
  });
}

void* mrs_batch_device_ptr(mrs_batch* b, int field) {
  if (!b || field < 0 || field >= MRS_FIELD_COUNT) return nullptr;
  // (xfrc_applied's buffer is made on first use, which can fail: NULL then, the code in mrs_last_status)
  void* p = nullptr;
  guarded([&] { p = mrs::batch_device_ptr(b->impl, field); });
  return p;
}

int mrs_batch_set_ctrl_device(mrs_batch* b, const float* d_ctrl) {
  return guarded([&] {
    if (!b || !d_ctrl) throw std::invalid_argument("null argument");
    mrs::batch_set_ctrl_device(b->impl, d_ctrl);
  });
}

int mrs_batch_bind_ctrl_device(mrs_batch* b, const float* d_ctrl) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_bind_ctrl_device(b->impl, d_ctrl);
  });
}

int mrs_batch_set_act(mrs_batch* b, const double* host, int env0, int n) {
  return guarded([&] {
    if (!b || !host) throw std::invalid_argument("null argument");
    mrs::batch_set_act(b->impl, host, env0, n);
  });
}

int mrs_batch_get_act(mrs_batch* b, double* host, int env0, int n) {
  return guarded([&] {
    if (!b || !host) throw std::invalid_argument("null argument");
    mrs::batch_get_act(b->impl, host, env0, n);
  });
}

float* mrs_batch_act_device_ptr(mrs_batch* b) { return b ? mrs::batch_act_device_ptr(b->impl) : nullptr; }

int mrs_batch_set_mocap(mrs_batch* b, const double* pos, const double* quat, int env0, int n) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_set_mocap(b->impl, pos, quat, env0, n);
  });
}

int mrs_batch_get_mocap(mrs_batch* b, double* pos, double* quat, int env0, int n) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_get_mocap(b->impl, pos, quat, env0, n);
  });
}

float* mrs_batch_mocap_pos_device_ptr(mrs_batch* b) { return b ? mrs::batch_mocap_pos_device_ptr(b->impl) : nullptr; }
float* mrs_batch_mocap_quat_device_ptr(mrs_batch* b) { return b ? mrs::batch_mocap_quat_device_ptr(b->impl) : nullptr; }

int mrs_batch_param_dim(const mrs_batch* b, int param) {
  int dim = MRS_ERR_INVALID;
  const int rc = guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    dim = mrs::batch_param_dim(b->impl, param);
  });
  return rc == MRS_OK ? dim : rc;
}

int mrs_batch_set_param(mrs_batch* b, int param, const double* host, int env0, int n) {
  return guarded([&] {
    if (!b || !host) throw std::invalid_argument("null argument");
    mrs::batch_set_param(b->impl, param, host, env0, n);
  });
}

int mrs_batch_get_param(mrs_batch* b, int param, double* host, int env0, int n) {
  return guarded([&] {
    if (!b || !host) throw std::invalid_argument("null argument");
    mrs::batch_get_param(b->impl, param, host, env0, n);
  });
}

float* mrs_batch_param_device_ptr(mrs_batch* b, int param) {
  // (the buffer is made on first use, which can fail: NULL then, the code in mrs_last_status)
  float* p = nullptr;
  guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    p = mrs::batch_param_device_ptr(b->impl, param);
  });
  return p;
}

int mrs_batch_inertial_dim(const mrs_batch* b, int which) {
  int dim = MRS_ERR_INVALID;
  const int rc = guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    dim = mrs::batch_inertial_dim(b->impl, which);
  });
  return rc == MRS_OK ? dim : rc;
}

int mrs_batch_set_inertial(mrs_batch* b, const double* mass, const double* inertia, const double* armature,
                           int env0, int n) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_set_inertial(b->impl, mass, inertia, armature, env0, n);
  });
}

int mrs_batch_get_inertial(mrs_batch* b, double* mass, double* inertia, double* armature, int env0, int n) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_get_inertial(b->impl, mass, inertia, armature, env0, n);
  });
}

int mrs_batch_get_inertial_derived(mrs_batch* b, int env, double* body_subtreemass, double* dof_invweight0,
                                   double* body_invweight0, double* meaninertia) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_get_inertial_derived(b->impl, env, body_subtreemass, dof_invweight0, body_invweight0, meaninertia);
  });
}

int mrs_batch_step(mrs_batch* b, int n_steps) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_launch(b->impl, n_steps, false);
  });
}

int mrs_batch_forward(mrs_batch* b) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_launch(b->impl, 1, true);
  });
}

int mrs_batch_render_depth(mrs_batch* b, int cam, int env0, int n, float* host_out) {
  return guarded([&] {
    if (!b || !host_out) throw std::invalid_argument("null argument");
    mrs::batch_render_depth(b->impl, cam, env0, n, host_out, false);
  });
}

int mrs_batch_render_depth_device(mrs_batch* b, int cam, int env0, int n, float* d_out) {
  return guarded([&] {
    if (!b || !d_out) throw std::invalid_argument("null argument");
    mrs::batch_render_depth(b->impl, cam, env0, n, d_out, true);
  });
}

int mrs_batch_render_rgbd(mrs_batch* b, int cam, int env0, int n, float* host_depth, unsigned char* host_rgb) {
  return guarded([&] {
    if (!b || !host_depth || !host_rgb) throw std::invalid_argument("null argument");
    mrs::batch_render_depth(b->impl, cam, env0, n, host_depth, false, host_rgb);
  });
}

int mrs_batch_render_rgbd_device(mrs_batch* b, int cam, int env0, int n, float* d_depth, unsigned char* d_rgb) {
  return guarded([&] {
    if (!b || !d_depth || !d_rgb) throw std::invalid_argument("null argument");
    mrs::batch_render_depth(b->impl, cam, env0, n, d_depth, true, d_rgb);
  });
}

int mrs_batch_render_async(mrs_batch* b, int cam, int env0, int n, float* d_depth, unsigned char* d_rgb) {
  return guarded([&] {
    if (!b || !d_depth) throw std::invalid_argument("null argument");
    mrs::batch_render_async(b->impl, cam, env0, n, d_depth, d_rgb);
  });
}

int mrs_batch_render_wait(mrs_batch* b) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_render_wait(b->impl);
  });
}

int mrs_batch_ray_device(mrs_batch* b, const float* d_pnt, const float* d_vec, int n_rays, int flags, int frame_type,
                         int frame_id, unsigned group_mask, int bodyexclude, float* d_dist, int* d_geomid) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_ray_device(b->impl, d_pnt, d_vec, n_rays, flags, frame_type, frame_id, group_mask, bodyexclude, d_dist,
                          d_geomid);
  });
}

int mrs_batch_ray(mrs_batch* b, const double* pnt, const double* vec, int n_rays, int flags, int frame_type,
                  int frame_id, unsigned group_mask, int bodyexclude, double* dist, int* geomid, int env0, int n) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_ray(b->impl, pnt, vec, n_rays, flags, frame_type, frame_id, group_mask, bodyexclude, dist, geomid, env0,
                   n);
  });
}

int mrs_batch_get_contacts(mrs_batch* b, int env, int max, int* geom, double* dist, double* pos, double* frame) {
  int ncon = 0;
  const int rc = guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    ncon = mrs::batch_get_contacts(b->impl, env, max, geom, dist, pos, frame);
  });
  return rc == MRS_OK ? ncon : rc;
}

int mrs_batch_get_efc(mrs_batch* b, int env, int max, int* type, double* J, double* R, double* aref,
                      double* force) {
  int nefc = 0;
  const int rc = guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    nefc = mrs::batch_get_efc(b->impl, env, max, type, J, R, aref, force);
  });
  return rc == MRS_OK ? nefc : rc;
}

int mrs_batch_get_contact_forces(mrs_batch* b, int env, int max, double* force) {
  int ncon = 0;
  const int rc = guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    ncon = mrs::batch_get_contact_forces(b->impl, env, max, force);
  });
  return rc == MRS_OK ? ncon : rc;
}

float* mrs_batch_contact_wrench_device_ptr(mrs_batch* b) {
  // (the buffer is made on first use, which can fail: NULL then, the code in mrs_last_status)
  float* p = nullptr;
  guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    p = mrs::batch_contact_wrench_device_ptr(b->impl);
  });
  return p;
}

int mrs_batch_get_contact_wrench(mrs_batch* b, double* host, int env0, int n) {
  return guarded([&] {
    if (!b || !host) throw std::invalid_argument("null argument");
    mrs::batch_get_contact_wrench(b->impl, host, env0, n);
  });
}

int mrs_batch_set_jac_sites(mrs_batch* b, const int* site_ids, int n) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_set_jac_sites(b->impl, site_ids, n);
  });
}

int mrs_batch_dyn_dim(const mrs_batch* b, int which) {
  int dim = 0;
  const int rc = guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    dim = mrs::batch_dyn_dim(b->impl, which);
  });
  return rc == MRS_OK ? dim : rc;
}

float* mrs_batch_dyn_device_ptr(mrs_batch* b, int which) {
  // (NULL with MRS_OK in mrs_last_status: a site output with no site selected; NULL otherwise: the error)
  float* p = nullptr;
  guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    p = mrs::batch_dyn_device_ptr(b->impl, which);
  });
  return p;
}

int mrs_batch_get_dyn(mrs_batch* b, int which, double* host, int env0, int n) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_get_dyn(b->impl, which, host, env0, n);
  });
}

int mrs_batch_get_field_device(mrs_batch* b, int field, float* d_out, int env0, int n) {
  return guarded([&] {
    if (!b || !d_out) throw std::invalid_argument("null argument");
    mrs::batch_get_field_device(b->impl, field, d_out, env0, n);
  });
}

int mrs_batch_sync(mrs_batch* b) {
  return guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    mrs::batch_sync(b->impl);
  });
}

int mrs_batch_set_timing(mrs_batch* b, int mask) {
  return guarded([&] {
    if (!b || mask < 0 || mask > 3) throw std::invalid_argument("timing mask must be 0..3");
    mrs::batch_set_timing(b->impl, mask);
  });
}

double mrs_batch_last_kernel_ms(mrs_batch* b, int kind) {
  double ms = -1;
  guarded([&] {
    if (!b) throw std::invalid_argument("null batch");
    ms = mrs::batch_last_kernel_ms(b->impl, kind);
  });
  return ms;
}

int mrs_debug_phase_cycles(double* out, int n, int reset) {
  if (!out || n < 0) return MRS_ERR_INVALID;
  return mrs::phase_cycles(out, n, reset != 0);
}

int mrs_debug_batch_layout(const mrs_batch* b, int* out, int n) {
  if (!b || !out || n < 0) return MRS_ERR_INVALID;
  return mrs::batch_layout(b->impl, out, n);
}

int mrs_debug_plan_layout(const mrs_model* m, int n_envs, int cu_count, int max_contacts, int* out, int n) {
  int k = 0;
  const int rc = guarded([&] {
    if (!m || !out || n < 0) throw std::invalid_argument("null model or output");
    if (n_envs < 1) throw std::invalid_argument("n_envs must be positive");
    k = mrs::plan_layout(m->m, n_envs, cu_count, max_contacts, out, n);
  });
  return rc == MRS_OK ? k : rc;
}

int mrs_debug_pairs(const mrs_model* m, int* geom, int max, int* pruned) {
  int k = 0;
  const int rc = guarded([&] {
    if (!m) throw std::invalid_argument("null model");
    if (max < 0 || (max > 0 && !geom)) throw std::invalid_argument("null output or negative capacity");
    k = mrs::walked_pairs(m->m, geom, max, pruned);
  });
  return rc == MRS_OK ? k : rc;
}

int mrs_debug_table_image(const mrs_model* m, int n_envs, int cu_count, int max_contacts, float* image, int max,
                          int* offsets, int n_off) {
  int k = 0;
  const int rc = guarded([&] {
    if (!m) throw std::invalid_argument("null model");
    if (n_envs < 1) throw std::invalid_argument("n_envs must be positive");
    if (max < 0 || (max > 0 && !image) || n_off < 0 || (n_off > 0 && !offsets))
      throw std::invalid_argument("null output or negative capacity");
    k = mrs::table_image(m->m, n_envs, cu_count, max_contacts, image, max, offsets, n_off);
  });
  return rc == MRS_OK ? k : rc;
}

int mrs_debug_staged_table(const mrs_model* m, int max_contacts, int which, float* out, int max) {
  int k = 0;
  const int rc = guarded([&] {
    if (!m) throw std::invalid_argument("null model");
    if (max < 0 || (max > 0 && !out)) throw std::invalid_argument("null output or negative capacity");
    k = mrs::staged_table(m->m, max_contacts, which, out, max);
  });
  return rc == MRS_OK ? k : rc;
}

int mrs_debug_render_plan(const mrs_model* m, int cam, int n_frames, int max_lds, long long* out, int n) {
  int k = 0;
  const int rc = guarded([&] {
    if (!m || !out || n < 0) throw std::invalid_argument("null model or output");
    if (n_frames < 1) throw std::invalid_argument("n_frames must be positive");
    if (max_lds < 0) throw std::invalid_argument("negative LDS limit");
    k = mrs::render_plan(m->m, cam, n_frames, max_lds, out, n);
  });
  return rc == MRS_OK ? k : rc;
}

int mrs_debug_ray_filter(const mrs_model* m, unsigned group_mask, int flags, int bodyexclude, int* out, int max) {
  int k = 0;
  const int rc = guarded([&] {
    if (!m) throw std::invalid_argument("null model");
    if (max < 0 || (max > 0 && !out)) throw std::invalid_argument("null output or negative capacity");
    mrs::check_ray_filter(m->m, flags, bodyexclude);
    const std::vector<mrs::RayGeom> list =
        mrs::build_ray_filter(m->m, group_mask, (flags & MRS_RAY_NO_STATIC) != 0, bodyexclude);
    k = static_cast<int>(list.size());
    for (int i = 0; i < k && i < max; ++i) out[i] = list[i].id;
  });
  return rc == MRS_OK ? k : rc;
}

}  // extern "C"
