// Batch of environments resident on one GPU: model upload, the per-env arrays, state transfer, resets,
// exports and the step/forward launches.  Host side of the C ABI in include/mrs.h; frames and ray
// queries are render.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/mrs.h"
#include "../mjcf/model.h"
#include "batch.h"
#include "batch_impl.h"
#include "devmodel.h"
#include "devtables.h"
#include "plan.h"
#include "lit.h"
#include "start_rows.h"

namespace mrs {

hipError_t launch_step(const DevModel* d_model, int lds_floats, int shared_floats, const DevState& st, int n_envs,
                       int n_steps, bool forward_only, int group, bool primal, bool ext, bool params, bool dyn,
                       hipStream_t stream);

namespace {

// ------------------------------------------------------------------ masked reset kernel
// One 16-lane group per env.  The group of an env whose mask byte is set copies the env's start
// state (a row of the model's table -- row 0 qpos0, row 1 + k keyframe k -- or of the batch's pool)
// into the state fields and clears what batch_reset clears; the group of an unmasked env returns
// before its first store, so such an env's rows are never written.  The tables, the pool, the mask
// and the key array are only read.
struct ResetArgs {
  const unsigned char* mask;  // [n]
  const int* keys;            // [n] start indices, or null: `key` for every env
  int key, n, nq, nv, nu, na, nx, nkey, npool, nmocap;
  const float *tab_qpos, *tab_qvel, *tab_ctrl, *tab_act;  // [1 + nkey][nq | nv | nu | na]
  const float *tab_mpos, *tab_mquat;                      // [1 + nkey][3 nmocap | 4 nmocap]
  const double* tab_time;                       // [1 + nkey]
  const float *pool_qpos, *pool_qvel;           // [npool][nq | nv]
  float *qpos, *qvel, *ctrl, *qfrc_applied, *qacc_ws, *xfrc;  // ctrl / xfrc null: not written
  float* act;  // [n][na] (null when na == 0)
  float *mocap_pos, *mocap_quat;  // [n][nmocap][3 | 4] (null when nmocap == 0)
  double* time;
  int* warning;
};
__global__ __launch_bounds__(256) void reset_masked_kernel(const ResetArgs a) {
  const size_t e = (static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x) >> 4;
  const int lane = threadIdx.x & 15;
  if (e >= static_cast<size_t>(a.n) || !a.mask[e]) return;
  int k = a.keys ? a.keys[e] : a.key;
  if (k < -1 || k >= a.nkey + a.npool) k = -1;  // (an index outside the table and the pool: qpos0)
  const float *sq, *sv, *sc = nullptr, *sa = nullptr;  // (a pool row has no ctrl and no act: zeros)
  double t = 0;
  if (k < a.nkey) {
    const size_t row = static_cast<size_t>(k + 1);
    sq = a.tab_qpos + row * a.nq;
    sv = a.tab_qvel + row * a.nv;
    sc = a.tab_ctrl + row * a.nu;
    sa = a.tab_act + row * a.na;
    t = a.tab_time[row];
  } else {
    const size_t row = static_cast<size_t>(k - a.nkey);
    sq = a.pool_qpos + row * a.nq;
    sv = a.pool_qvel + row * a.nv;
  }
  for (int i = lane; i < a.nq; i += 16) a.qpos[e * a.nq + i] = sq[i];
  for (int i = lane; i < a.nv; i += 16) {
    a.qvel[e * a.nv + i] = sv[i];
    a.qfrc_applied[e * a.nv + i] = 0;
    a.qacc_ws[e * a.nv + i] = 0;
  }
  if (a.ctrl)
    for (int i = lane; i < a.nu; i += 16) a.ctrl[e * a.nu + i] = sc ? sc[i] : 0.0f;
  if (a.xfrc)
    for (int i = lane; i < a.nx; i += 16) a.xfrc[e * a.nx + i] = 0;
  for (int i = lane; i < a.na; i += 16) a.act[e * a.na + i] = sa ? sa[i] : 0.0f;
  {  // mocap poses: the keyframe's, else (qpos0 and pool rows) the bodies' pos / quat in row 0
    const size_t row = k < a.nkey ? static_cast<size_t>(k + 1) : 0;
    for (int i = lane; i < 3 * a.nmocap; i += 16) a.mocap_pos[e * 3 * a.nmocap + i] = a.tab_mpos[row * 3 * a.nmocap + i];
    for (int i = lane; i < 4 * a.nmocap; i += 16) a.mocap_quat[e * 4 * a.nmocap + i] = a.tab_mquat[row * 4 * a.nmocap + i];
  }
  if (lane < 4) a.warning[e * 4 + lane] = 0;
  if (lane == 4) a.time[e] = t;
}

static_assert(kRlitHead == kLitHead && kRlitLight == kLitLight && kRlitMat == kLitMat && kRlitTex == kLitTex &&
                  kRlitMaxLights == kLitMaxLights,
              "devtables.h restates lit.h's block layout");
// (the test suite of the revision before renderplan.h reads this limit's definition out of this file)
static_assert(kMaxRenderGeoms == 256, "renderplan.h: constexpr int kMaxRenderGeoms = 256;");

// ---- the per-env arrays: every array [n_envs][dim] that the host reads or writes by env range.  One
// row of env_array() describes one array -- where the kernels read its pointer (a member of DevState or
// DevModel: the table points at that slot and keeps no copy), its elements per env, their type and
// when the array is made -- and creation, the row copies and the accessors below all go by it.
// Ids: the MRS_FIELD_* values, then
enum { kArrAct = MRS_FIELD_COUNT, kArrMocapPos, kArrMocapQuat, kArrParam0, kArrInertial = kArrParam0 + MRS_PARAM_COUNT,
       kArrContactWrench, kArrDyn0, kArrCount = kArrDyn0 + MRS_DYNOUT_COUNT };
static_assert(MRS_DYNOUT_COUNT == 4 && MRS_MAX_JAC_SITES == 16 && kDynBias == 1 << MRS_DYNOUT_QFRC_BIAS &&
                  kDynM == 1 << MRS_DYNOUT_MASS_MATRIX && kDynJac == 1 << MRS_DYNOUT_SITE_JAC &&
                  kDynPose == 1 << MRS_DYNOUT_SITE_POSE,
              "DevModel::dyn_out / dyn_site / dyn_mask follow mrs.h");

struct EnvArray {
  enum Type { F32, I32, F64 } type;
  // AT_CREATE: with the batch, a buffer even when dim == 0; IF_DIM: with the batch, null when dim == 0;
  // ON_USE: null until first used (ensure_xfrc, ensure_param, ensure_inertial, ensure_contact_wrench,
  // ensure_dyn)
  enum Made { AT_CREATE, IF_DIM, ON_USE } made;
  int dim;     // elements per env; -1: no such array
  void* ptr;   // the array as its slot holds it now (null: not made)
  void* slot;  // the pointer member itself
  size_t width() const { return type == F64 ? sizeof(double) : 4; }
  // (the slots are float*, const float*, int* and double* members: written as the pointer's bytes)
  void bind(void* p) const { std::memcpy(slot, &p, sizeof p); }
};

template <class T>
EnvArray env_array_at(T*& slot, int dim, EnvArray::Made made = EnvArray::AT_CREATE) {
  using U = typename std::remove_const<T>::type;
  return {std::is_same<U, double>::value ? EnvArray::F64 : std::is_same<U, int>::value ? EnvArray::I32 : EnvArray::F32,
          made, dim, const_cast<U*>(slot), &slot};
}

// floats per env of dynamics output `which` (MRS_DYNOUT_*); the site outputs' follow the selection
int dyn_dim(const BatchImpl& b, int which) {
  const Model& m = *b.model;
  switch (which) {
    case MRS_DYNOUT_QFRC_BIAS: return m.nv;
    case MRS_DYNOUT_MASS_MATRIX: return m.nv * m.nv;
    case MRS_DYNOUT_SITE_JAC: return b.dm.dyn_nsel * 6 * m.nv;
    case MRS_DYNOUT_SITE_POSE: return b.dm.dyn_nsel * 12;
  }
  throw std::invalid_argument("unknown dynamics output");
}

EnvArray env_array(BatchImpl& b, int id) {
  const Model& m = *b.model;
  DevState& s = b.st;
  DevModel& d = b.dm;
  switch (id) {
    case MRS_FIELD_QPOS: return env_array_at(s.qpos, m.nq);
    case MRS_FIELD_QVEL: return env_array_at(s.qvel, m.nv);
    case MRS_FIELD_CTRL: return env_array_at(s.ctrl, m.nu);
    case MRS_FIELD_QFRC_APPLIED: return env_array_at(s.qfrc_applied, m.nv);
    case MRS_FIELD_QACC_WARMSTART: return env_array_at(s.qacc_ws, m.nv);
    case MRS_FIELD_QACC: return env_array_at(s.qacc, m.nv);
    case MRS_FIELD_QFRC_ACTUATOR: return env_array_at(s.qfrc_act, m.nv);
    case MRS_FIELD_SENSORDATA: return env_array_at(s.sensordata, m.nsensordata);
    case MRS_FIELD_TIME: return env_array_at(s.time, 1);
    case MRS_FIELD_WARNING: return env_array_at(s.warning, 4);
    case MRS_FIELD_NCON: return env_array_at(s.ncon, 1);
    case MRS_FIELD_SOLVER_NITER: return env_array_at(s.niter, 1);
    case MRS_FIELD_XFRC_APPLIED: return env_array_at(s.xfrc_applied, 6 * m.nbody, EnvArray::ON_USE);
    case kArrAct: return env_array_at(s.act, m.na, EnvArray::IF_DIM);
    case kArrMocapPos: return env_array_at(d.mocap_pos, 3 * m.nmocap, EnvArray::IF_DIM);
    case kArrMocapQuat: return env_array_at(d.mocap_quat, 4 * m.nmocap, EnvArray::IF_DIM);
    case kArrParam0 + MRS_PARAM_ACT_GAINPRM: return env_array_at(d.prm_gain, 3 * m.nu, EnvArray::ON_USE);
    case kArrParam0 + MRS_PARAM_ACT_BIASPRM: return env_array_at(d.prm_bias, 3 * m.nu, EnvArray::ON_USE);
    case kArrParam0 + MRS_PARAM_DOF_DAMPING: return env_array_at(d.prm_damp, m.nv, EnvArray::ON_USE);
    case kArrParam0 + MRS_PARAM_GEOM_FRICTION: return env_array_at(d.prm_fric, m.ngeom, EnvArray::ON_USE);
    case kArrInertial: return env_array_at(d.prm_inr, inertial_layout(m).dim, EnvArray::ON_USE);
    case kArrContactWrench: return env_array_at(d.cfrc_contact, 6 * m.nbody, EnvArray::ON_USE);
    case kArrDyn0 + MRS_DYNOUT_QFRC_BIAS:
    case kArrDyn0 + MRS_DYNOUT_MASS_MATRIX:
    case kArrDyn0 + MRS_DYNOUT_SITE_JAC:
    case kArrDyn0 + MRS_DYNOUT_SITE_POSE: return env_array_at(d.dyn_out[id - kArrDyn0], dyn_dim(b, id - kArrDyn0), EnvArray::ON_USE);
  }
  return {EnvArray::F32, EnvArray::ON_USE, -1, nullptr, nullptr};
}
EnvArray field_array(BatchImpl& b, int field) {
  if (field < 0 || field >= MRS_FIELD_COUNT) throw std::invalid_argument("unknown field");
  return env_array(b, field);
}
EnvArray param_array(BatchImpl& b, int param) {
  if (param < 0 || param >= MRS_PARAM_COUNT) throw std::invalid_argument("unknown model parameter");
  return env_array(b, kArrParam0 + param);
}

// the arrays made with the batch, zero-filled.  Called before build_devmodel: the mocap poses' pointers
// travel in the model block it uploads
void make_env_arrays(BatchImpl& b) {
  for (int id = 0; id < kArrCount; ++id) {
    const EnvArray a = env_array(b, id);
    if (a.made == EnvArray::ON_USE || (a.made == EnvArray::IF_DIM && a.dim == 0)) continue;
    a.bind(dalloc(b, static_cast<size_t>(b.n) * std::max(1, a.dim) * a.width()));
  }
}

// The device part of batch creation: the model's tables (devtables.h) and the launch plan (plan.h) are
// host values; this uploads the two blocks, points DevModel's tables into them, allocates the static
// ray hits and uploads DevModel.  The arrays make_env_arrays bound to DevModel members stay bound: the
// env-array table says which they are
void build_devmodel(BatchImpl& b, int max_con_req, const Overrides& o) {
  const Model& m = *b.model;
  const DevTables T = build_tables(m, max_con_req, o);
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b.device) != hipSuccess) cus = 0;
  const Plan p = choose_plan(m, T, b.n, cus, o);
  void* made[kArrCount];
  for (int id = 0; id < kArrCount; ++id) made[id] = env_array(b, id).ptr;
  b.dm = p.dm;
  for (int id = 0; id < kArrCount; ++id)
    if (made[id]) env_array(b, id).bind(made[id]);
  b.dblock_f = dalloc(b, T.f.size() * sizeof(float));
  b.dblock_i = dalloc(b, T.i.size() * sizeof(int));
  HIP_CHECK(hipMemcpyAsync(b.dblock_f, T.f.data(), T.f.size() * sizeof(float), hipMemcpyHostToDevice, b.stream));
  HIP_CHECK(hipMemcpyAsync(b.dblock_i, T.i.data(), T.i.size() * sizeof(int), hipMemcpyHostToDevice, b.stream));
  T.patch(b.dm, static_cast<const float*>(b.dblock_f), static_cast<const int*>(b.dblock_i));
  // the workgroup-shared tables as one image (DevModel::shr_image), which the launches copy; the static
  // ray hits live inside it, where the producer pass writes them.  No later call writes a staged table
  // (set_param / set_inertial fill per-env rows), so the image stays what it is here
  const std::vector<float> image = o.no_table_image ? std::vector<float>() : pack_shared_image(T, b.dm);
  float* d_image = nullptr;
  if (!o.no_table_image) {
    d_image = static_cast<float*>(dalloc(b, image.size() * sizeof(float)));
    if (!image.empty())
      HIP_CHECK(hipMemcpyAsync(d_image, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice, b.stream));
    b.dm.shr_image = d_image;
  }
  b.dm.rf_static = !b.dm.rf_mode ? nullptr
                   : d_image     ? d_image + b.dm.shr_rfst
                                 : static_cast<float*>(dalloc(b, std::max(1, b.dm.nrf) * sizeof(float)));
  b.group = p.group; b.g16_one_wg = p.g16_one_wg; b.wpb16 = p.wpb16; b.helpers = p.helpers; b.ext = p.ext;
  b.pair_g1 = T.pair_g1; b.pair_g2 = T.pair_g2; b.pair_dim = T.pair_dim; b.pair_mu = T.pair_mu;
  b.pairs_pruned = T.pairs_pruned;
  b.d_dm = static_cast<DevModel*>(dalloc(b, sizeof(DevModel)));
  HIP_CHECK(hipMemcpyAsync(b.d_dm, &b.dm, sizeof(DevModel), hipMemcpyHostToDevice, b.stream));
  HIP_CHECK(hipStreamSynchronize(b.stream));  // (the host blocks of T are read until here)
}

// ---- the two row copies every host accessor goes through.  Each part is an array and the host's fp64
// rows [n][dim] for envs [env0, env0 + n); a part with a null host pointer or no elements is skipped.
// Every part's copy is queued on the batch stream, then the stream is synchronised once (not at all if
// nothing was queued).  The caller has checked the env range and made the arrays
struct RowStage { double* host; std::vector<float> f; std::vector<int> i; };

// fp64 host rows into the arrays: static_cast to float (F32) or int (I32), as they are (F64)
void rows_to_device(BatchImpl& b, int env0, int n, std::initializer_list<std::pair<EnvArray, const double*>> parts) {
  HIP_CHECK(hipSetDevice(b.device));
  std::deque<RowStage> stage;  // the converted rows, alive until the synchronise
  bool queued = false;
  for (const auto& part : parts) {
    const EnvArray& a = part.first;
    const double* host = part.second;
    const size_t cnt = static_cast<size_t>(n) * std::max(0, a.dim);
    if (!host || cnt == 0) continue;
    const void* src = host;
    if (a.type == EnvArray::F32) {
      std::vector<float>& t = stage.emplace_back().f;
      t.resize(cnt);
      for (size_t k = 0; k < cnt; ++k) t[k] = static_cast<float>(host[k]);
      src = t.data();
    } else if (a.type == EnvArray::I32) {
      std::vector<int>& t = stage.emplace_back().i;
      t.resize(cnt);
      for (size_t k = 0; k < cnt; ++k) t[k] = static_cast<int>(host[k]);
      src = t.data();
    }
    HIP_CHECK(hipMemcpyAsync(static_cast<char*>(a.ptr) + static_cast<size_t>(env0) * a.dim * a.width(), src,
                             cnt * a.width(), hipMemcpyHostToDevice, b.stream));
    queued = true;
  }
  if (queued) HIP_CHECK(hipStreamSynchronize(b.stream));
}

// the arrays' rows into fp64 host rows
void rows_to_host(BatchImpl& b, int env0, int n, std::initializer_list<std::pair<EnvArray, double*>> parts) {
  HIP_CHECK(hipSetDevice(b.device));
  std::deque<RowStage> stage;  // the fp32 / int32 rows, widened after the synchronise
  bool queued = false;
  for (const auto& part : parts) {
    const EnvArray& a = part.first;
    const size_t cnt = static_cast<size_t>(n) * std::max(0, a.dim);
    if (!part.second || cnt == 0) continue;
    void* dst = part.second;
    if (a.type != EnvArray::F64) {
      RowStage& t = stage.emplace_back();
      t.host = part.second;
      if (a.type == EnvArray::F32) { t.f.resize(cnt); dst = t.f.data(); } else { t.i.resize(cnt); dst = t.i.data(); }
    }
    HIP_CHECK(hipMemcpyAsync(dst, static_cast<const char*>(a.ptr) + static_cast<size_t>(env0) * a.dim * a.width(),
                             cnt * a.width(), hipMemcpyDeviceToHost, b.stream));
    queued = true;
  }
  if (queued) HIP_CHECK(hipStreamSynchronize(b.stream));
  for (const RowStage& t : stage) {
    std::copy(t.f.begin(), t.f.end(), t.host);
    std::copy(t.i.begin(), t.i.end(), t.host);
  }
}

// the per-body wrench buffer [n][nbody][6], made and zero-filled when the field is first used; from
// then on the step kernel reads it (DevState::xfrc_applied, and DevModel::xfrc for the phases).  The
// earlier launches have finished before the model block changes
float* ensure_xfrc(BatchImpl& b) {
  if (!b.st.xfrc_applied) {
    HIP_CHECK(hipSetDevice(b.device));
    float* p = static_cast<float*>(dalloc(b, static_cast<size_t>(b.n) * 6 * b.model->nbody * sizeof(float)));
    HIP_CHECK(hipStreamSynchronize(b.stream));
    b.dm.xfrc = p;
    HIP_CHECK(hipMemcpy(b.d_dm, &b.dm, sizeof(DevModel), hipMemcpyHostToDevice));
    b.st.xfrc_applied = p;
  }
  return b.st.xfrc_applied;
}
// a parameter's buffer [n][dim], made when the parameter is first used and filled with the model's own
// values for every env; from then on the step kernel reads it (DevModel::prm_*).  Like ensure_xfrc:
// the earlier launches have finished before the model block changes.  Null when dim == 0
float* ensure_param(BatchImpl& b, int param) {
  const EnvArray a = param_array(b, param);
  if (a.dim == 0 || a.ptr) return static_cast<float*>(a.ptr);
  HIP_CHECK(hipSetDevice(b.device));
  const std::vector<float> row = param_model_row(*b.model, param);
  std::vector<float> all(static_cast<size_t>(b.n) * a.dim);
  for (int e = 0; e < b.n; ++e) std::copy(row.begin(), row.end(), all.begin() + static_cast<size_t>(e) * a.dim);
  float* p = static_cast<float*>(dalloc(b, all.size() * sizeof(float)));
  HIP_CHECK(hipStreamSynchronize(b.stream));
  HIP_CHECK(hipMemcpy(p, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
  a.bind(p);
  b.dm.prm_mask |= 1 << param;
  HIP_CHECK(hipMemcpy(b.d_dm, &b.dm, sizeof(DevModel), hipMemcpyHostToDevice));
  return p;
}

// the inertial rows [n][dim] (start_rows.h inertial_layout: mass, inertia, armature and the constants
// derived from them), made on the first set_inertial and filled with the model's own row for every env;
// from then on the step kernel reads them (DevModel::prm_inr, bit kPrmInr of prm_mask).  Like ensure_param
float* ensure_inertial(BatchImpl& b) {
  const EnvArray a = env_array(b, kArrInertial);
  if (a.ptr) return static_cast<float*>(a.ptr);
  HIP_CHECK(hipSetDevice(b.device));
  const Model& m = *b.model;
  const std::vector<float> row = inertial_model_row(m, inertial_layout(m));
  std::vector<float> all(static_cast<size_t>(b.n) * a.dim);
  for (int e = 0; e < b.n; ++e) std::copy(row.begin(), row.end(), all.begin() + static_cast<size_t>(e) * a.dim);
  float* p = static_cast<float*>(dalloc(b, all.size() * sizeof(float)));
  HIP_CHECK(hipStreamSynchronize(b.stream));
  HIP_CHECK(hipMemcpy(p, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
  a.bind(p);
  b.dm.inr_dim = a.dim;
  b.dm.prm_mask |= kPrmInr;
  HIP_CHECK(hipMemcpy(b.d_dm, &b.dm, sizeof(DevModel), hipMemcpyHostToDevice));
  // the host's fp64 copy of the inputs starts from the model's too
  const size_t hd = 4 * static_cast<size_t>(m.nbody) + m.nv;
  b.inr_host.resize(static_cast<size_t>(b.n) * hd);
  for (int e = 0; e < b.n; ++e) {
    double* h = b.inr_host.data() + e * hd;
    std::copy(m.body_mass.begin(), m.body_mass.end(), h);
    std::copy(m.body_inertia.begin(), m.body_inertia.end(), h + m.nbody);
    std::copy(m.dof_armature.begin(), m.dof_armature.end(), h + 4 * m.nbody);
  }
  return p;
}

// the net contact wrench per body [n][nbody][6] (an output; DevModel::cfrc_contact), made and zero-filled
// when it is first asked for; from then on every launch's last forward pass writes it (step.hip
// contact_wrench_out).  Like ensure_xfrc: the earlier launches have finished before the model block
// changes.  No reset touches it, as none touches qacc or sensordata
float* ensure_contact_wrench(BatchImpl& b) {
  const EnvArray a = env_array(b, kArrContactWrench);
  if (a.ptr) return static_cast<float*>(a.ptr);
  HIP_CHECK(hipSetDevice(b.device));
  float* p = static_cast<float*>(dalloc(b, static_cast<size_t>(b.n) * a.dim * sizeof(float)));
  HIP_CHECK(hipStreamSynchronize(b.stream));
  a.bind(p);
  HIP_CHECK(hipMemcpy(b.d_dm, &b.dm, sizeof(DevModel), hipMemcpyHostToDevice));
  return p;
}

// dynamics output `which` [n][dim] (DevModel::dyn_out, its bit of dyn_mask), made and zero-filled when it is
// first asked for; from then on every launch's last forward pass writes it (step.hip dyn_outputs).  Like
// ensure_contact_wrench.  A site output with no site selected has no buffer (null) but counts as asked for:
// batch_set_jac_sites makes it with the selection
float* ensure_dyn(BatchImpl& b, int which) {
  const int dim = dyn_dim(b, which);  // (throws for an unknown output)
  const EnvArray a = env_array(b, kArrDyn0 + which);
  b.dyn_asked |= 1 << which;
  if (a.ptr || dim == 0) return static_cast<float*>(a.ptr);
  HIP_CHECK(hipSetDevice(b.device));
  float* p = static_cast<float*>(dalloc(b, static_cast<size_t>(b.n) * dim * sizeof(float)));
  HIP_CHECK(hipStreamSynchronize(b.stream));
  a.bind(p);
  b.dm.dyn_mask |= 1 << which;
  HIP_CHECK(hipMemcpy(b.d_dm, &b.dm, sizeof(DevModel), hipMemcpyHostToDevice));
  return p;
}

// the model's start states as the masked reset reads them: b.start (start_rows.h) in one device table
void upload_start_table(BatchImpl& b) {
  auto put = [&](const void* src, size_t bytes) {
    void* dst = dalloc(b, bytes);
    if (bytes) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, b.stream));
    return dst;
  };
  auto putf = [&](const std::vector<float>& v) { return static_cast<float*>(put(v.data(), v.size() * sizeof(float))); };
  const StartRows& s = b.start;
  b.tab_qpos = putf(s.qpos);
  b.tab_qvel = putf(s.qvel);
  b.tab_ctrl = putf(s.ctrl);
  b.tab_act = putf(s.act);
  b.tab_mpos = putf(s.mpos);
  b.tab_mquat = putf(s.mquat);
  b.tab_time = static_cast<double*>(put(s.time.data(), s.time.size() * sizeof(double)));
  HIP_CHECK(hipStreamSynchronize(b.stream));
}

// room for `count` pool rows.  A pool that grows past its capacity, or is freed (count 0), waits for
// the queued work that may still read the old rows before releasing them; otherwise nothing waits
void reserve_pool(BatchImpl& b, int count) {
  if (count < 0) throw std::invalid_argument("negative start-state count");
  HIP_CHECK(hipSetDevice(b.device));
  if (count != 0 && count <= b.pool_cap) return;
  if (b.pool_qpos || b.pool_qvel) {
    HIP_CHECK(hipStreamSynchronize(b.stream));
    HIP_CHECK(hipFree(b.pool_qpos));
    b.pool_qpos = nullptr;
    HIP_CHECK(hipFree(b.pool_qvel));
    b.pool_qvel = nullptr;
    b.pool_cap = b.pool_n = 0;
  }
  if (count == 0) return;
  const Model& m = *b.model;
  HIP_CHECK(hipMalloc(&b.pool_qpos, static_cast<size_t>(count) * std::max(1, m.nq) * sizeof(float)));
  HIP_CHECK(hipMalloc(&b.pool_qvel, static_cast<size_t>(count) * std::max(1, m.nv) * sizeof(float)));
  b.pool_cap = count;
}

}  // namespace

BatchImpl* batch_create(const Model* model, int n_envs, int device, int max_contacts) {
  if (n_envs < 1) throw std::invalid_argument("n_envs must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw DeviceError("no HIP device available");
  if (device < 0 || device >= ndev) throw std::invalid_argument("device index out of range");
  HIP_CHECK(hipSetDevice(device));
  auto* b = new BatchImpl();
  try {
    b->model = model;
    b->n = n_envs;
    b->device = device;
    HIP_CHECK(hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking));
    b->stream = b->own_stream;
    for (int k = 0; k < 2; ++k) { HIP_CHECK(hipEventCreate(&b->ev0[k])); HIP_CHECK(hipEventCreate(&b->ev1[k])); }
    b->start = start_rows(*model);
    make_env_arrays(*b);
    const Overrides o = read_overrides();  // (every batch reads them anew)
    build_devmodel(*b, max_contacts, o);
    const Model& m = *model;
    const size_t n = static_cast<size_t>(n_envs);
    // padded to whole workgroups of the chosen group width: idle groups use it
    const size_t epb = static_cast<size_t>(envs_per_block(b->group, b->wpb16));
    const size_t n_pad = (static_cast<size_t>(n) + epb - 1) / epb * epb;
    // env spread (opt-in, MRS_SPREAD=<shift>): 2^shift lane groups per env, the extra ones mirroring
    // the first, so a small batch occupies more waves.  Measured slower (round 5, same box: C4 18.2
    // vs 22.9 M env-steps/s at shift 2, C2 147 vs 156 M at shift 1): the mirrors' issue slots cost
    // more than the latency they hide, so it is off by default
    const int shift = o.spread;
    const size_t n_virt = ((static_cast<size_t>(n) << shift) + epb - 1) / epb * epb;
    b->st.spread_shift = shift;
    b->st.wpb16 = b->wpb16;
    b->st.ray_helpers = b->helpers;  // (build_devmodel)
    b->st.scr_mirror = static_cast<int>(n_pad);
    b->st.scratch = static_cast<float*>(dalloc(*b, (n_pad + (shift ? n_virt : 0)) * b->S.total * sizeof(float)));
    b->st.geom_xpos = static_cast<float*>(dalloc(*b, n * std::max(1, m.ngeom) * 3 * sizeof(float)));
    b->st.geom_xmat = static_cast<float*>(dalloc(*b, n * std::max(1, m.ngeom) * 9 * sizeof(float)));
    b->st.cam_xpos = static_cast<float*>(dalloc(*b, n * std::max(1, m.ncam) * 3 * sizeof(float)));
    b->st.cam_xmat = static_cast<float*>(dalloc(*b, n * std::max(1, m.ncam) * 9 * sizeof(float)));
    batch_reset(b, -1, 0, n_envs);
    upload_start_table(*b);
    if (b->dm.rf_mode == 2) {
      // static ray hits: one forward-only pass of env 0 with the producer's model copy
      DevModel prod = b->dm;
      prod.rf_mode = 1;
      prod.rf_sweep = 0;  // (the producer pass is a block pass over the static geoms)
      DevModel* d_prod = static_cast<DevModel*>(dalloc(*b, sizeof(DevModel)));
      HIP_CHECK(hipMemcpyAsync(d_prod, &prod, sizeof(DevModel), hipMemcpyHostToDevice, b->stream));
      HIP_CHECK(launch_step(d_prod, b->L.total, b->dm.shr_total, b->st, 1, 1, true, b->group, false, b->ext, b->dm.nact_site > 0, false, b->stream));
      HIP_CHECK(hipStreamSynchronize(b->stream));
    }
    batch_launch(b, 1, true);  // mj_forward after load (src/mujoco_system_interface.cpp:741)
    HIP_CHECK(hipStreamSynchronize(b->stream));
  } catch (...) {
    batch_free(b);
    throw;
  }
  return b;
}

void batch_free(BatchImpl* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->rstream) (void)hipStreamSynchronize(b->rstream);
  for (void* p : b->allocs) (void)hipFree(p);
  if (b->pool_qpos) (void)hipFree(b->pool_qpos);
  if (b->pool_qvel) (void)hipFree(b->pool_qvel);
  render_free(*b);
  for (int k = 0; k < 2; ++k) {
    if (b->ev0[k]) (void)hipEventDestroy(b->ev0[k]);
    if (b->ev1[k]) (void)hipEventDestroy(b->ev1[k]);
  }
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
}

int batch_num_envs(const BatchImpl* b) { return b->n; }

int batch_layout(const BatchImpl* b, int* out, int n) {
  int v[22];
  plan_layout_values(b->dm, b->group, b->g16_one_wg, b->wpb16, b->helpers, v);  // (the first 16: plan.h)
  v[16] = b->dm.cfrc_contact ? 1 : 0;
  v[17] = b->dm.dyn_mask;
  v[18] = b->dm.solve_fuse;
  v[19] = b->dm.npair;
  v[20] = b->pairs_pruned;
  v[21] = b->dm.shr_image.p ? 1 : 0;
  int k = 0;
  for (; k < n && k < 22; ++k) out[k] = v[k];
  return k;
}

// mrs_debug_pairs: the pairs a batch of this model walks, as build_tables chooses them; touches no device
int walked_pairs(const Model& m, int* geom, int max, int* pruned) {
  const DevTables T = build_tables(m, 0, read_overrides());
  const int k = static_cast<int>(T.pair_g1.size());
  for (int q = 0; q < k && q < max; ++q) { geom[2 * q] = T.pair_g1[q]; geom[2 * q + 1] = T.pair_g2[q]; }
  if (pruned) *pruned = T.pairs_pruned;
  return k;
}

// mrs_debug_table_image: the packed image of the workgroup-shared tables as a batch of this plan would
// upload it, and the plan's shr_* offsets; touches no device
int table_image(const Model& m, int n_envs, int cu_count, int max_contacts, float* image, int max, int* offsets, int n_off) {
  const Overrides o = read_overrides();
  const DevTables T = build_tables(m, max_contacts, o);
  const Plan p = choose_plan(m, T, n_envs, cu_count, o);
  const DevModel& d = p.dm;
  const std::vector<float> img = pack_shared_image(T, d);
  for (int k = 0; k < max && k < static_cast<int>(img.size()); ++k) image[k] = img[k];
  const int off[18] = {d.shr_rf, d.shr_rfst, d.shr_blk, d.shr_sens, d.shr_fric, d.shr_lim, d.shr_act, d.shr_dof, d.shr_body,
                       d.shr_mpair, d.shr_jump, d.shr_kbody, d.shr_kjnt, d.shr_kgeom, d.shr_flag, d.shr_total, d.blocked,
                       shared_image_floats(d)};
  for (int k = 0; k < n_off && k < 18; ++k) offsets[k] = off[k];
  return static_cast<int>(img.size());
}

// mrs_debug_staged_table: one of the tables the launches stage, as build_tables packs it (jump: int bits)
int staged_table(const Model& m, int max_contacts, int which, float* out, int max) {
  using D = DevModel;
  const DevTables T = build_tables(m, max_contacts, read_overrides());
  CPtr<float> D::*const ftab[14] = {&D::rgeom, &D::rfray, &D::rfblk, &D::sensrec, &D::fricrec, &D::limrec, &D::actrec,
                                    &D::dofrec, &D::bodytab, &D::mpairtab, nullptr, &D::kinbody, &D::kinjnt, &D::kingeom};
  if (which < 0 || which >= 14) throw std::invalid_argument("unknown staged table");
  if (!ftab[which]) {
    for (const auto& s : T.islot)
      if (s.member == &D::jump) {
        for (size_t k = 0; k < s.len && static_cast<int>(k) < max; ++k) out[k] = int_bits(T.i[s.off + k]);
        return static_cast<int>(s.len);
      }
    throw std::logic_error("table not packed");
  }
  for (const auto& s : T.fslot)
    if (s.member == ftab[which]) {
      for (size_t k = 0; k < s.len && static_cast<int>(k) < max; ++k) out[k] = T.f[s.off + k];
      return static_cast<int>(s.len);
    }
  throw std::logic_error("table not packed");
}

// mrs_debug_plan_layout: the overrides, the tables and the plan of a model; touches no device
int plan_layout(const Model& m, int n_envs, int cu_count, int max_contacts, int* out, int n) {
  const Overrides o = read_overrides();
  const DevTables T = build_tables(m, max_contacts, o);
  const Plan p = choose_plan(m, T, n_envs, cu_count, o);
  int v[kPlanLayoutValues];
  plan_layout_values(p.dm, p.group, p.g16_one_wg, p.wpb16, p.helpers, v);
  int k = 0;
  for (; k < n && k < kPlanLayoutValues; ++k) out[k] = v[k];
  return k;
}

void batch_set_stream(BatchImpl* b, void* stream) {
  b->stream = stream ? static_cast<hipStream_t>(stream) : b->own_stream;
}

// mj_resetData (key < 0) / mj_resetDataKeyframe of a range of envs by host copy: row key + 1 of the
// start rows, replicated, through the same row copy as every set.  qacc, qfrc_actuator, sensordata,
// ncon, solver_niter and the parameters keep their values
void batch_reset(BatchImpl* b, int key, int env0, int n) {
  const Model& m = *b->model;
  check_env_range(*b, env0, n);
  if (key >= m.nkey) throw std::invalid_argument("keyframe index out of range");
  b->ctrl_bound = nullptr;  // (host ctrl replaces a bound buffer, as in batch_set)
  if (n == 0) return;
  const StartRows& s = b->start;
  const size_t r = key < 0 ? 0 : static_cast<size_t>(key) + 1;
  auto rows = [&](const std::vector<float>& tab, int dim) {
    std::vector<double> v(static_cast<size_t>(n) * dim);
    for (size_t i = 0; i < v.size(); ++i) v[i] = tab[r * dim + i % dim];
    return v;
  };
  const std::vector<double> qpos = rows(s.qpos, m.nq), qvel = rows(s.qvel, m.nv), ctrl = rows(s.ctrl, m.nu),
                            act = rows(s.act, m.na), mp = rows(s.mpos, 3 * m.nmocap), mq = rows(s.mquat, 4 * m.nmocap),
                            t(n, s.time[r]), zeros(static_cast<size_t>(n) * std::max(m.nv, 4), 0.0);
  HIP_CHECK(hipSetDevice(b->device));
  if (b->st.xfrc_applied) {  // (mj_resetData zeroes xfrc_applied; a buffer never used stays unmade)
    const size_t row = static_cast<size_t>(6) * m.nbody;
    HIP_CHECK(hipMemsetAsync(b->st.xfrc_applied + env0 * row, 0, n * row * sizeof(float), b->stream));
  }
  rows_to_device(*b, env0, n, {{env_array(*b, MRS_FIELD_QPOS), qpos.data()},
                               {env_array(*b, MRS_FIELD_QVEL), qvel.data()},
                               {env_array(*b, MRS_FIELD_CTRL), ctrl.data()},
                               {env_array(*b, MRS_FIELD_QFRC_APPLIED), zeros.data()},
                               {env_array(*b, MRS_FIELD_QACC_WARMSTART), zeros.data()},
                               {env_array(*b, MRS_FIELD_TIME), t.data()},
                               {env_array(*b, kArrAct), act.data()},
                               {env_array(*b, kArrMocapPos), mp.data()},
                               {env_array(*b, kArrMocapQuat), mq.data()},
                               {env_array(*b, MRS_FIELD_WARNING), zeros.data()}});
}

// ---- start-state pool and masked reset (no reference counterpart: the reference resets one mjData
// on the host).  The pool rows are copied as given, as mj_resetDataKeyframe copies a keyframe.
void batch_set_start_states(BatchImpl* b, const double* qpos, const double* qvel, int count) {
  const Model& m = *b->model;
  if (count > 0 && !qpos) throw std::invalid_argument("null start-state qpos");
  reserve_pool(*b, count);
  b->pool_n = count;
  if (count == 0) return;
  std::vector<float> q(static_cast<size_t>(count) * m.nq), v(static_cast<size_t>(count) * m.nv, 0.0f);
  for (size_t i = 0; i < q.size(); ++i) q[i] = static_cast<float>(qpos[i]);
  if (qvel)
    for (size_t i = 0; i < v.size(); ++i) v[i] = static_cast<float>(qvel[i]);
  if (!q.empty())
    HIP_CHECK(hipMemcpyAsync(b->pool_qpos, q.data(), q.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
  if (!v.empty())
    HIP_CHECK(hipMemcpyAsync(b->pool_qvel, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
  HIP_CHECK(hipStreamSynchronize(b->stream));  // (the host rows are read by then)
}

void batch_set_start_states_device(BatchImpl* b, const float* d_qpos, const float* d_qvel, int count) {
  const Model& m = *b->model;
  if (count > 0 && !d_qpos) throw std::invalid_argument("null start-state qpos");
  reserve_pool(*b, count);
  b->pool_n = count;
  if (count == 0) return;
  const size_t nq = static_cast<size_t>(count) * m.nq * sizeof(float), nv = static_cast<size_t>(count) * m.nv * sizeof(float);
  if (nq) HIP_CHECK(hipMemcpyAsync(b->pool_qpos, d_qpos, nq, hipMemcpyDeviceToDevice, b->stream));
  if (nv && d_qvel) HIP_CHECK(hipMemcpyAsync(b->pool_qvel, d_qvel, nv, hipMemcpyDeviceToDevice, b->stream));
  if (nv && !d_qvel) HIP_CHECK(hipMemsetAsync(b->pool_qvel, 0, nv, b->stream));
}

int batch_num_start_states(const BatchImpl* b) { return b->pool_n; }

void batch_reset_masked_device(BatchImpl* b, const unsigned char* d_mask, const int* d_key, int key) {
  const Model& m = *b->model;
  if (!d_mask) throw std::invalid_argument("null reset mask");
  if (!d_key && key >= m.nkey + b->pool_n) throw std::invalid_argument("keyframe index out of range");
  HIP_CHECK(hipSetDevice(b->device));
  ResetArgs a{};
  a.mask = d_mask;
  a.keys = d_key;
  a.key = key < 0 ? -1 : key;
  a.n = b->n; a.nq = m.nq; a.nv = m.nv; a.nu = m.nu; a.na = m.na; a.nx = 6 * m.nbody; a.nmocap = m.nmocap;
  a.tab_mpos = b->tab_mpos; a.tab_mquat = b->tab_mquat; a.mocap_pos = b->dm.mocap_pos; a.mocap_quat = b->dm.mocap_quat;
  a.nkey = m.nkey; a.npool = b->pool_n;
  a.tab_qpos = b->tab_qpos; a.tab_qvel = b->tab_qvel; a.tab_ctrl = b->tab_ctrl; a.tab_act = b->tab_act; a.tab_time = b->tab_time;
  a.pool_qpos = b->pool_qpos; a.pool_qvel = b->pool_qvel;
  a.qpos = b->st.qpos; a.qvel = b->st.qvel; a.act = b->st.act;
  // a bound ctrl buffer is the caller's (a policy's output): it stays bound and unwritten, and so does
  // st.ctrl, which no launch reads while the binding lasts
  a.ctrl = b->ctrl_bound ? nullptr : b->st.ctrl;
  a.qfrc_applied = b->st.qfrc_applied; a.qacc_ws = b->st.qacc_ws;
  a.xfrc = b->st.xfrc_applied;  // (null until the field is first used: nothing to zero, none made)
  a.time = b->st.time;
  a.warning = b->st.warning;
  const unsigned blocks = static_cast<unsigned>((static_cast<size_t>(b->n) + 15) / 16);  // 16 envs per workgroup
  hipLaunchKernelGGL(reset_masked_kernel, dim3(blocks), dim3(256), 0, b->stream, a);
  HIP_CHECK(hipGetLastError());
}

void batch_reset_masked(BatchImpl* b, const unsigned char* mask, const int* keys, int key) {
  if (!mask) throw std::invalid_argument("null reset mask");
  if (!keys && key >= b->model->nkey + b->pool_n) throw std::invalid_argument("keyframe index out of range");
  HIP_CHECK(hipSetDevice(b->device));
  const size_t n = static_cast<size_t>(b->n);
  if (!b->mask_stage) b->mask_stage = static_cast<unsigned char*>(dalloc(*b, n));
  if (keys && !b->key_stage) b->key_stage = static_cast<int*>(dalloc(*b, n * sizeof(int)));
  HIP_CHECK(hipMemcpyAsync(b->mask_stage, mask, n, hipMemcpyHostToDevice, b->stream));
  if (keys) HIP_CHECK(hipMemcpyAsync(b->key_stage, keys, n * sizeof(int), hipMemcpyHostToDevice, b->stream));
  HIP_CHECK(hipStreamSynchronize(b->stream));  // (the host arrays are read by then; the kernel is not waited for)
  batch_reset_masked_device(b, b->mask_stage, keys ? b->key_stage : nullptr, key);
}

void batch_set(BatchImpl* b, int field, const double* host, int env0, int n) {
  EnvArray a = field_array(*b, field);
  check_env_range(*b, env0, n);
  if (field == MRS_FIELD_CTRL) b->ctrl_bound = nullptr;  // (host ctrl replaces a bound buffer)
  if (n == 0 || a.dim == 0) return;
  if (field == MRS_FIELD_XFRC_APPLIED) a.ptr = ensure_xfrc(*b);
  rows_to_device(*b, env0, n, {{a, host}});
}

void batch_get(BatchImpl* b, int field, double* host, int env0, int n) {
  EnvArray a = field_array(*b, field);
  check_env_range(*b, env0, n);
  if (n == 0 || a.dim == 0) return;
  if (field == MRS_FIELD_XFRC_APPLIED && !a.ptr) {  // never used: zeros, and no buffer made
    std::fill(host, host + static_cast<size_t>(n) * a.dim, 0.0);
    return;
  }
  if (field == MRS_FIELD_CTRL && b->ctrl_bound) a.ptr = const_cast<float*>(b->ctrl_bound);
  rows_to_host(*b, env0, n, {{a, host}});
}

void* batch_device_ptr(BatchImpl* b, int field) {
  return field == MRS_FIELD_XFRC_APPLIED ? ensure_xfrc(*b) : field_array(*b, field).ptr;
}

void batch_set_act(BatchImpl* b, const double* host, int env0, int n) {
  check_env_range(*b, env0, n);
  rows_to_device(*b, env0, n, {{env_array(*b, kArrAct), host}});
}

void batch_get_act(BatchImpl* b, double* host, int env0, int n) {
  check_env_range(*b, env0, n);
  rows_to_host(*b, env0, n, {{env_array(*b, kArrAct), host}});
}

float* batch_act_device_ptr(BatchImpl* b) { return b->st.act; }

void batch_set_mocap(BatchImpl* b, const double* pos, const double* quat, int env0, int n) {
  check_env_range(*b, env0, n);
  rows_to_device(*b, env0, n, {{env_array(*b, kArrMocapPos), pos}, {env_array(*b, kArrMocapQuat), quat}});
}

void batch_get_mocap(BatchImpl* b, double* pos, double* quat, int env0, int n) {
  check_env_range(*b, env0, n);
  rows_to_host(*b, env0, n, {{env_array(*b, kArrMocapPos), pos}, {env_array(*b, kArrMocapQuat), quat}});
}

float* batch_mocap_pos_device_ptr(BatchImpl* b) { return b->dm.mocap_pos; }
float* batch_mocap_quat_device_ptr(BatchImpl* b) { return b->dm.mocap_quat; }

int batch_param_dim(BatchImpl* b, int param) { return param_array(*b, param).dim; }

void batch_set_param(BatchImpl* b, int param, const double* host, int env0, int n) {
  EnvArray a = param_array(*b, param);
  check_env_range(*b, env0, n);
  if (n == 0 || a.dim == 0) return;
  // checked before anything is made or written: finite (in fp32 too), and no negative damping or friction
  const bool nonneg = param == MRS_PARAM_DOF_DAMPING || param == MRS_PARAM_GEOM_FRICTION;
  for (size_t i = 0; i < static_cast<size_t>(n) * a.dim; ++i) {
    const double x = host[i];
    if (!std::isfinite(x) || !std::isfinite(static_cast<float>(x))) throw std::invalid_argument("model parameter value is not finite");
    if (nonneg && x < 0) throw std::invalid_argument("negative damping or friction");
  }
  a.ptr = ensure_param(*b, param);
  rows_to_device(*b, env0, n, {{a, host}});
}

void batch_get_param(BatchImpl* b, int param, double* host, int env0, int n) {
  const EnvArray a = param_array(*b, param);
  check_env_range(*b, env0, n);
  if (n == 0 || a.dim == 0) return;
  if (!a.ptr) {  // never used: the model's values for every env, and no buffer made
    const std::vector<float> row = param_model_row(*b->model, param);
    for (int e = 0; e < n; ++e) std::copy(row.begin(), row.end(), host + static_cast<size_t>(e) * a.dim);
    return;
  }
  rows_to_host(*b, env0, n, {{a, host}});
}

float* batch_param_device_ptr(BatchImpl* b, int param) { return ensure_param(*b, param); }

int batch_inertial_dim(BatchImpl* b, int which) {
  const Model& m = *b->model;
  switch (which) {
    case MRS_INERTIAL_BODY_MASS: return m.nbody;
    case MRS_INERTIAL_BODY_INERTIA: return 3 * m.nbody;
    case MRS_INERTIAL_DOF_ARMATURE: return m.nv;
  }
  throw std::invalid_argument("unknown inertial quantity");
}

void batch_set_inertial(BatchImpl* b, const double* mass, const double* inertia, const double* armature, int env0, int n) {
  const Model& m = *b->model;
  if (!m.tendon_adr.empty()) throw UnsupportedError("per-env mass / inertia / armature on a model with tendons (tendon_invweight0)");
  check_env_range(*b, env0, n);
  if (n == 0 || (!mass && !inertia && !armature)) return;
  const int nb = m.nbody, nv = m.nv;
  const size_t hd = 4 * static_cast<size_t>(nb) + nv;
  // the envs' new inputs: what they hold now (the model's before the first set), the given quantities
  // substituted, the world's row kept.  Checked and derived before anything is made or written
  std::vector<double> in(static_cast<size_t>(n) * hd);
  for (int e = 0; e < n; ++e) {
    double* h = in.data() + e * hd;
    if (!b->inr_host.empty()) {
      std::copy_n(b->inr_host.data() + (static_cast<size_t>(env0) + e) * hd, hd, h);
    } else {
      std::copy(m.body_mass.begin(), m.body_mass.end(), h);
      std::copy(m.body_inertia.begin(), m.body_inertia.end(), h + nb);
      std::copy(m.dof_armature.begin(), m.dof_armature.end(), h + 4 * nb);
    }
    if (mass) std::copy_n(mass + static_cast<size_t>(e) * nb + 1, nb - 1, h + 1);
    if (inertia) std::copy_n(inertia + static_cast<size_t>(e) * 3 * nb + 3, 3 * (nb - 1), h + nb + 3);
    if (armature) std::copy_n(armature + static_cast<size_t>(e) * nv, nv, h + 4 * nb);
    check_inertial_values(m, h, h + nb, h + 4 * nb);
  }
  // one re-derivation per env (host, fp64; linear in n), over at most 16 threads for large ranges
  const InertialLayout l = inertial_layout(m);
  std::vector<double> rows(static_cast<size_t>(n) * l.dim);
  auto derive = [&](int e0, int e1) {
    for (int e = e0; e < e1; ++e) {
      const double* h = in.data() + e * hd;
      const std::vector<float> r = inertial_row(m, l, h, h + nb, h + 4 * nb);
      std::copy(r.begin(), r.end(), rows.begin() + static_cast<size_t>(e) * l.dim);
    }
  };
  const int nthreads = std::min(16, n / 64);
  if (nthreads < 2) {
    derive(0, n);
  } else {
    std::vector<std::thread> pool;
    std::vector<std::exception_ptr> err(nthreads);
    for (int t = 0; t < nthreads; ++t)
      pool.emplace_back([&, t] {
        try {
          derive(static_cast<int>(static_cast<long long>(n) * t / nthreads), static_cast<int>(static_cast<long long>(n) * (t + 1) / nthreads));
        } catch (...) {
          err[t] = std::current_exception();
        }
      });
    for (std::thread& t : pool) t.join();
    for (const std::exception_ptr& e : err) if (e) std::rethrow_exception(e);
  }
  ensure_inertial(*b);
  std::copy(in.begin(), in.end(), b->inr_host.begin() + static_cast<size_t>(env0) * hd);
  rows_to_device(*b, env0, n, {{env_array(*b, kArrInertial), rows.data()}});
}

void batch_get_inertial(BatchImpl* b, double* mass, double* inertia, double* armature, int env0, int n) {
  const Model& m = *b->model;
  check_env_range(*b, env0, n);
  const int nb = m.nbody, nv = m.nv;
  const size_t hd = 4 * static_cast<size_t>(nb) + nv;
  for (int e = 0; e < n; ++e) {
    // never set: the model's values for every env
    const double* h = b->inr_host.empty() ? nullptr : b->inr_host.data() + (static_cast<size_t>(env0) + e) * hd;
    if (mass) std::copy_n(h ? h : m.body_mass.data(), nb, mass + static_cast<size_t>(e) * nb);
    if (inertia) std::copy_n(h ? h + nb : m.body_inertia.data(), 3 * nb, inertia + static_cast<size_t>(e) * 3 * nb);
    if (armature) std::copy_n(h ? h + 4 * nb : m.dof_armature.data(), nv, armature + static_cast<size_t>(e) * nv);
  }
}

void batch_get_inertial_derived(BatchImpl* b, int env, double* body_subtreemass, double* dof_invweight0,
                                double* body_invweight0, double* meaninertia) {
  const Model& m = *b->model;
  check_env_range(*b, env, 1);
  const InertialLayout l = inertial_layout(m);
  const EnvArray a = env_array(*b, kArrInertial);
  std::vector<double> row(l.dim);
  if (a.ptr) {
    rows_to_host(*b, env, 1, {{a, row.data()}});
  } else {  // never set: the model's own row, and no buffer made
    const std::vector<float> r = inertial_model_row(m, l);
    std::copy(r.begin(), r.end(), row.begin());
  }
  if (body_subtreemass) std::copy_n(row.data() + l.subtreemass, m.nbody, body_subtreemass);
  if (dof_invweight0) std::copy_n(row.data() + l.dof_invweight0, m.nv, dof_invweight0);
  if (body_invweight0) std::copy_n(row.data() + l.body_invweight0, 2 * m.nbody, body_invweight0);
  if (meaninertia) *meaninertia = 1.0 / (row[l.pgs_scale] * std::max(1, m.nv));
}

void batch_bind_ctrl_device(BatchImpl* b, const float* d_ctrl) { b->ctrl_bound = d_ctrl; }

void batch_set_timing(BatchImpl* b, int mask) {
  b->timing = mask;
  if (!(mask & 1)) b->ev_valid[0] = false;
  if (!(mask & 2)) b->ev_valid[1] = false;
}

void batch_set_ctrl_device(BatchImpl* b, const float* d_ctrl) {
  const Model& m = *b->model;
  b->ctrl_bound = nullptr;
  if (m.nu == 0) return;
  HIP_CHECK(hipSetDevice(b->device));
  HIP_CHECK(hipMemcpyAsync(b->st.ctrl, d_ctrl, static_cast<size_t>(b->n) * m.nu * sizeof(float),
                           hipMemcpyDeviceToDevice, b->stream));
}

void batch_launch(BatchImpl* b, int n_steps, bool forward_only) {
  if (n_steps < 1) throw std::invalid_argument("n_steps must be positive");
  HIP_CHECK(hipSetDevice(b->device));
  const bool timed = (b->timing & 1) != 0;
  if (timed) HIP_CHECK(hipEventRecord(b->ev0[0], b->stream));
  DevState st = b->st;
  if (b->ctrl_bound) st.ctrl = const_cast<float*>(b->ctrl_bound);  // (read only: loaded at launch start)
  // (a model with site actuators takes the parameter parts, which alone carry their code: DESIGN.md §3.24)
  HIP_CHECK(launch_step(b->d_dm, b->L.total, b->dm.shr_total, st, b->n, n_steps, forward_only, b->group,
                        b->model->solver != MRS_SOL_PGS, b->ext, b->dm.prm_mask != 0 || b->dm.nact_site > 0,
                        b->dm.dyn_mask != 0, b->stream));
  if (timed) HIP_CHECK(hipEventRecord(b->ev1[0], b->stream));
  b->ev_valid[0] = timed;
}

// mjData.efc_* of the last forward pass of one env (type, dense J rows, R, aref, force).  Returns
// nefc: 0 when no row was built (constraints disabled, or none active).
int batch_get_efc(BatchImpl* b, int env, int max, int* type, double* J, double* R, double* aref, double* force) {
  if (env < 0 || env >= b->n) throw std::invalid_argument("env out of bounds");
  if (max < 0) throw std::invalid_argument("negative capacity");
  if (b->dm.blocked && b->model->solver == MRS_SOL_PGS && b->model->cone != MRS_CONE_ELLIPTIC && b->dm.xrows == 0)
    throw UnsupportedError("blocked-mode PGS keeps its constraint rows in sparse records");
  HIP_CHECK(hipSetDevice(b->device));
  const ScratchLayout& S = b->S;
  const float* base = b->st.scratch + static_cast<size_t>(env) * S.total;
  int nefc = 0;
  HIP_CHECK(hipMemcpyAsync(&nefc, base + S.efc_n, sizeof(int), hipMemcpyDeviceToHost, b->stream));
  HIP_CHECK(hipStreamSynchronize(b->stream));
  if (nefc < 0) throw UnsupportedError("the register friction-loss path keeps no dense rows");
  const int n = std::min(nefc, max), nv = b->model->nv;
  if (n <= 0) return nefc;
  std::vector<float> t(n), j(static_cast<size_t>(n) * nv), r(n), a(n), f(n);
  auto get = [&](float* dst, int off, size_t count) {
    HIP_CHECK(hipMemcpyAsync(dst, base + off, count * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  };
  get(t.data(), S.efc_type, n); get(j.data(), S.efc_J, j.size()); get(r.data(), S.efc_R, n);
  get(a.data(), S.efc_aref, n); get(f.data(), S.efc_f, n);
  HIP_CHECK(hipStreamSynchronize(b->stream));
  for (int i = 0; i < n; ++i) {
    int code;
    std::memcpy(&code, &t[i], sizeof code);
    if (type) type[i] = code >> 16;
    if (R) R[i] = r[i];
    if (aref) aref[i] = a[i];
    if (force) force[i] = f[i];
    if (J) for (int k = 0; k < nv; ++k) J[static_cast<size_t>(i) * nv + k] = j[static_cast<size_t>(i) * nv + k];
  }
  return nefc;
}

// mjData.contact of the last forward pass of one env (geom1/geom2 as mj_collision orders them: pair
// order g1 < g2 with the lower geom type first, then the narrow phase's order).  Records are read from
// the env's contact scratch (step.hip collision(): pair id, dist, pos, frame).  Returns ncon.
int batch_get_contacts(BatchImpl* b, int env, int max, int* geom, double* dist, double* pos, double* frame) {
  if (env < 0 || env >= b->n) throw std::invalid_argument("env out of bounds");
  if (max < 0) throw std::invalid_argument("negative capacity");
  HIP_CHECK(hipSetDevice(b->device));
  int ncon = 0;
  HIP_CHECK(hipMemcpyAsync(&ncon, b->st.ncon + env, sizeof(int), hipMemcpyDeviceToHost, b->stream));
  HIP_CHECK(hipStreamSynchronize(b->stream));
  const int n = std::min(ncon, max);
  if (n <= 0) return ncon;
  std::vector<float> rec(static_cast<size_t>(n) * kConRec);
  const float* src = b->st.scratch + static_cast<size_t>(env) * b->S.total + b->S.con;
  HIP_CHECK(hipMemcpyAsync(rec.data(), src, rec.size() * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  HIP_CHECK(hipStreamSynchronize(b->stream));
  for (int c = 0; c < n; ++c) {
    const float* r = &rec[static_cast<size_t>(c) * kConRec];
    int p;
    std::memcpy(&p, r, sizeof(int));
    if (p < 0 || p >= static_cast<int>(b->pair_g1.size())) throw DeviceError("corrupt contact record");
    if (geom) { geom[2 * c] = b->pair_g1[p]; geom[2 * c + 1] = b->pair_g2[p]; }
    if (dist) dist[c] = r[1];
    if (pos) for (int i = 0; i < 3; ++i) pos[3 * c + i] = r[2 + i];
    if (frame) for (int i = 0; i < 9; ++i) frame[9 * c + i] = r[5 + i];
  }
  return ncon;
}

// mj_contactForce of every contact of batch_get_contacts' list, in its order: [max][6] in the contact
// frame (normal, tangent 1, tangent 2, then the torques, zero at condim 1 and 3), decoded on the host
// from the env's contact records and row forces (efc_f at the record's first row, rec[14]) as step.hip
// rne_post decodes them; a contact whose rows the cap cut gives zeros.  The pyramid's friction is the
// pair's as the kernel sees it (pair_mu): per-env geom friction where the parameter is set.  Returns ncon
int batch_get_contact_forces(BatchImpl* b, int env, int max, double* force) {
  if (env < 0 || env >= b->n) throw std::invalid_argument("env out of bounds");
  if (max < 0) throw std::invalid_argument("negative capacity");
  if (max > 0 && !force) throw std::invalid_argument("null force buffer");
  HIP_CHECK(hipSetDevice(b->device));
  int ncon = 0;
  HIP_CHECK(hipMemcpyAsync(&ncon, b->st.ncon + env, sizeof(int), hipMemcpyDeviceToHost, b->stream));
  HIP_CHECK(hipStreamSynchronize(b->stream));
  const int n = std::min(ncon, max);
  if (n <= 0) return ncon;
  const Model& m = *b->model;
  const ScratchLayout& S = b->S;
  const float* base = b->st.scratch + static_cast<size_t>(env) * S.total;
  const int ne = std::max(1, b->dm.max_efc);
  std::vector<float> rec(static_cast<size_t>(n) * kConRec), f(ne), fric;
  HIP_CHECK(hipMemcpyAsync(rec.data(), base + S.con, rec.size() * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  HIP_CHECK(hipMemcpyAsync(f.data(), base + S.efc_f, f.size() * sizeof(float), hipMemcpyDeviceToHost, b->stream));
  if (b->dm.prm_fric) {
    fric.resize(m.ngeom);
    HIP_CHECK(hipMemcpyAsync(fric.data(), b->dm.prm_fric + static_cast<size_t>(env) * m.ngeom, fric.size() * sizeof(float),
                             hipMemcpyDeviceToHost, b->stream));
  }
  HIP_CHECK(hipStreamSynchronize(b->stream));
  const bool elliptic = m.cone == MRS_CONE_ELLIPTIC;
  for (int c = 0; c < n; ++c) {
    const float* r = &rec[static_cast<size_t>(c) * kConRec];
    double* out = force + 6 * static_cast<size_t>(c);
    std::fill(out, out + 6, 0.0);
    int p, r0;
    std::memcpy(&p, r, sizeof(int));
    std::memcpy(&r0, r + 14, sizeof(int));
    if (p < 0 || p >= static_cast<int>(b->pair_g1.size())) throw DeviceError("corrupt contact record");
    if (r0 < 0) continue;
    const int rows = b->pair_dim[p] == 1 ? 1 : (elliptic ? 3 : 4);
    if (r0 + rows > ne) throw DeviceError("corrupt contact record");
    if (b->pair_dim[p] == 1) {
      out[0] = f[r0];
    } else if (elliptic) {
      for (int i = 0; i < 3; ++i) out[i] = f[r0 + i];
    } else {
      float mu = b->pair_mu[p];
      if (!fric.empty() && p >= b->dm.npair_explicit) mu = std::max(fric[b->pair_g1[p]], fric[b->pair_g2[p]]);
      // (in fp32 and in the kernel's order of operations: the same value as its decode)
      float lf[3] = {0, 0, 0};
      for (int k = 0; k < 2; ++k) {
        const float fp = f[r0 + 2 * k], fm = f[r0 + 2 * k + 1];
        lf[0] += fp + fm;
        lf[k + 1] = (fp - fm) * mu;
      }
      for (int i = 0; i < 3; ++i) out[i] = lf[i];
    }
  }
  return ncon;
}

// the net contact wrench per body: the device buffer [n_envs][nbody][6] (made on first use, which turns
// the output on for every later launch), and host rows [n][nbody][6] of it
float* batch_contact_wrench_device_ptr(BatchImpl* b) { return ensure_contact_wrench(*b); }

void batch_get_contact_wrench(BatchImpl* b, double* host, int env0, int n) {
  check_env_range(*b, env0, n);
  ensure_contact_wrench(*b);
  rows_to_host(*b, env0, n, {{env_array(*b, kArrContactWrench), host}});
}

// the dynamics outputs (mrs.h MRS_DYNOUT_*): the sites the two site outputs cover, an output's floats per
// env, its device buffer (made on first use, which turns it on for every later launch) and host rows
void batch_set_jac_sites(BatchImpl* b, const int* site_ids, int n) {
  const Model& m = *b->model;
  if (n < 0 || n > MRS_MAX_JAC_SITES) throw std::invalid_argument("site count out of range");
  if (n > 0 && !site_ids) throw std::invalid_argument("null site list");
  for (int k = 0; k < n; ++k) {
    if (site_ids[k] < 0 || site_ids[k] >= m.nsite) throw std::invalid_argument("site id out of range");
    for (int q = 0; q < k; ++q)
      if (site_ids[q] == site_ids[k]) throw std::invalid_argument("duplicate site id");
  }
  // Nothing has changed up to here: a rejected call leaves the selection and the buffers as they were.
  // From here on the order keeps a failure harmless: the new buffers are made first (a failed allocation
  // leaves the batch as it was), then the model block with them is uploaded, and only then are the old
  // buffers freed -- the device block never names freed memory
  HIP_CHECK(hipSetDevice(b->device));
  HIP_CHECK(hipStreamSynchronize(b->stream));
  DevModel nd = b->dm;
  nd.dyn_nsel = n;
  for (int k = 0; k < MRS_MAX_JAC_SITES; ++k) nd.dyn_site[k] = k < n ? site_ids[k] : 0;
  const int dims[2] = {n * 6 * m.nv, n * 12};
  const int which[2] = {MRS_DYNOUT_SITE_JAC, MRS_DYNOUT_SITE_POSE};
  float* old[2] = {b->dm.dyn_out[which[0]], b->dm.dyn_out[which[1]]};
  auto release = [&](float* p) {
    if (!p) return;
    b->allocs.erase(std::remove(b->allocs.begin(), b->allocs.end(), static_cast<void*>(p)), b->allocs.end());
    (void)hipFree(p);
  };
  try {
    for (int k = 0; k < 2; ++k) {
      const int w = which[k];
      nd.dyn_out[w] = nullptr;
      nd.dyn_mask &= ~(1 << w);
      if (!(b->dyn_asked & (1 << w)) || dims[k] == 0) continue;
      nd.dyn_out[w] = static_cast<float*>(dalloc(*b, static_cast<size_t>(b->n) * dims[k] * sizeof(float)));
      nd.dyn_mask |= 1 << w;
    }
    HIP_CHECK(hipStreamSynchronize(b->stream));
    HIP_CHECK(hipMemcpy(b->d_dm, &nd, sizeof(DevModel), hipMemcpyHostToDevice));
  } catch (...) {
    for (int k = 0; k < 2; ++k) release(nd.dyn_out[which[k]]);
    throw;
  }
  b->dm = nd;
  for (int k = 0; k < 2; ++k) release(old[k]);
}

int batch_dyn_dim(const BatchImpl* b, int which) { return dyn_dim(*b, which); }

float* batch_dyn_device_ptr(BatchImpl* b, int which) { return ensure_dyn(*b, which); }

void batch_get_dyn(BatchImpl* b, int which, double* host, int env0, int n) {
  check_env_range(*b, env0, n);
  // (a site output with no site selected has no elements: nothing is copied, and host may be null)
  if (!host && n > 0 && dyn_dim(*b, which) > 0) throw std::invalid_argument("null host buffer");
  ensure_dyn(*b, which);
  rows_to_host(*b, env0, n, {{env_array(*b, kArrDyn0 + which), host}});
}

// fp32 field rows [env0, env0 + n) into a caller device buffer [n][dim], ordered on the batch stream
// (observation export without a host round trip, e.g. for the end-of-step RCCL gather)
void batch_get_field_device(BatchImpl* b, int field, float* d_out, int env0, int n) {
  EnvArray a = env_array(*b, field);
  if (field < 0 || field >= MRS_FIELD_COUNT || a.type != EnvArray::F32) throw std::invalid_argument("not an fp32 state field");
  check_env_range(*b, env0, n);
  if (n == 0 || a.dim == 0) return;
  HIP_CHECK(hipSetDevice(b->device));
  if (field == MRS_FIELD_XFRC_APPLIED) a.ptr = ensure_xfrc(*b);
  if (field == MRS_FIELD_CTRL && b->ctrl_bound) a.ptr = const_cast<float*>(b->ctrl_bound);
  HIP_CHECK(hipMemcpyAsync(d_out, static_cast<const float*>(a.ptr) + static_cast<size_t>(env0) * a.dim,
                           static_cast<size_t>(n) * a.dim * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
}

void batch_sync(BatchImpl* b) {
  HIP_CHECK(hipSetDevice(b->device));
  HIP_CHECK(hipStreamSynchronize(b->stream));
  if (b->rstream) HIP_CHECK(hipStreamSynchronize(b->rstream));
}

double batch_last_kernel_ms(BatchImpl* b, int kind) {
  if (kind < 0 || kind > 1 || !b->ev_valid[kind]) return -1;
  HIP_CHECK(hipSetDevice(b->device));
  HIP_CHECK(hipEventSynchronize(b->ev1[kind]));
  float ms = -1;
  if (hipEventElapsedTime(&ms, b->ev0[kind], b->ev1[kind]) != hipSuccess) return -1;
  return ms;
}

}  // namespace mrs
