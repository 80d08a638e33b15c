// What a batch's per-env arrays start from, in the fp32 the device holds: the model's start states
// (qpos0 and the keyframes) and its own row of each per-env parameter.  Host only, no HIP: the range
// reset copies these rows, the masked reset reads their upload, and an unset parameter reads as its row,
// so the three cannot disagree on a rounding.
#pragma once

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <vector>

#include "../../../include/mrs.h"
#include "../mjcf/model.h"
#include "../mjcf/setconst.h"

namespace mrs {

// [rows = 1 + nkey] start states in the state arrays' layout: row 0 is qpos0 with zero qvel / ctrl /
// act / time and the mocap bodies' own pos / quat (mj_resetData), row 1 + k is keyframe k
// (mj_resetDataKeyframe).  time stays fp64, like the time field
struct StartRows {
  int rows = 0;
  std::vector<float> qpos, qvel, ctrl, act, mpos, mquat;  // [rows][nq | nv | nu | na | 3 nmocap | 4 nmocap]
  std::vector<double> time;                              // [rows]
};

inline StartRows start_rows(const Model& m) {
  StartRows s;
  s.rows = m.nkey + 1;
  const size_t nkey = static_cast<size_t>(m.nkey);
  std::vector<double> mp0(3 * static_cast<size_t>(m.nmocap)), mq0(4 * static_cast<size_t>(m.nmocap));
  for (int bd = 0; bd < m.nbody; ++bd) {
    const int id = m.body_mocapid[bd];
    if (id < 0) continue;
    std::copy(&m.body_pos[3 * bd], &m.body_pos[3 * bd] + 3, &mp0[3 * id]);
    std::copy(&m.body_quat[4 * bd], &m.body_quat[4 * bd] + 4, &mq0[4 * id]);
  }
  // row 0 (null: zeros), then the keyframes' rows
  auto fill = [nkey](std::vector<float>& dst, int dim, const double* row0, const std::vector<double>& keys) {
    dst.assign((nkey + 1) * dim, 0.0f);
    for (int i = 0; row0 && i < dim; ++i) dst[i] = static_cast<float>(row0[i]);
    for (size_t i = 0; i < nkey * dim; ++i) dst[dim + i] = static_cast<float>(keys[i]);
  };
  fill(s.qpos, m.nq, m.qpos0.data(), m.key_qpos);
  fill(s.qvel, m.nv, nullptr, m.key_qvel);
  fill(s.ctrl, m.nu, nullptr, m.key_ctrl);
  fill(s.act, m.na, nullptr, m.key_act);
  fill(s.mpos, 3 * m.nmocap, mp0.data(), m.key_mpos);
  fill(s.mquat, 4 * m.nmocap, mq0.data(), m.key_mquat);
  s.time.assign(nkey + 1, 0.0);
  std::copy(m.key_time.begin(), m.key_time.begin() + m.nkey, s.time.begin() + 1);
  return s;
}

// the model's own row of a per-env parameter (MRS_PARAM_*; empty for an unknown one), in the fp32
// rounding the kernel's tables hold (actrec, dofrec, pair_friction)
inline std::vector<float> param_model_row(const Model& m, int param) {
  std::vector<float> r;
  switch (param) {
    case MRS_PARAM_ACT_GAINPRM:
      for (int i = 0; i < 3 * m.nu; ++i) r.push_back(static_cast<float>(m.actuator_gainprm[MRS_NGAIN * (i / 3) + i % 3]));
      break;
    case MRS_PARAM_ACT_BIASPRM:
      for (int i = 0; i < 3 * m.nu; ++i) r.push_back(static_cast<float>(m.actuator_biasprm[MRS_NBIAS * (i / 3) + i % 3]));
      break;
    case MRS_PARAM_DOF_DAMPING:
      for (int i = 0; i < m.nv; ++i) r.push_back(static_cast<float>(m.dof_damping[i]));
      break;
    case MRS_PARAM_GEOM_FRICTION:
      for (int i = 0; i < m.ngeom; ++i) r.push_back(static_cast<float>(m.geom_friction[3 * i]));
      break;
  }
  return r;
}

// ---- per-env body mass / inertia / dof armature and the constants derived from them (MRS_INERTIAL_*;
// DESIGN.md §3.16).  One fp32 row per env, inputs first, then what mj_setConst derives from them:
//   mass [nbody] | inertia [3 nbody] | armature [nv] | body_subtreemass [nbody] | dof_invweight0 [nv] |
//   body_invweight0 [2 nbody] | R of each friction-loss dof's row [nfric] | pgs_scale [1]
// step.hip reads the row by these offsets (inr_* there).
struct InertialLayout {
  int mass, inertia, armature, subtreemass, dof_invweight0, body_invweight0, fric_R, pgs_scale, dim;
};
inline int num_fric_dofs(const Model& m) {
  int n = 0;
  for (int j = 0; j < m.nv; ++j) n += m.dof_frictionloss[j] > 0;
  return n;
}
inline InertialLayout inertial_layout(const Model& m) {
  InertialLayout l;
  l.mass = 0;
  l.inertia = m.nbody;
  l.armature = 4 * m.nbody;
  l.subtreemass = l.armature + m.nv;
  l.dof_invweight0 = l.subtreemass + m.nbody;
  l.body_invweight0 = l.dof_invweight0 + m.nv;
  l.fric_R = l.body_invweight0 + 2 * m.nbody;
  l.pgs_scale = l.fric_R + num_fric_dofs(m);
  l.dim = l.pgs_scale + 1;
  return l;
}

// the regulariser R of dof j's friction-loss row (distance 0 at margin 0, so a model constant) from the
// dof's invweight0, in fp32 and in the order the kernel's row_impedance computes it: the one expression
// behind the shared fricrec table and an env's inertial row
inline float fric_row_R(const Model& m, int j, double dof_invweight0) {
  auto clampf = [](float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); };
  const float si0 = static_cast<float>(m.dof_solimp[5 * j]), si1 = static_cast<float>(m.dof_solimp[5 * j + 1]);
  const float width = static_cast<float>(m.dof_solimp[5 * j + 2]);
  const float dmin = clampf(si0, 0.0001f, 0.9999f), dmax = clampf(si1, 0.0001f, 0.9999f);
  const float imp = (dmin == dmax || width <= 1e-15f) ? 0.5f * (dmin + dmax) : dmin;
  float R = (1 - imp) * static_cast<float>(dof_invweight0) / imp;
  R = R > 1e-15f ? R : 1e-15f;
  return R;
}
// the PGS stop test's / primal solvers' scale, as the model block holds it
inline float solver_scale(double meaninertia, int nv) {
  return static_cast<float>(1.0 / (meaninertia * std::max(1, nv)));
}

// finite and non-negative, in fp32 too (what set_inertial and mrs_model_derive_inertial check before
// anything is derived or written); row 0 (the world) is not looked at by the callers that ignore it
inline void check_inertial_values(const Model& m, const double* mass, const double* inertia, const double* armature) {
  auto check = [](const double* v, int n) {
    for (int i = 0; v && i < n; ++i) {
      if (!std::isfinite(v[i]) || !std::isfinite(static_cast<float>(v[i])))
        throw std::invalid_argument("inertial value is not finite");
      if (v[i] < 0) throw std::invalid_argument("negative mass, inertia or armature");
    }
  };
  check(mass, m.nbody);
  check(inertia, 3 * m.nbody);
  check(armature, m.nv);
}

// an env's inertial row from its fp64 mass / inertia / armature: the constants by the compiler's own
// function (setconst.h), each rounded to fp32 exactly as the model block is packed, so the model's own
// values give the values the shared tables hold.  Throws std::invalid_argument when M(qpos0) is not
// positive definite
inline std::vector<float> inertial_row(const Model& m, const InertialLayout& l, const double* mass, const double* inertia,
                                       const double* armature) {
  setconst::InertialConst c;
  try {
    setconst::derive_inertial(m, mass, inertia, armature, c);
  } catch (const std::runtime_error&) {
    throw std::invalid_argument("M(qpos0) is not positive definite for these inertial values");
  }
  std::vector<float> r(l.dim);
  for (int b = 0; b < m.nbody; ++b) {
    r[l.mass + b] = static_cast<float>(mass[b]);
    for (int i = 0; i < 3; ++i) r[l.inertia + 3 * b + i] = static_cast<float>(inertia[3 * b + i]);
    r[l.subtreemass + b] = static_cast<float>(c.body_subtreemass[b]);
    for (int i = 0; i < 2; ++i) r[l.body_invweight0 + 2 * b + i] = static_cast<float>(c.body_invweight0[2 * b + i]);
  }
  int k = 0;
  for (int j = 0; j < m.nv; ++j) {
    r[l.armature + j] = static_cast<float>(armature[j]);
    r[l.dof_invweight0 + j] = static_cast<float>(c.dof_invweight0[j]);
    if (m.dof_frictionloss[j] > 0) r[l.fric_R + k++] = fric_row_R(m, j, c.dof_invweight0[j]);
  }
  r[l.pgs_scale] = solver_scale(c.meaninertia, m.nv);
  return r;
}
// the model's own inertial row: what every env holds until it is set
inline std::vector<float> inertial_model_row(const Model& m, const InertialLayout& l) {
  return inertial_row(m, l, m.body_mass.data(), m.body_inertia.data(), m.dof_armature.data());
}

}  // namespace mrs
