// What a batch's per-env arrays start from, in the fp32 the device holds: the model's start states
// (qpos0 and the keyframes) and its own row of each per-env parameter.  Host only, no HIP: the range
// reset copies these rows, the masked reset reads their upload, and an unset parameter reads as its row,
// so the three cannot disagree on a rounding.
#pragma once

#include <algorithm>
#include <vector>

#include "../../../include/mrs.h"
#include "../mjcf/model.h"

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

}  // namespace mrs
