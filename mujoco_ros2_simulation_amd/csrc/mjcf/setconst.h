// The constants mj_setConst derives from body_mass / body_inertia / dof_armature at qpos0
// (MuJoCo engine_setconst.c, restated): body_subtreemass, dof_M0, stat_meaninertia, dof_invweight0 and
// body_invweight0.  One source: the MJCF compiler calls derive_inertial() on the model it is building,
// and a batch calls it again per env with that env's mass / inertia / armature substituted (DESIGN.md
// §3.16), so the two cannot disagree by a bit.  Host only, fp64, no HIP.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "model.h"

namespace mrs {
namespace setconst {

constexpr double kMinVal = 1e-15;

// ---------------------------------------------------------------- fp64 3D math
inline void quat_mul(double r[4], const double a[4], const double b[4]) {
  double t[4] = {a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                 a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                 a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                 a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]};
  std::memcpy(r, t, sizeof t);
}
inline void quat_normalize(double q[4]) {
  double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < kMinVal) { q[0] = 1; q[1] = q[2] = q[3] = 0; return; }
  for (int i = 0; i < 4; ++i) q[i] /= n;
}
inline void quat2mat(double m[9], const double q[4]) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
inline void rot_vec_quat(double r[3], const double v[3], const double q[4]) {
  double m[9];
  quat2mat(m, q);
  double t[3] = {m[0] * v[0] + m[1] * v[1] + m[2] * v[2], m[3] * v[0] + m[4] * v[1] + m[5] * v[2],
                 m[6] * v[0] + m[7] * v[1] + m[8] * v[2]};
  std::memcpy(r, t, sizeof t);
}
inline void cross3(double r[3], const double a[3], const double b[3]) {
  double t[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  std::memcpy(r, t, sizeof t);
}

// spatial inertia about the tree's com (mju_inertCom): principal moments `inert` in the frame `mat`,
// com offset `dif`
inline void inert_com(double res[10], const double inert[3], const double mat[9], const double dif[3], double mass) {
  double full[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double v = 0;
      for (int k = 0; k < 3; ++k) v += mat[r * 3 + k] * inert[k] * mat[c * 3 + k];
      full[r * 3 + c] = v;
    }
  res[0] = full[0] + mass * (dif[1] * dif[1] + dif[2] * dif[2]);
  res[1] = full[4] + mass * (dif[0] * dif[0] + dif[2] * dif[2]);
  res[2] = full[8] + mass * (dif[0] * dif[0] + dif[1] * dif[1]);
  res[3] = full[1] - mass * dif[0] * dif[1];
  res[4] = full[2] - mass * dif[0] * dif[2];
  res[5] = full[5] - mass * dif[1] * dif[2];
  res[6] = mass * dif[0]; res[7] = mass * dif[1]; res[8] = mass * dif[2];
  res[9] = mass;
}
inline void mul_inert_vec(double r[6], const double i[10], const double v[6]) {
  r[0] = i[0] * v[0] + i[3] * v[1] + i[4] * v[2] - i[8] * v[4] + i[7] * v[5];
  r[1] = i[3] * v[0] + i[1] * v[1] + i[5] * v[2] + i[8] * v[3] - i[6] * v[5];
  r[2] = i[4] * v[0] + i[5] * v[1] + i[2] * v[2] - i[7] * v[3] + i[6] * v[4];
  r[3] = i[8] * v[1] - i[7] * v[2] + i[9] * v[3];
  r[4] = i[6] * v[2] - i[8] * v[0] + i[9] * v[4];
  r[5] = i[7] * v[0] - i[6] * v[1] + i[9] * v[5];
}
// inverse of a symmetric positive definite matrix by dense Cholesky; throws when a pivot is not positive
inline void dense_inverse_spd(const std::vector<double>& A, std::vector<double>& inv, int n) {
  std::vector<double> L(n * n, 0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = A[i * n + j];
      for (int k = 0; k < j; ++k) s -= L[i * n + k] * L[j * n + k];
      if (i == j) {
        if (s <= 0) throw std::runtime_error("MJCF error: mass matrix at qpos0 is not positive definite");
        L[i * n + i] = std::sqrt(s);
      } else {
        L[i * n + j] = s / L[j * n + j];
      }
    }
  for (int c = 0; c < n; ++c) {
    std::vector<double> y(n, 0);
    for (int i = 0; i < n; ++i) {
      double s = (i == c) ? 1 : 0;
      for (int k = 0; k < i; ++k) s -= L[i * n + k] * y[k];
      y[i] = s / L[i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
      double s = y[i];
      for (int k = i + 1; k < n; ++k) s -= L[k * n + i] * inv[k * n + c];
      inv[i * n + c] = s / L[i * n + i];
    }
  }
}

// what derive_inertial() computes: the derived constants, and the kinematics at qpos0 and M^-1 that
// the compiler goes on to use (light poses, tendon_invweight0, the statistics)
struct InertialConst {
  std::vector<double> body_subtreemass, dof_M0, dof_invweight0, body_invweight0;
  double meaninertia = 1;
  std::vector<double> xpos, xquat, xipos;  // body frames and inertial-frame origins at qpos0
  std::vector<double> Minv;                // M(qpos0)^-1, dense [nv][nv]
  std::vector<double> scom, cdof;          // subtree coms [nbody][3] and motion axes about them [nv][6] at qpos0
};

// The constants of model m with body_mass [nbody], body_inertia [nbody][3] and dof_armature [nv]
// replaced by the given arrays (the tree, the joints, body_ipos / body_iquat and qpos0 are m's).
// Throws std::runtime_error when M(qpos0) is not positive definite.
inline void derive_inertial(const Model& m, const double* body_mass, const double* body_inertia,
                            const double* dof_armature, InertialConst& out) {
  const int nb = m.nbody, nv = m.nv;
  out.body_subtreemass.assign(body_mass, body_mass + nb);
  for (int b = nb - 1; b > 0; --b) out.body_subtreemass[m.body_parentid[b]] += out.body_subtreemass[b];
  const std::vector<double>& body_subtreemass = out.body_subtreemass;

  std::vector<double>&xpos = out.xpos, &xquat = out.xquat, &xipos = out.xipos;
  xpos.assign(3 * nb, 0); xquat.assign(4 * nb, 0); xipos.assign(3 * nb, 0);
  std::vector<double> xmat(9 * nb), ximat(9 * nb);
  std::vector<double> xanchor(3 * std::max(1, m.njnt)), xaxis(3 * std::max(1, m.njnt));
  xquat[0] = 1;
  quat2mat(&xmat[0], &xquat[0]);
  std::memcpy(&ximat[0], &xmat[0], 9 * sizeof(double));
  for (int b = 1; b < nb; ++b) {
    int p = m.body_parentid[b];
    double* pos = &xpos[3 * b];
    double* q = &xquat[4 * b];
    int ja = m.body_jntadr[b];
    if (m.body_jntnum[b] > 0 && m.jnt_type[ja] == MRS_JNT_FREE) {
      int a = m.jnt_qposadr[ja];
      for (int i = 0; i < 3; ++i) pos[i] = m.qpos0[a + i];
      for (int i = 0; i < 4; ++i) q[i] = m.qpos0[a + 3 + i];
      quat_normalize(q);
      for (int i = 0; i < 3; ++i) { xanchor[3 * ja + i] = pos[i]; xaxis[3 * ja + i] = 0; }
    } else {
      double r[3];
      rot_vec_quat(r, &m.body_pos[3 * b], &xquat[4 * p]);
      for (int i = 0; i < 3; ++i) pos[i] = xpos[3 * p + i] + r[i];
      quat_mul(q, &xquat[4 * p], &m.body_quat[4 * b]);
      for (int k = 0; k < m.body_jntnum[b]; ++k) {
        int j = ja + k;
        rot_vec_quat(&xanchor[3 * j], &m.jnt_pos[3 * j], q);
        for (int i = 0; i < 3; ++i) xanchor[3 * j + i] += pos[i];
        rot_vec_quat(&xaxis[3 * j], &m.jnt_axis[3 * j], q);
        // at qpos0 hinge/slide displacement is zero and ball is identity
      }
    }
    quat_normalize(q);
    quat2mat(&xmat[9 * b], q);
    double r[3], iq[4];
    rot_vec_quat(r, &m.body_ipos[3 * b], q);
    for (int i = 0; i < 3; ++i) xipos[3 * b + i] = pos[i] + r[i];
    quat_mul(iq, q, &m.body_iquat[4 * b]);
    quat2mat(&ximat[9 * b], iq);
  }
  // subtree com
  std::vector<double>& scom = out.scom;
  scom.assign(3 * nb, 0);
  for (int b = 0; b < nb; ++b)
    for (int i = 0; i < 3; ++i) scom[3 * b + i] = body_mass[b] * xipos[3 * b + i];
  for (int b = nb - 1; b > 0; --b)
    for (int i = 0; i < 3; ++i) scom[3 * m.body_parentid[b] + i] += scom[3 * b + i];
  for (int b = 0; b < nb; ++b)
    for (int i = 0; i < 3; ++i)
      scom[3 * b + i] = body_subtreemass[b] > kMinVal ? scom[3 * b + i] / body_subtreemass[b] : xipos[3 * b + i];
  // cdof
  std::vector<double>& cdof = out.cdof;
  cdof.assign(6 * std::max(1, nv), 0);
  for (int j = 0; j < m.njnt; ++j) {
    int b = m.jnt_bodyid[j], d = m.jnt_dofadr[j];
    const double* c = &scom[3 * m.body_rootid[b]];
    double off[3];
    for (int i = 0; i < 3; ++i) off[i] = c[i] - xanchor[3 * j + i];
    auto rot_dof = [&](double* o, const double* ax) {
      o[0] = ax[0]; o[1] = ax[1]; o[2] = ax[2];
      cross3(o + 3, ax, off);
    };
    switch (m.jnt_type[j]) {
      case MRS_JNT_HINGE: rot_dof(&cdof[6 * d], &xaxis[3 * j]); break;
      case MRS_JNT_SLIDE:
        for (int i = 0; i < 3; ++i) { cdof[6 * d + i] = 0; cdof[6 * d + 3 + i] = xaxis[3 * j + i]; }
        break;
      case MRS_JNT_FREE:
        for (int k = 0; k < 3; ++k)
          for (int i = 0; i < 6; ++i) cdof[6 * (d + k) + i] = (i == 3 + k) ? 1 : 0;
        d += 3;
        [[fallthrough]];
      case MRS_JNT_BALL:
        for (int k = 0; k < 3; ++k) {
          double ax[3] = {xmat[9 * b + k], xmat[9 * b + 3 + k], xmat[9 * b + 6 + k]};
          rot_dof(&cdof[6 * (d + k)], ax);
        }
        break;
    }
  }
  // cinert, crb, M
  std::vector<double> crb(10 * nb, 0);
  for (int b = 1; b < nb; ++b) {
    double dif[3];
    for (int i = 0; i < 3; ++i) dif[i] = xipos[3 * b + i] - scom[3 * m.body_rootid[b] + i];
    inert_com(&crb[10 * b], &body_inertia[3 * b], &ximat[9 * b], dif, body_mass[b]);
  }
  for (int b = nb - 1; b > 0; --b)
    if (m.body_parentid[b] > 0)
      for (int i = 0; i < 10; ++i) crb[10 * m.body_parentid[b] + i] += crb[10 * b + i];
  std::vector<double> M(nv * nv, 0);
  for (int i = 0; i < nv; ++i) {
    double buf[6];
    mul_inert_vec(buf, &crb[10 * m.dof_bodyid[i]], &cdof[6 * i]);
    for (int j = i; j >= 0; j = m.dof_parentid[j]) {
      double v = 0;
      for (int k = 0; k < 6; ++k) v += cdof[6 * j + k] * buf[k];
      M[i * nv + j] = M[j * nv + i] = v;
    }
    M[i * nv + i] += dof_armature[i];
  }
  out.dof_M0.resize(nv);
  double trace = 0;
  for (int i = 0; i < nv; ++i) { out.dof_M0[i] = M[i * nv + i]; trace += M[i * nv + i]; }
  out.meaninertia = nv > 0 ? trace / nv : 1;
  // inverse of M (dense Cholesky) for invweight0
  std::vector<double>& Minv = out.Minv;
  Minv.assign(nv * nv, 0);
  if (nv > 0) dense_inverse_spd(M, Minv, nv);
  out.dof_invweight0.assign(nv, 0);
  for (int j = 0; j < m.njnt; ++j) {
    int d = m.jnt_dofadr[j];
    switch (m.jnt_type[j]) {
      case MRS_JNT_FREE: {
        double t = (Minv[d * nv + d] + Minv[(d + 1) * nv + d + 1] + Minv[(d + 2) * nv + d + 2]) / 3;
        double r = (Minv[(d + 3) * nv + d + 3] + Minv[(d + 4) * nv + d + 4] + Minv[(d + 5) * nv + d + 5]) / 3;
        for (int k = 0; k < 3; ++k) { out.dof_invweight0[d + k] = t; out.dof_invweight0[d + 3 + k] = r; }
        break;
      }
      case MRS_JNT_BALL: {
        double r = (Minv[d * nv + d] + Minv[(d + 1) * nv + d + 1] + Minv[(d + 2) * nv + d + 2]) / 3;
        for (int k = 0; k < 3; ++k) out.dof_invweight0[d + k] = r;
        break;
      }
      default: out.dof_invweight0[d] = Minv[d * nv + d];
    }
  }
  // body_invweight0: mean diagonal of J M^-1 J' (translation, rotation) at the body com
  out.body_invweight0.assign(2 * nb, 0);
  for (int b = 1; b < nb; ++b) {
    if (m.body_weldid[b] == 0) continue;
    std::vector<double> J(6 * nv, 0);  // rows 0-2 translation, 3-5 rotation
    for (int j = nv - 1; j >= 0; --j) {
      // dof j affects body b if dof j's body is b or an ancestor of b
      bool affects = false;
      for (int x = b; x != 0; x = m.body_parentid[x])
        if (x == m.dof_bodyid[j]) { affects = true; break; }
      if (!affects) continue;
      double off[3];
      for (int i = 0; i < 3; ++i) off[i] = xipos[3 * b + i] - scom[3 * m.body_rootid[b] + i];
      double cr[3];
      cross3(cr, &cdof[6 * j], off);
      for (int i = 0; i < 3; ++i) {
        J[i * nv + j] = cdof[6 * j + 3 + i] + cr[i];
        J[(3 + i) * nv + j] = cdof[6 * j + i];
      }
    }
    double A[6] = {0};
    for (int r = 0; r < 6; ++r)
      for (int a = 0; a < nv; ++a)
        for (int c = 0; c < nv; ++c) A[r] += J[r * nv + a] * Minv[a * nv + c] * J[r * nv + c];
    double t = (A[0] + A[1] + A[2]) / 3, r = (A[3] + A[4] + A[5]) / 3;
    // a body that can only translate or only rotate borrows the other weight
    if (t < kMinVal) t = r;
    if (r < kMinVal) r = t;
    out.body_invweight0[2 * b] = t;
    out.body_invweight0[2 * b + 1] = r;
  }
}

// translational Jacobian [3][nv] at qpos0 of the world point p on body b (mj_jac's jacp): the columns of
// the dofs of b and its ancestors, cdof's linear part plus its angular part crossed with the offset from
// the tree's com
inline void point_jacp(const Model& m, const InertialConst& c, int b, const double p[3], std::vector<double>& jacp) {
  const int nv = m.nv;
  jacp.assign(3 * std::max(1, nv), 0.0);
  double off[3];
  for (int i = 0; i < 3; ++i) off[i] = p[i] - c.scom[3 * m.body_rootid[b] + i];
  for (int x = b; x != 0; x = m.body_parentid[x])
    for (int j = m.body_dofadr[x]; j < m.body_dofadr[x] + m.body_dofnum[x]; ++j) {
      double cr[3];
      cross3(cr, &c.cdof[6 * j], off);
      for (int i = 0; i < 3; ++i) jacp[i * nv + j] = c.cdof[6 * j + 3 + i] + cr[i];
    }
}

// mj_tendon at qpos0 for a path of sites and pulleys (wraps [adr, adr + num) of m.wrap_*): the length
// sum_seg w |p1 - p0| and the Jacobian sum_seg w dir' (jacp(site1) - jacp(site0)) [nv], w = 1 / divisor
// of the last pulley before the segment (1 before the first); a segment within one body adds length only
inline double spatial_tendon0(const Model& m, const InertialConst& c, int adr, int num, std::vector<double>& J) {
  const int nv = m.nv;
  J.assign(std::max(1, nv), 0.0);
  double len = 0, w = 1;
  auto site_world = [&](int sid, double p[3]) {
    const int b = m.site_bodyid[sid];
    rot_vec_quat(p, &m.site_pos[3 * sid], &c.xquat[4 * b]);
    for (int i = 0; i < 3; ++i) p[i] += c.xpos[3 * b + i];
  };
  std::vector<double> j0, j1;
  for (int k = adr; k < adr + num; ++k) {
    if (m.wrap_type[k] == MRS_WRAP_PULLEY) { w = 1 / m.wrap_prm[k]; continue; }
    if (k + 1 >= adr + num || m.wrap_type[k + 1] != MRS_WRAP_SITE) continue;
    const int s0 = m.wrap_objid[k], s1 = m.wrap_objid[k + 1];
    double p0[3], p1[3], d[3];
    site_world(s0, p0);
    site_world(s1, p1);
    for (int i = 0; i < 3; ++i) d[i] = p1[i] - p0[i];
    const double n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    len += w * n;
    if (m.site_bodyid[s0] == m.site_bodyid[s1]) continue;
    if (n < kMinVal) { d[0] = 1; d[1] = d[2] = 0; }  // (mju_normalize3 of a null vector)
    else for (int i = 0; i < 3; ++i) d[i] /= n;
    point_jacp(m, c, m.site_bodyid[s0], p0, j0);
    point_jacp(m, c, m.site_bodyid[s1], p1, j1);
    for (int j = 0; j < nv; ++j)
      for (int i = 0; i < 3; ++i) J[j] += w * d[i] * (j1[i * nv + j] - j0[i * nv + j]);
  }
  return len;
}

// mj_transmission's mjTRN_SITE branch (no refsite) at qpos0: the moment [nv] of an actuator on site sid
// with the six gear numbers g in the site's frame, moment_j = R g[0:3] . jacp_j + R g[3:6] . jacr_j --
// jacp of the site's world position on its body, jacr the angular half of cdof for the dofs of that
// body and its ancestors.  A site on the world (or welded to it) gets zeros
inline void site_moment0(const Model& m, const InertialConst& c, int sid, const double g[6], std::vector<double>& mom) {
  const int nv = m.nv, b = m.site_bodyid[sid];
  mom.assign(std::max(1, nv), 0.0);
  double p[3], l[3], wl[3], wr[3];
  rot_vec_quat(p, &m.site_pos[3 * sid], &c.xquat[4 * b]);
  for (int i = 0; i < 3; ++i) p[i] += c.xpos[3 * b + i];
  rot_vec_quat(l, g, &m.site_quat[4 * sid]);
  rot_vec_quat(wl, l, &c.xquat[4 * b]);
  rot_vec_quat(l, g + 3, &m.site_quat[4 * sid]);
  rot_vec_quat(wr, l, &c.xquat[4 * b]);
  std::vector<double> jacp;
  point_jacp(m, c, b, p, jacp);
  for (int j = 0; j < nv; ++j)
    for (int i = 0; i < 3; ++i) mom[j] += wl[i] * jacp[i * nv + j];
  for (int x = b; x != 0; x = m.body_parentid[x])
    for (int j = m.body_dofadr[x]; j < m.body_dofadr[x] + m.body_dofnum[x]; ++j)
      for (int i = 0; i < 3; ++i) mom[j] += wr[i] * c.cdof[6 * j + i];
}

}  // namespace setconst
}  // namespace mrs
