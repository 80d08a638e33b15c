// The launch plan of a batch: group width, workgroup shape, helper waves, the ray paths and the LDS /
// scratch layouts, chosen from the model, the tables' counts (devtables.h), the batch size and the
// device's CU count.  Host only, no HIP, pure functions: the same inputs give the same plan with or
// without a device (mrs_debug_plan_layout).
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "devtables.h"

namespace mrs {

// --- LDS layout (floats) of one env.  Dense mode: M and its factor as nv x nv.  Blocked mode (one env
// per wave, G = 64): M and its factor per kinematic tree, row forces and the island scratch of the
// sparse constraint solver.  want_lh: the slot of the integrator's factor (helper waves, fuse_ih)
inline LdsLayout lds_layout(const Model& m, const DevModel& d, bool blocked, bool want_lh) {
  LdsLayout L{};
  int off = 0;
  auto take = [&](int n) { int o = off; off += n; off = (off + 3) & ~3; return o; };
  const int nb = m.nbody, nj = std::max(1, m.njnt), nv = std::max(1, m.nv), ng = std::max(1, m.ngeom);
  L.xpos = take(3 * nb); L.xquat = take(4 * nb); L.xmat = take(9 * nb); L.xipos = take(3 * nb);
  L.xanchor = take(3 * nj); L.xaxis = take(3 * nj); L.gxpos = take(3 * ng); L.gxmat = take(9 * ng);
  L.scom = take(3 * nb); L.cinert = take(10 * nb); L.crb = d.acc_sens ? take(10 * nb) : 0; L.cdof = take(6 * nv);
  L.cdofdot = take(6 * nv); L.cvel = take(6 * nb); L.cacc = take(6 * nb); L.cfrc = take(6 * nb);
  // without accelerometer / force / torque sensors (no rne_post), crb shares cacc + cfrc (12 nb):
  // CRBA's composite inertias are dead before mj_rne starts, and mj_rne's subtree force sums
  // (6 per body at crb) overwrite only cacc, which is dead once cfrc is built
  if (!d.acc_sens) L.crb = L.cacc;
  const int msize = blocked ? std::max(1, d.nMblk) : nv * nv;
  L.M = take(msize); L.L = take(msize); L.qpos = take(std::max(1, m.nq)); L.qvel = take(nv);
  L.ctrl = take(std::max(1, m.nu)); L.qfrc_applied = take(nv); L.qacc_ws = take(nv); L.qfrc_bias = take(nv);
  L.qfrc_passive = take(nv); L.qfrc_act = take(nv); L.qfrc_smooth = take(nv); L.qacc_smooth = take(nv);
  L.qacc = take(nv + 1); L.qfrc_con = take(nv + 1);  // + a dummy word (blocked-mode solver)
  L.act_force = take(std::max(1, m.nu));
  // tendon lengths and velocities of the step; behind them the site actuators' (DevModel::nact_site: 0
  // and their velocity, slot ntendon + k), which only a model with a site actuator takes
  L.ten = d.ntendon + d.nact_site > 0 ? take(2 * (d.ntendon + d.nact_site)) : 0;
  L.niter = take(1);
  L.hcon = take(1);
  L.Lh = want_lh ? take(nv * nv) : 0;
  L.rfmask = take(std::max(1, d.nrfblk));
  L.trees = blocked ? take(4 * std::max(1, d.ntree)) : 0;
  L.dofb = blocked ? take(2 * nv) : 0;
  // primal solvers in blocked mode: H = M + J'DJ couples the trees a contact joins, so it is
  // stored dense (dense mode builds H in the factor slot L.L instead)
  L.H = blocked && m.solver != MRS_SOL_PGS ? take(nv * nv) : 0;
  L.Li = blocked && m.solver == MRS_SOL_PGS ? take(std::max(1, d.nMblk)) : 0;
  L.rk = m.integrator == MRS_INT_RK4 ? take(std::max(1, m.nq) + 4 * nv) : 0;
  L.act = m.na > 0 ? take(4 * m.na) : 0;
  L.mocap = m.nmocap > 0 ? take(7 * m.nmocap) : 0;
  // the spatial tendons' Jacobian rows of the step, the layout's last extent (DevModel::lds_tenJ, lds_tenj())
  if (d.nten_spatial > 0) take(d.nten_spatial * nv);
  L.total = off;
  return L;
}

// offset of the spatial tendons' Jacobian slot [nten_spatial][nv] in the layout L of lds_layout (its last
// extent); 0 without spatial tendons
inline int lds_tenj(const Model& m, const DevModel& d, const LdsLayout& L) {
  return d.nten_spatial > 0 ? L.total - ((d.nten_spatial * std::max(1, m.nv) + 3) & ~3) : 0;
}

// workgroup-shared tables (DevModel::shr_*, offsets in floats from shr_off): ray-geom records, the
// per-ray direction + address when every ray starts at one point of one body (rf_common), the rays'
// static hits (rf_mode 2), then the records in the order below.  Returns d with the offsets for its
// rf_common and rf_mode.  The smooth-dynamics tables (from shr_act on) are staged only by lane-group
// kernels (G < 64); blocked mode (one env per workgroup) reads them from the model block instead of
// paying their LDS per env: its tables end at shr_act
inline DevModel shared_layout(const Model& m, DevModel d) {
  d.shr_rf = d.nrgeom * 8;
  d.shr_rfst = d.shr_rf + (d.rf_common ? 4 * d.nrf : 0);
  d.shr_blk = d.shr_rfst + (d.rf_mode == 2 ? d.nrf : 0);
  d.shr_sens = d.shr_blk + 17 * d.nrfblk;
  d.shr_fric = d.shr_sens + 16 * d.nsens_other + 32 * d.nsens_more;
  d.shr_lim = d.shr_fric + 4 * d.nfric;
  d.shr_act = d.shr_lim + 4 * d.nlim;
  d.shr_dof = d.shr_act + 20 * m.nu;
  d.shr_body = d.shr_dof + 16 * m.nv;
  d.shr_mpair = d.shr_body + 8 * m.nbody;
  d.shr_jump = d.shr_mpair + 4 * d.nMpair;
  d.shr_kbody = d.shr_jump + d.njump * m.nbody;
  d.shr_kjnt = d.shr_kbody + 25 * m.nbody;
  d.shr_kgeom = d.shr_kjnt + 13 * m.njnt;
  d.shr_flag = d.shr_kgeom + 9 * m.ngeom;  // (helper waves' signal words, one per physics wave)
  d.shr_total = d.shr_flag + 4;
  return d;
}

// --- scratch layout (floats) of one env.  Dense mode: rows J and M^-1 J' as nefc x nv plus per-row
// scalars; blocked mode: one record per row in solver order (J, M^-1 J' and dof per pipe slot, scalars)
inline ScratchLayout scratch_layout(const Model& m, const DevModel& d, bool blocked) {
  ScratchLayout S{};
  int off = 0;
  auto take = [&](int n) { int o = off; off += n; off = (off + 3) & ~3; return o; };
  const int nv = std::max(1, m.nv), ne = std::max(1, d.max_efc);
  // dense rows: dense mode, and blocked mode with a primal solver (the sparse records are PGS's)
  const int dn = blocked && m.solver == MRS_SOL_PGS && m.cone != MRS_CONE_ELLIPTIC && d.xrows == 0 ? 0 : ne;
  S.efc_J = take(dn * nv); S.efc_MJ = take(dn * nv); S.efc_type = take(ne); S.efc_pos = take(ne);
  S.efc_margin = take(ne); S.efc_floss = take(ne); S.efc_R = take(dn); S.efc_aref = take(dn);
  S.efc_b = take(dn); S.efc_f = take(ne); S.efc_ARii = take(dn); S.con = take(kConRec * std::max(1, d.max_con));
  S.efc_rec = take(blocked ? ne * (2 * d.pipe_w + 12) : 0);  // step.hip RF
  S.efc_rowof = take(blocked ? ne : 0);
  S.efc_item = take(blocked ? ne : 0);
  S.efc_fq = take(blocked ? ne : 0);
  S.efc_hdr = take(blocked ? 24 * ne : 0);  // step.hip kHdr
  S.efc_quad = take(blocked ? 64 : 0);
  S.efc_fd = take(m.cone == MRS_CONE_ELLIPTIC && m.solver == MRS_SOL_PGS ? 2 * ne : 0);  // (16-byte aligned)
  // <= 64 lanes x 8 contacts x 7 floats (max_con > 0: the static filter admits a pair, walked or not)
  S.stage = take(d.max_con > 0 ? 64 * kMaxPairCon * 7 : 0);
  S.efc_n = take(1);
  S.sens = take(std::max(1, m.nsensordata));
  S.xfrc = take(1);
  S.total = off;
  return S;
}

struct Plan {
  int group = 64;      // lanes per environment in the step kernel (64 / group envs per wavefront)
  int g16_one_wg = 0;  // G = 16 with one workgroup per CU (tables past the two-per-CU budget)
  int wpb16 = WavesPerBlock<16>::value;  // waves per workgroup of the G = 16 kernels (DevState::wpb16)
  int helpers = 0;     // helper waves (DevState::ray_helpers)
  bool ext = false;    // the extended step kernels (step/base.h MRS_EXT)
  bool want_lh = false;  // L has the integrator factor's slot (L.Lh)
  // the tables' DevModel with the plan's fields filled in: L, S, shr_*, blocked, fuse_ih, rf_common,
  // rf_mode, rf_sweep and the sweep's fan rf_sw* (all zero without it); the pointers still null
  DevModel dm{};
};

// Ray sweep (step.hip rays_sweep): a static lidar over a static world (rf_mode 2) whose rays are one
// planar, evenly spaced fan from one point -- what <replicate> builds -- and whose sensordata slots
// are consecutive.  Each step then computes, per moving ray geom, the interval of ray indices its
// bounding sphere can reach, copies the static hit of every ray in no interval and traces only the
// rows of G rays that meet one.  The fan is fitted in fp64 over all rays, as the block fit does per
// block; ray k must lie within a quarter increment of phi0 + k dphi.  Fills d.rf_sw* when it fits
inline void fit_ray_sweep(const Model& m, const DevTables& T, DevModel& d) {
  const float *rgeom = T.table(&DevModel::rgeom), *rfray = T.table(&DevModel::rfray), *rfblk = T.table(&DevModel::rfblk);
  bool ok = true;
  for (int i = 0; i < d.nrgeom; ++i)
    if (!((d.rf_static_mask >> i) & 1u) && bits_int(rgeom[8 * i + 1]) == MRS_GEOM_MESH) ok = false;
  const int adr0 = m.sensor_adr[T.rf[0]];
  for (int k = 0; k < d.nrf; ++k) ok = ok && m.sensor_adr[T.rf[k]] == adr0 + k;
  // (the directions the kernel traces: rfray, world frame)
  auto dir = [&](int k, double v[3]) { for (int i = 0; i < 3; ++i) v[i] = rfray[8 * k + i]; };
  double cov[3][3] = {}, c[3] = {0, 0, 1}, a[3], bv[3], d0[3];
  for (int k = 0; k < d.nrf; ++k) {
    double v[3];
    dir(k, v);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) cov[i][j] += v[i] * v[j];
  }
  smallest_eigvec(cov, c);
  dir(0, d0);
  const double cd = c[0] * d0[0] + c[1] * d0[1] + c[2] * d0[2];
  for (int i = 0; i < 3; ++i) a[i] = d0[i] - cd * c[i];
  const double an = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  const double cn = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  if (an < 0.5 || cn < 0.5) ok = false;
  if (!ok) return;
  double dphi = 0, eps = 0;
  for (int i = 0; i < 3; ++i) { a[i] /= an; c[i] /= cn; }
  auto cross_ca = [&]() {
    bv[0] = c[1] * a[2] - c[2] * a[1];
    bv[1] = c[2] * a[0] - c[0] * a[2];
    bv[2] = c[0] * a[1] - c[1] * a[0];
  };
  cross_ca();
  double d1[3];
  dir(1, d1);
  if (d1[0] * bv[0] + d1[1] * bv[1] + d1[2] * bv[2] < 0) {  // the sweep runs counter-clockwise about c
    for (int i = 0; i < 3; ++i) c[i] = -c[i];
    cross_ca();
  }
  // unwrapped in-plane angles (phi0 = 0: a is ray 0), each increment in (0, pi)
  std::vector<double> phi(d.nrf, 0.0);
  for (int k = 0; k < d.nrf; ++k) {
    double v[3];
    dir(k, v);
    const double da = v[0] * a[0] + v[1] * a[1] + v[2] * a[2], db = v[0] * bv[0] + v[1] * bv[1] + v[2] * bv[2];
    eps = std::max(eps, std::abs(v[0] * c[0] + v[1] * c[1] + v[2] * c[2]));
    if (k == 0) continue;
    const double kPi = 3.14159265358979323846;
    double inc = std::atan2(db, da) - std::fmod(phi[k - 1], 2 * kPi);
    while (inc <= 0) inc += 2 * kPi;
    if (inc >= kPi) ok = false;
    phi[k] = phi[k - 1] + inc;
  }
  const double kTwoPi = 6.28318530717958647692;
  dphi = phi[d.nrf - 1] / (d.nrf - 1);
  // (increments fine enough for fp32 angles to stay well inside the one-ray margin of the intervals)
  if (!(dphi >= 5e-3) || dphi > 0.5 || eps > 1e-3) ok = false;
  for (int k = 0; k < d.nrf && ok; ++k) ok = std::abs(phi[k] - k * dphi) <= 0.25 * dphi;
  // no ray direction twice: the fan ends before ray 0 comes round again
  if (ok && (d.nrf - 1) * dphi > kTwoPi - 0.5 * dphi) ok = false;
  if (!ok) return;
  d.rf_sw_full = std::abs(d.nrf * dphi - kTwoPi) <= 0.25 * dphi ? 1 : 0;
  d.rf_sw_plo = static_cast<int>(std::floor(kTwoPi / dphi));
  d.rf_sw_phi = static_cast<int>(std::ceil(kTwoPi / dphi));
  d.rf_sw_n = d.nrf;
  d.rf_sw_adr0 = adr0;
  for (int i = 0; i < 3; ++i) {
    d.rf_sw[i] = rfblk[2 + i];  // the origin every pass traces from (and level 1 tests against)
    d.rf_sw[3 + i] = static_cast<float>(a[i]);
    d.rf_sw[6 + i] = static_cast<float>(bv[i]);
    d.rf_sw[9 + i] = static_cast<float>(c[i]);
  }
  d.rf_sw[12] = 0.0f;
  d.rf_sw[13] = static_cast<float>(1.0 / dphi);
  d.rf_sw[14] = static_cast<float>(eps + 1e-6);
  d.rf_sw[15] = static_cast<float>(kTwoPi / dphi);
  d.rf_sweep = 1;
}

// cu_count: the device's compute units; <= 0 (unknown) keeps four-wave workgroups and lets the helper
// waves' fit test pass
inline Plan choose_plan(const Model& m, const DevTables& T, int n_envs, int cu_count, const Overrides& o) {
  Plan p;
  DevModel& d = p.dm;
  d = T.dm;  // (rf_common: every ray block a fan from one point of one body, which the plan may give up)
  d.L = lds_layout(m, d, false, false);
  // static ray split: every rangefinder on a body fixed in the world and some ray geom on one too
  d.rf_mode = d.nrfblk > 0 && T.rf_fixed && d.rf_static_mask && !o.no_static_rays ? 2 : 0;
  d = shared_layout(m, d);
  // lanes per environment: the narrowest group that still gives every dof its own lane (the
  // dense M / Cholesky / PGS phases are lane-per-dof) and keeps a workgroup's LDS within 80 KB
  // (two workgroups per CU); MRS_GROUP overrides (8, 16, 32 or 64)
  auto lds_bytes = [&](const DevModel& s, int g) {
    return (static_cast<size_t>(d.L.total) * envs_per_block(g) + (g == 64 ? s.shr_act : s.shr_total)) * sizeof(float);
  };
  // (narrow groups win even when they leave CUs idle: C4's 2048 envs run a 10-step launch in
  // 1.33 ms at G = 16 on 128 workgroups vs 4.0 ms at G = 64 on 512)
  for (int g : {32, 16})
    if (m.nv <= g && lds_bytes(d, g) <= 80 * 1024) p.group = g;
  // a 16-lane model whose workgroup tables outgrow the two-per-CU budget (a dense lidar: the per-ray
  // direction table is 16 B per ray) keeps its 16-lane groups rather than dropping to 32 (~4x slower
  // on C3): the per-ray table moves out of LDS (rays read from the model block, L1/L2-resident: the
  // pass's non-common path).  MRS_G16_ONE_WG also allows one workgroup per CU (up to 160 KB)
  if (p.group > 16 && m.nv <= 16) {
    // drop the common-frame ray table only if that is what lets the 16-lane layout fit; otherwise
    // the model keeps its wider groups and the table (no silent slowdown of the ray pass)
    DevModel without = d;
    without.rf_common = 0;
    without = shared_layout(m, without);
    if (d.rf_common && lds_bytes(without, 16) <= 80 * 1024) {
      p.group = 16;
      d = without;
    }
    // (one 160 KB workgroup per CU was measured slower than 32-lane groups on the mesh robot: 27 vs
    // 15 ms per 10-step launch -- a single wave per SIMD cannot hide its memory latency)
    if (p.group > 16 && lds_bytes(d, 16) <= 160 * 1024 && o.g16_one_wg) { p.group = 16; p.g16_one_wg = 1; }
  }
  if ((o.group == 8 || o.group == 16 || o.group == 32 || o.group == 64) && m.nv <= o.group) p.group = o.group;
  // G = 16 with fewer waves than the device has SIMDs (C4: 2048 envs = 512 waves on 1024 SIMDs):
  // one-wave workgroups, so the waves spread over every CU instead of filling half of them four to
  // a CU (measured C4: 0.802 vs 0.822 ms per launch; C3 and C2 have a wave per SIMD or more and keep
  // four-wave workgroups -- C3's LDS tables per workgroup would cost it residency).  MRS_G16_WPB
  // overrides (1, 2 or 4)
  const long waves = (static_cast<long>(n_envs) * 16 + 63) / 64;
  if (p.group == 16 && !p.g16_one_wg) {
    if (cu_count > 0 && waves < 4L * cu_count) p.wpb16 = 1;
    if (o.g16_wpb == 1 || o.g16_wpb == 2 || o.g16_wpb == 4)
      p.wpb16 = std::min(o.g16_wpb, static_cast<int>(WavesPerBlock<16>::value));
  }
  // extended step kernels (step/base.h MRS_EXT) for models with general convex (MPR) pairs -- a pair
  // that is not plane-* and has an ellipsoid, cylinder or mesh (narrowphase's analytic routines cover
  // the rest) -- or rangefinders over more than 32 ray geoms
  // (DevTables::convex_pairs: of the full pair list, so pruning never changes the kernel)
  p.ext = (d.nrgeom > 32 && d.nrf > 0) || T.convex_pairs;
  // helper waves: with one-wave workgroups (fewer waves than SIMDs, so the helpers take SIMDs that
  // would idle) every physics wave gets a second wave that runs its envs' collision pass, builds their
  // constraint rows, traces their rangefinders and factors the integrator's M + h D each step while it
  // runs the dynamics (step_kernel); models with rangefinders (<= 32 ray geoms) without RK4 and
  // without the extended kernels only.  MRS_RAY_HELPERS=0 turns them off.
  // (the helper kernels run at one wave per SIMD, step.hip MRS_HELPER_OCC: physics plus helper
  // waves must fit the device's SIMDs at once, i.e. at most two physics waves per CU)
  const bool fit = cu_count <= 0 || waves <= 2L * cu_count;
  p.helpers = o.ray_helpers && fit && p.group == 16 && p.wpb16 == 1 && !p.ext && d.nrf > 0 && d.nrgeom <= 32 &&
              m.integrator != MRS_INT_RK4 && !(m.disableflags & MRS_DSBL_SENSOR) ? 1 : 0;
  // the integrator factor slot (implicit-damping Euler and implicitfast; the full implicit
  // integrator factors its own LU)
  p.want_lh = p.helpers && m.integrator != MRS_INT_IMPLICIT;
  // the integrator's M + h D factored together with M (step.hip cholesky_ih): into M's own LDS slot
  // for PGS models, which no longer read M after the factor, into the L.Lh slot for Newton / CG
  // (their primal solve multiplies by M).  16-lane groups without helper waves (they factor it on the
  // helper), implicitfast, and no force-limited actuator (their velocity derivative depends on the
  // step's actuator forces, which come after the factor).  MRS_NO_FUSE_IH=1 factors it in integrate()
  // instead (A/B)
  bool flim = false;
  for (int a = 0; a < m.nu; ++a) flim |= m.actuator_forcelimited[a] != 0;
  d.fuse_ih = p.group == 16 && !p.helpers && m.integrator == MRS_INT_IMPLICITFAST && !flim && m.nv <= 16 &&
              !o.no_fuse_ih ? 1 : 0;
  if (d.fuse_ih && m.solver != MRS_SOL_PGS && !p.want_lh) {
    // (when the extra nv x nv slot does not fit the workgroup's LDS: factor in integrate())
    const size_t with_lh = static_cast<size_t>(lds_layout(m, d, false, true).total) * envs_per_block(p.group, p.wpb16) + d.shr_total;
    if (with_lh * sizeof(float) > 160 * 1024) d.fuse_ih = 0;
    else p.want_lh = true;
  }
  // the 16-lane register solves with one reciprocal per lane and qacc_smooth solved with the
  // friction-loss rows (step.hip chol_solve_rows16, pgs_small16_qacc): PGS batches without helper
  // waves.  MRS_NO_SOLVE_FUSE=1: the separate solves with a divide per level, out of line (a reference
  // for the bits, not for speed)
  d.solve_fuse = p.group == 16 && m.solver == MRS_SOL_PGS && !p.helpers && !o.no_solve_fuse ? 1 : 0;
  // the helper-wave kernels keep the block passes.  MRS_NO_RAY_SWEEP=1 forces them (A/B)
  if (d.rf_mode == 2 && d.rf_common && d.rf_static_frame && d.nrgeom <= 32 && (p.group == 16 || p.group == 32) &&
      !p.helpers && d.nrf >= 3 && (d.nrf + p.group - 1) / p.group <= 32 && !o.no_ray_sweep)
    fit_ray_sweep(m, T, d);
  d.blocked = p.group == 64 ? 1 : 0;
  if (d.blocked) d.shr_total = d.shr_act;
  d.L = lds_layout(m, d, d.blocked != 0, p.want_lh);
  d.lds_tenJ = lds_tenj(m, d, d.L);
  d.shr_off = d.L.total * envs_per_block(p.group, p.wpb16);
  if ((static_cast<size_t>(d.shr_off) + d.shr_total) * sizeof(float) > 160 * 1024)
    throw UnsupportedError("model too large for the per-environment LDS working set");
  d.S = scratch_layout(m, d, d.blocked != 0);
  return p;
}

// the first 16 values of mrs_debug_batch_layout (mrs.h), the ones a plan decides
constexpr int kPlanLayoutValues = 16;
inline void plan_layout_values(const DevModel& d, int group, int g16_one_wg, int wpb16, int helpers, int v[kPlanLayoutValues]) {
  const int x[kPlanLayoutValues] = {group, d.L.total, d.S.total, d.blocked, d.pipe_w, d.max_efc, d.max_con, d.ntree,
                                    d.shr_total, d.rf_common, g16_one_wg, group == 16 ? wpb16 : 0, helpers, d.fuse_ih,
                                    d.rf_sweep, d.sens_every};
  std::copy(x, x + kPlanLayoutValues, v);
}

}  // namespace mrs
