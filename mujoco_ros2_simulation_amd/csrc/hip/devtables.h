// The compiled model as the flat tables the kernels read: one fp32 block and one int32 block, the
// DevModel counts derived while packing them, and the A/B switches of batch creation.  Host only, no
// HIP: batch.hip uploads the blocks and patches their device addresses into DevModel, plan.h chooses the
// launch plan from the counts, and tests/sanitize/driver.cc checks every offset and index here against
// its range, since the kernels read these tables without a bounds check.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/mrs.h"
#include "../mjcf/model.h"
#include "batch.h"
#include "devmodel.h"
#include "renderplan.h"
#include "start_rows.h"

namespace mrs {

// ------------------------------------------------------------------ overrides
// The environment switches of batch creation (tests and A/B runs; none is set in a measured run).
// read_overrides() is the one place that reads them, once per batch: tests flip them between batches.
// The render switches (MRS_DEPTH_V1, MRS_DEPTH_V2, MRS_RAST_BUDGET_MB) are read per render call by
// renderplan.h's read_render_overrides() and are not part of a batch's tables or plan.
struct Overrides {
  int group = 0;             // MRS_GROUP: lanes per env (8, 16, 32 or 64, when nv allows); 0: the plan's choice
  int g16_wpb = 0;           // MRS_G16_WPB: waves per workgroup of a 16-lane batch (1, 2 or 4); 0: the plan's
  bool g16_one_wg = false;   // MRS_G16_ONE_WG: allow 16 lanes with one workgroup per CU (up to 160 KB of LDS)
  bool ray_helpers = true;   // MRS_RAY_HELPERS=0: no helper waves
  bool no_fuse_ih = false;   // MRS_NO_FUSE_IH: factor M + h D in integrate(), not beside M
  // MRS_NO_SOLVE_FUSE: the 16-lane solves separate, a divide per level (DevModel::solve_fuse).  A
  // bit-identity reference only, not a speed baseline: the separate form then runs out of line, slower
  // than it ran before the fused form existed
  bool no_solve_fuse = false;
  // MRS_NO_TABLE_IMAGE: the launch stages the workgroup-shared tables one by one (DevModel::shr_image
  // null).  A bit-identity reference only, like MRS_NO_SOLVE_FUSE: that form runs out of line
  bool no_table_image = false;
  bool no_ray_sweep = false; // MRS_NO_RAY_SWEEP: a static planar lidar keeps the block passes
  bool no_pair_prune = false;  // MRS_NO_PAIR_PRUNE: the device walks every statically admissible pair (prune_pairs)
  bool no_static_rays = false;   // MRS_NO_STATIC_RAYS: no static ray split (rf_mode 0)
  bool no_static_frame = false;  // MRS_NO_STATIC_FRAME: ray tables stay in the body frame
  bool kin_twopass = false;  // MRS_KIN_TWOPASS: the kinematics' joint frames from a second pass
  int sparse_off = 0;        // MRS_SPARSE_OFF: sparse solver paths switched off (DevModel::sparse_off bits)
  int diag_skip = 0;         // MRS_DIAG_SKIP: profiling ablation (bit 0 sensors, 1 collision, 2 constraints)
  bool sensors_every_step = false;  // MRS_SENSORS_EVERY_STEP=1: every step of a fused launch stores the sensors
  bool no_multiccd = false;  // MRS_NO_MULTICCD: sets MRS_RESTATE_NO_MULTICCD (A/B of the face contacts)
  bool no_bvh = false;       // MRS_NO_BVH: no mesh hierarchy, every triangle is tested
  int bvh_leaf = 4;          // MRS_BVH_LEAF: triangles per hierarchy leaf (1..64)
  bool bvh_median = false;   // MRS_BVH_MEDIAN: median splits instead of the surface-area heuristic
  int spread = 0;            // MRS_SPREAD: 2^spread lane groups per env (0..3)
};

inline Overrides read_overrides() {
  auto set = [](const char* name) { return std::getenv(name) != nullptr; };
  auto num = [](const char* name, int absent) { const char* e = std::getenv(name); return e ? std::atoi(e) : absent; };
  Overrides o;
  o.group = num("MRS_GROUP", 0);
  o.g16_wpb = num("MRS_G16_WPB", 0);
  o.g16_one_wg = set("MRS_G16_ONE_WG");
  o.ray_helpers = num("MRS_RAY_HELPERS", 1) != 0;
  o.no_fuse_ih = set("MRS_NO_FUSE_IH");
  o.no_solve_fuse = set("MRS_NO_SOLVE_FUSE");
  o.no_table_image = set("MRS_NO_TABLE_IMAGE");
  o.no_ray_sweep = set("MRS_NO_RAY_SWEEP");
  o.no_pair_prune = set("MRS_NO_PAIR_PRUNE");
  o.no_static_rays = set("MRS_NO_STATIC_RAYS");
  o.no_static_frame = set("MRS_NO_STATIC_FRAME");
  o.kin_twopass = set("MRS_KIN_TWOPASS");
  o.sparse_off = num("MRS_SPARSE_OFF", 0) & 15;
  o.diag_skip = num("MRS_DIAG_SKIP", 0);
  o.sensors_every_step = num("MRS_SENSORS_EVERY_STEP", 0) != 0;
  o.no_multiccd = set("MRS_NO_MULTICCD");
  o.no_bvh = set("MRS_NO_BVH");
  o.bvh_leaf = std::max(1, std::min(64, num("MRS_BVH_LEAF", 4)));
  o.bvh_median = set("MRS_BVH_MEDIAN");
  o.spread = std::max(0, std::min(3, num("MRS_SPREAD", 0)));
  return o;
}

// ------------------------------------------------------------------ the packed blocks
// restated limits of the render code (batch.hip asserts them against lit.h); the frame kernels' geom
// limit kDepthGeoms is renderplan.h's own
constexpr int kRlitHead = 12, kRlitLight = 24, kRlitMat = 12, kRlitTex = 16, kRlitMaxLights = 8;

template <class T>
struct Slot {
  CPtr<T> DevModel::*member;  // the DevModel pointer that addresses the table
  size_t off, len;            // first element in the block, elements (each table is padded to 4)
};

struct DevTables {
  // counts, options and table-derived flags; every pointer null.  The launch plan's fields (L, S,
  // shr_*, blocked, fuse_ih, rf_mode, rf_sweep, ...) are plan.h's; rf_common here is "every ray block is
  // a fan from one point of one body", which the plan may still give up
  DevModel dm{};
  std::vector<float> f;
  std::vector<int> i;
  std::vector<Slot<float>> fslot;
  std::vector<Slot<int>> islot;
  // host copies the batch keeps: the collision pairs the device walks (contact export: a contact record
  // holds an index into this list), their condim and sliding friction (contact forces)
  std::vector<int> pair_g1, pair_g2, pair_dim;
  std::vector<float> pair_mu;
  // statically admissible pairs left out of that list because they can never touch (prune_pairs), and
  // whether the full list has a general convex (MPR) pair: the plan reads the full list's properties
  int pairs_pruned = 0;
  bool convex_pairs = false;
  // what the plan reads again: rangefinder sensor ids, and whether every one sits on a body fixed in
  // the world
  std::vector<int> rf;
  bool rf_fixed = false;

  void addf(CPtr<float> DevModel::*dst, const std::vector<double>& v) {
    fslot.push_back({dst, f.size(), v.size()});
    for (double x : v) f.push_back(static_cast<float>(x));
    while (f.size() % 4) f.push_back(0);
  }
  void addf(CPtr<float> DevModel::*dst, const std::vector<float>& v) {
    fslot.push_back({dst, f.size(), v.size()});
    f.insert(f.end(), v.begin(), v.end());
    while (f.size() % 4) f.push_back(0);
  }
  void addi(CPtr<int> DevModel::*dst, const std::vector<int>& v) {
    islot.push_back({dst, i.size(), v.size()});
    i.insert(i.end(), v.begin(), v.end());
    while (i.size() % 4) i.push_back(0);
  }
  // a packed fp32 table on the host
  const float* table(CPtr<float> DevModel::*member) const {
    for (const auto& s : fslot)
      if (s.member == member) return f.data() + s.off;
    throw std::logic_error("table not packed");
  }
  // a packed int32 table on the host
  const int* itable(CPtr<int> DevModel::*member) const {
    for (const auto& s : islot)
      if (s.member == member) return i.data() + s.off;
    throw std::logic_error("table not packed");
  }
  // the tables' addresses once the blocks live at fbase / ibase
  void patch(DevModel& d, const float* fbase, const int* ibase) const {
    for (const auto& s : fslot) (d.*s.member).p = fbase + s.off;
    for (const auto& s : islot) (d.*s.member).p = ibase + s.off;
  }
};

inline float int_bits(int v) { float f; std::memcpy(&f, &v, sizeof f); return f; }
inline int bits_int(float f) { int v; std::memcpy(&v, &f, sizeof v); return v; }

// rotation matrix of a unit quaternion (row-major)
inline void quat_to_mat(const double q[4], double R[9]) {
  R[0] = q[0] * q[0] + q[1] * q[1] - q[2] * q[2] - q[3] * q[3]; R[1] = 2 * (q[1] * q[2] - q[0] * q[3]);
  R[2] = 2 * (q[1] * q[3] + q[0] * q[2]); R[3] = 2 * (q[1] * q[2] + q[0] * q[3]);
  R[4] = q[0] * q[0] - q[1] * q[1] + q[2] * q[2] - q[3] * q[3]; R[5] = 2 * (q[2] * q[3] - q[0] * q[1]);
  R[6] = 2 * (q[1] * q[3] - q[0] * q[2]); R[7] = 2 * (q[2] * q[3] + q[0] * q[1]);
  R[8] = q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3];
}

// unit ray direction of a rangefinder site in its body's frame: the z column of the site rotation
inline std::array<double, 3> site_z_axis(const Model& m, int site) {
  double R[9];
  quat_to_mat(&m.site_quat[4 * site], R);
  const double n = std::sqrt(R[2] * R[2] + R[5] * R[5] + R[8] * R[8]);
  return {R[2] / n, R[5] / n, R[8] / n};
}

// a body whose world pose is the same in every env for good: welded to the world and not on or below
// a mocap body (whose pose is per-env state)
inline bool fixed_in_world(const Model& m, int body) {
  return m.body_weldid[body] == 0 && m.body_mocapid[m.body_rootid[body]] < 0;
}

// world pose of a body without joints above it
inline void body_world(const Model& m, int b, double R[9], double p[3]) {
  double q[4] = {1, 0, 0, 0};
  p[0] = p[1] = p[2] = 0;
  std::vector<int> chain;
  for (int x = b; x != 0; x = m.body_parentid[x]) chain.push_back(x);
  for (auto it = chain.rbegin(); it != chain.rend(); ++it) {
    const double* bp = &m.body_pos[3 * *it];
    const double* bq = &m.body_quat[4 * *it];
    double Rq[9];
    quat_to_mat(q, Rq);
    for (int i = 0; i < 3; ++i) p[i] += Rq[3 * i] * bp[0] + Rq[3 * i + 1] * bp[1] + Rq[3 * i + 2] * bp[2];
    const double t[4] = {q[0] * bq[0] - q[1] * bq[1] - q[2] * bq[2] - q[3] * bq[3],
                         q[0] * bq[1] + q[1] * bq[0] + q[2] * bq[3] - q[3] * bq[2],
                         q[0] * bq[2] - q[1] * bq[3] + q[2] * bq[0] + q[3] * bq[1],
                         q[0] * bq[3] + q[1] * bq[2] - q[2] * bq[1] + q[3] * bq[0]};
    const double tn = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + t[3] * t[3]);
    for (int i = 0; i < 4; ++i) q[i] = t[i] / tn;
  }
  quat_to_mat(q, R);
}

// eigenvector of the smallest eigenvalue of a symmetric 3 x 3 matrix (cyclic Jacobi): the normal of
// a fan of directions from their sum d d'
inline void smallest_eigvec(const double cov[3][3], double c[3]) {
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  std::memcpy(A, cov, sizeof A);
  for (int sweep = 0; sweep < 50; ++sweep)
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (std::abs(A[p][q]) < 1e-15) continue;
        const double th = 0.5 * std::atan2(2 * A[p][q], A[q][q] - A[p][p]);
        const double cs = std::cos(th), sn = std::sin(th);
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = cs * akp - sn * akq; A[k][q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = cs * apk - sn * aqk; A[q][k] = sn * apk + cs * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq; V[k][q] = sn * vkp + cs * vkq;
        }
      }
  int imin = 0;
  for (int i = 1; i < 3; ++i) if (A[i][i] < A[imin][imin]) imin = i;
  for (int i = 0; i < 3; ++i) c[i] = V[i][imin];
}

// ------------------------------------------------------------------ mesh hierarchies
// Per-mesh bounding volume hierarchy for rays (rangefinders, depth and colour): a binary tree over a
// mesh's triangles in depth-first order; each node stores its AABB, inflated by 1e-5 of the mesh's
// extent so that the fp32 slab test never rejects a triangle that Moller-Trumbore hits, and the index
// of the node after its subtree (stackless traversal, raymesh.h).  Leaves hold up to 4 consecutive
// triangles of the mesh's device face list, which is reordered for it (face ids stay relative to the
// mesh's vertices; only ties between triangles at equal ray parameter can pick a different triangle).
// Meshes of at most 64 triangles keep no hierarchy: a wave tests their triangles with scalar loads.
inline void build_mesh_bvh(const Model& m, const Overrides& o, std::vector<int>& face_out, std::vector<float>& node,
                           std::vector<int>& adr, std::vector<int>& num) {
  face_out = m.mesh_face;
  const int nmesh = static_cast<int>(m.mesh_faceadr.size());
  adr.assign(std::max(1, nmesh), 0);
  num.assign(std::max(1, nmesh), 0);
  for (int k = 0; k < nmesh; ++k) {
    const int fa = m.mesh_faceadr[k], fn = m.mesh_facenum[k], va = m.mesh_vertadr[k];
    adr[k] = static_cast<int>(node.size() / 8);
    if (fn <= 64 || o.no_bvh) continue;
    struct Tri { double lo[3], hi[3], c[3]; int f[3]; };
    std::vector<Tri> tris(fn);
    double mlo[3] = {1e300, 1e300, 1e300}, mhi[3] = {-1e300, -1e300, -1e300};
    for (int f = 0; f < fn; ++f) {
      Tri& t = tris[f];
      for (int c = 0; c < 3; ++c) { t.lo[c] = 1e300; t.hi[c] = -1e300; t.f[c] = m.mesh_face[3 * (fa + f) + c]; }
      for (int v = 0; v < 3; ++v)
        for (int c = 0; c < 3; ++c) {
          const double x = m.mesh_vert[3 * (va + t.f[v]) + c];
          t.lo[c] = std::min(t.lo[c], x); t.hi[c] = std::max(t.hi[c], x);
        }
      for (int c = 0; c < 3; ++c) {
        t.c[c] = 0.5 * (t.lo[c] + t.hi[c]);
        mlo[c] = std::min(mlo[c], t.lo[c]); mhi[c] = std::max(mhi[c], t.hi[c]);
      }
    }
    const double pad = 1e-5 * std::max(1e-9, std::max(mhi[0] - mlo[0], std::max(mhi[1] - mlo[1], mhi[2] - mlo[2])));
    const int leaf = o.bvh_leaf;
    std::vector<float> nodes;
    std::function<void(int, int)> build = [&](int b, int e) {
      const int me = static_cast<int>(nodes.size() / 8);
      double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, clo[3] = {1e300, 1e300, 1e300},
             chi[3] = {-1e300, -1e300, -1e300};
      for (int i = b; i < e; ++i)
        for (int c = 0; c < 3; ++c) {
          lo[c] = std::min(lo[c], tris[i].lo[c]); hi[c] = std::max(hi[c], tris[i].hi[c]);
          clo[c] = std::min(clo[c], tris[i].c[c]); chi[c] = std::max(chi[c], tris[i].c[c]);
        }
      for (int c = 0; c < 3; ++c) nodes.push_back(static_cast<float>(lo[c] - pad));
      nodes.push_back(0);
      for (int c = 0; c < 3; ++c) nodes.push_back(static_cast<float>(hi[c] + pad));
      nodes.push_back(int_bits(-1));
      if (e - b <= leaf) {
        nodes[8 * me + 7] = int_bits((b << 8) | (e - b));
      } else {
        // binned surface-area heuristic (16 centroid bins per axis): the split minimising
        // N_left A_left + N_right A_right, i.e. the expected triangle tests of a ray that enters the
        // node; the median of the longest axis when no bin boundary separates the centroids
        constexpr int kBins = 16;
        auto area = [](const double* l, const double* h) {
          const double dx = h[0] - l[0], dy = h[1] - l[1], dz = h[2] - l[2];
          return dx * dy + dy * dz + dz * dx;
        };
        int best_ax = -1, best_s = 0;
        double best_cost = 1e300;
        for (int ax = 0; ax < 3; ++ax) {
          const double ext = chi[ax] - clo[ax];
          if (ext <= 1e-12) continue;
          int cnt[kBins] = {};
          double blo[kBins][3], bhi[kBins][3];
          for (int q = 0; q < kBins; ++q)
            for (int c = 0; c < 3; ++c) { blo[q][c] = 1e300; bhi[q][c] = -1e300; }
          for (int i = b; i < e; ++i) {
            const int q = std::min(kBins - 1, static_cast<int>((tris[i].c[ax] - clo[ax]) / ext * kBins));
            ++cnt[q];
            for (int c = 0; c < 3; ++c) { blo[q][c] = std::min(blo[q][c], tris[i].lo[c]); bhi[q][c] = std::max(bhi[q][c], tris[i].hi[c]); }
          }
          double rl[kBins][3], rh[kBins][3];
          int rn[kBins];
          for (int c = 0; c < 3; ++c) { rl[kBins - 1][c] = blo[kBins - 1][c]; rh[kBins - 1][c] = bhi[kBins - 1][c]; }
          rn[kBins - 1] = cnt[kBins - 1];
          for (int q = kBins - 2; q >= 0; --q) {
            rn[q] = rn[q + 1] + cnt[q];
            for (int c = 0; c < 3; ++c) { rl[q][c] = std::min(rl[q + 1][c], blo[q][c]); rh[q][c] = std::max(rh[q + 1][c], bhi[q][c]); }
          }
          double ll[3] = {1e300, 1e300, 1e300}, lh[3] = {-1e300, -1e300, -1e300};
          int ln = 0;
          for (int q = 1; q < kBins; ++q) {
            ln += cnt[q - 1];
            for (int c = 0; c < 3; ++c) { ll[c] = std::min(ll[c], blo[q - 1][c]); lh[c] = std::max(lh[c], bhi[q - 1][c]); }
            if (ln == 0 || rn[q] == 0) continue;
            const double cost = ln * area(ll, lh) + rn[q] * area(rl[q], rh[q]);
            if (cost < best_cost) { best_cost = cost; best_ax = ax; best_s = q; }
          }
        }
        int mid = (b + e) / 2;
        if (best_ax >= 0 && !o.bvh_median) {
          const double ext = chi[best_ax] - clo[best_ax];
          const int ax = best_ax, sp = best_s;
          const double lo0 = clo[ax];
          auto it = std::partition(tris.begin() + b, tris.begin() + e, [&](const Tri& t) {
            return std::min(kBins - 1, static_cast<int>((t.c[ax] - lo0) / ext * kBins)) < sp;
          });
          mid = static_cast<int>(it - tris.begin());
        } else {
          int ax = 0;
          for (int c = 1; c < 3; ++c)
            if (chi[c] - clo[c] > chi[ax] - clo[ax]) ax = c;
          std::nth_element(tris.begin() + b, tris.begin() + mid, tris.begin() + e,
                           [ax](const Tri& x, const Tri& y) { return x.c[ax] < y.c[ax]; });
        }
        build(b, mid);
        build(mid, e);
      }
      nodes[8 * me + 3] = int_bits(static_cast<int>(nodes.size() / 8));
    };
    build(0, fn);
    for (int f = 0; f < fn; ++f)
      for (int c = 0; c < 3; ++c) face_out[3 * (fa + f) + c] = tris[f].f[c];
    num[k] = static_cast<int>(nodes.size() / 8);
    node.insert(node.end(), nodes.begin(), nodes.end());
  }
  if (node.empty()) node.assign(8, 0.0f);
}

// ------------------------------------------------------------------ table families
// Each function below computes one family of tables from the model.  build_tables() calls them and
// appends their results to the two blocks in one fixed order (the blocks' layout).

// sizes and options copied from the model, and the switches that are plain DevModel fields
inline void model_counts(const Model& m, const Overrides& o, DevModel& d) {
  for (int s = 0; s < m.nsensor; ++s) {
    int t = m.sensor_type[s];
    if (t == MRS_SENS_ACCELEROMETER) d.acc_sens |= 1;
    if (t == MRS_SENS_FORCE || t == MRS_SENS_TORQUE) d.acc_sens |= 3;
    if (t == MRS_SENS_FRAMELINACC) d.acc_sens |= 1;  // reads cacc
    if (t == MRS_SENS_TOUCH) d.acc_sens |= 2;        // reads the row forces
  }
  d.na = m.na;
  d.nmocap = m.nmocap;
  d.nq = m.nq; d.nv = m.nv; d.nu = m.nu; d.nbody = m.nbody; d.njnt = m.njnt; d.ngeom = m.ngeom;
  d.nsite = m.nsite; d.ncam = m.ncam; d.nsensor = m.nsensor; d.nsensordata = m.nsensordata;
  d.max_depth = m.max_depth;
  d.integrator = m.integrator; d.iterations = m.iterations; d.disableflags = m.disableflags;
  d.solver = m.solver; d.ls_iterations = m.ls_iterations; d.cone = m.cone; d.restate = m.restate;
  if (o.no_multiccd) d.restate |= MRS_RESTATE_NO_MULTICCD;
  d.impratio = static_cast<float>(m.impratio); d.ls_tolerance = static_cast<float>(m.ls_tolerance);
  d.diag_skip = o.diag_skip;
  // a fused launch evaluates the sensors on its last step only (step.hip step_kernel); sens_every
  // evaluates them every step (A/B: the same outputs, bit for bit)
  d.sens_every = o.sensors_every_step ? 1 : 0;
  d.sparse_off = o.sparse_off;
  d.timestep = static_cast<float>(m.timestep);
  d.timestep_d = m.timestep;
  d.tolerance = static_cast<float>(m.tolerance);
  d.pgs_scale = solver_scale(m.stat_meaninertia, m.nv);
  for (int i = 0; i < 3; ++i) d.gravity[i] = static_cast<float>(m.gravity[i]);
}

// tree walks as flat lists: DFS subtree ends, bodies by depth, the pointer-jumping table and the
// (dof, ancestor-dof) pairs of M
struct TreeLists {
  std::vector<int> subtree_end, level_adr, level_num, level_body, jump, Mpair;
};
inline TreeLists tree_lists(const Model& m, const Overrides& o, DevModel& d) {
  TreeLists t;
  t.subtree_end.resize(m.nbody);
  for (int bI = m.nbody - 1; bI >= 0; --bI) {
    int e = bI + 1;
    while (e < m.nbody) {
      int x = e;
      bool inside = false;
      while (x != 0) { if (x == bI) { inside = true; break; } x = m.body_parentid[x]; }
      if (bI == 0) inside = true;
      if (!inside) break;
      ++e;
    }
    t.subtree_end[bI] = e;
  }
  t.level_adr.assign(m.max_depth + 2, 0);
  t.level_num.assign(m.max_depth + 2, 0);
  for (int lev = 1; lev <= m.max_depth; ++lev) {
    t.level_adr[lev] = static_cast<int>(t.level_body.size());
    for (int bI = 1; bI < m.nbody; ++bI)
      if (m.body_depth[bI] == lev) t.level_body.push_back(bI);
    t.level_num[lev] = static_cast<int>(t.level_body.size()) - t.level_adr[lev];
  }
  // every body has no joint or one hinge / free joint: the kinematics' one-pass joint frames
  d.kin_onepass = 1;
  for (int bI = 0; bI < m.nbody; ++bI) {
    const int nj = m.body_jntnum[bI];
    if (nj > 1) d.kin_onepass = 0;
    if (nj == 1) {
      const int jt = m.jnt_type[m.body_jntadr[bI]];
      if (jt != MRS_JNT_HINGE && jt != MRS_JNT_FREE) d.kin_onepass = 0;
    }
  }
  if (o.kin_twopass) d.kin_onepass = 0;
  // pointer-jumping tables for the tree passes: jump[r][b] = ancestor of b at distance 2^r when b
  // is deeper than 2^r (that ancestor is not the world body), else -1; ceil(log2(max_depth)) rounds
  d.njump = 0;
  while ((1 << d.njump) < m.max_depth) ++d.njump;
  t.jump.assign(std::max(1, d.njump * m.nbody), -1);
  for (int r = 0; r < d.njump; ++r)
    for (int bI = 1; bI < m.nbody; ++bI) {
      if (m.body_depth[bI] <= (1 << r)) continue;
      int a = bI;
      for (int k = 0; k < (1 << r); ++k) a = m.body_parentid[a];
      t.jump[r * m.nbody + bI] = a;
    }
  for (int i = 0; i < m.nv; ++i)
    for (int j = i; j >= 0; j = m.dof_parentid[j]) { t.Mpair.push_back(i); t.Mpair.push_back(j); }
  d.nMpair = static_cast<int>(t.Mpair.size() / 2);
  return t;
}

// static collision-pair filter (mj_collision broad phase minus the dynamic bounding test)
struct PairTables {
  std::vector<int> g1, g2, dim;
  std::vector<float> margin, gap, fric, solref, solimp;
};
inline PairTables collision_pairs(const Model& m, DevModel& d) {
  PairTables p;
  // explicit <contact><pair>s first, with their own parameters (mj_collision collides them before
  // the dynamic pairs; mrs::Model::expair_*)
  for (size_t q = 0; q < m.expair_geom1.size(); ++q) {
    const int ga = m.expair_geom1[q], gb = m.expair_geom2[q];
    const int ta = m.geom_type[ga], tb = m.geom_type[gb];
    if ((ta == MRS_GEOM_PLANE && tb == MRS_GEOM_PLANE) || ta == MRS_GEOM_HFIELD || tb == MRS_GEOM_HFIELD)
      throw UnsupportedError("explicit pair of geom types " + std::to_string(ta) + "/" + std::to_string(tb) +
                             " is not implemented");
    p.g1.push_back(ga); p.g2.push_back(gb);
    p.dim.push_back(m.expair_dim[q]);
    p.margin.push_back(static_cast<float>(m.expair_margin[q]));
    p.gap.push_back(static_cast<float>(m.expair_gap[q]));
    // (sliding, torsional, rolling) as the mixed pairs store them
    p.fric.push_back(static_cast<float>(m.expair_friction[5 * q]));
    p.fric.push_back(static_cast<float>(m.expair_friction[5 * q + 2]));
    p.fric.push_back(static_cast<float>(m.expair_friction[5 * q + 3]));
    for (int i = 0; i < 2; ++i) p.solref.push_back(static_cast<float>(m.expair_solref[2 * q + i]));
    for (int i = 0; i < 5; ++i) p.solimp.push_back(static_cast<float>(m.expair_solimp[5 * q + i]));
  }
  // the compiler's statically admissible pairs (mrs::Model::pair_geom1/2, lower geom type first)
  for (size_t q = 0; q < m.pair_geom1.size(); ++q) {
    const int ga = m.pair_geom1[q], gb = m.pair_geom2[q];
    const int g1 = std::min(ga, gb), g2 = std::max(ga, gb);
    int ta = m.geom_type[ga], tb = m.geom_type[gb];
    // every pair of the implemented types: dedicated primitives, plane-ellipsoid/cylinder/mesh,
    // and MPR for the rest (step.hip narrowphase); plane-plane pairs (a plane on a moving body
    // against another plane) are skipped, as mj_collision has no plane-plane collider; hfields
    // are absent
    if (ta == MRS_GEOM_PLANE && tb == MRS_GEOM_PLANE) continue;
    if (ta == MRS_GEOM_HFIELD || tb == MRS_GEOM_HFIELD)
      throw UnsupportedError("collision pair of geom types " + std::to_string(ta) + "/" + std::to_string(tb) +
                             " is not implemented (geoms " + std::to_string(g1) + "," + std::to_string(g2) + ")");
    p.g1.push_back(ga); p.g2.push_back(gb);
    p.dim.push_back(std::max(m.geom_condim[ga], m.geom_condim[gb]));
    p.margin.push_back(static_cast<float>(std::max(m.geom_margin[ga], m.geom_margin[gb])));
    p.gap.push_back(static_cast<float>(std::max(m.geom_gap[ga], m.geom_gap[gb])));
    double s1 = m.geom_solmix[ga], s2 = m.geom_solmix[gb], mix;
    if (s1 >= 1e-15 && s2 >= 1e-15) mix = s1 / (s1 + s2);
    else if (s1 < 1e-15 && s2 < 1e-15) mix = 0.5;
    else mix = s1 < 1e-15 ? 0 : 1;
    for (int i = 0; i < 3; ++i)
      p.fric.push_back(static_cast<float>(std::max(m.geom_friction[3 * ga + i], m.geom_friction[3 * gb + i])));
    for (int i = 0; i < 2; ++i)
      p.solref.push_back(static_cast<float>(mix * m.geom_solref[2 * ga + i] + (1 - mix) * m.geom_solref[2 * gb + i]));
    for (int i = 0; i < 5; ++i)
      p.solimp.push_back(static_cast<float>(mix * m.geom_solimp[5 * ga + i] + (1 - mix) * m.geom_solimp[5 * gb + i]));
  }
  d.npair = static_cast<int>(p.g1.size());
  d.npair_explicit = static_cast<int>(m.expair_geom1.size());
  return p;
}

// Reach ball of a geom: a centre fixed in the world and a radius rho such that the geom's centre lies
// inside the ball for every qpos, in every env.
//   - a geom of a body fixed in the world: its world position, rho = 0
//   - a geom below hinge and ball joints only, at most one per body, above them bodies fixed in the
//     world: the centre is the first joint's anchor a_1, and rho = sum |a_i - a_(i-1)| + |x_g - a_k|.
//     A rotation about an anchor keeps every distance from it, so each term is the same at every qpos
//     and is measured here at the pose with every joint at its reference (body_world); a jointless body
//     in the chain only adds its fixed offset
//   - anything else has no bound: a slide or free joint above, a mocap body above, two joints on a body
struct Reach {
  bool bounded = true, fixed = true;  // fixed: no joint above (then rho = 0 and `last` is unused)
  double c[3] = {0, 0, 0}, last[3] = {0, 0, 0}, rho = 0;  // last: the lowest anchor at the reference pose
};
inline std::vector<Reach> geom_reach(const Model& m) {
  auto point = [&](int body, const double* local, double out[3]) {
    double R[9], p[3];
    body_world(m, body, R, p);
    for (int i = 0; i < 3; ++i) out[i] = p[i] + R[3 * i] * local[0] + R[3 * i + 1] * local[1] + R[3 * i + 2] * local[2];
  };
  auto dist = [](const double a[3], const double b[3]) {
    return std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
  };
  std::vector<Reach> body(m.nbody);
  for (int b = 1; b < m.nbody; ++b) {  // (a parent's id is below its children's)
    Reach r = body[m.body_parentid[b]];
    if (m.body_mocapid[b] >= 0 || m.body_jntnum[b] > 1) r.bounded = false;
    if (r.bounded && m.body_jntnum[b] == 1) {
      const int j = m.body_jntadr[b];
      if (m.jnt_type[j] != MRS_JNT_HINGE && m.jnt_type[j] != MRS_JNT_BALL) r.bounded = false;
      else {
        double a[3];
        point(b, &m.jnt_pos[3 * j], a);
        if (r.fixed) std::copy(a, a + 3, r.c);
        else r.rho += dist(a, r.last);
        std::copy(a, a + 3, r.last);
        r.fixed = false;
      }
    }
    body[b] = r;
  }
  std::vector<Reach> geom(m.ngeom);
  for (int g = 0; g < m.ngeom; ++g) {
    Reach r = body[m.geom_bodyid[g]];
    if (r.bounded) {
      double x[3];
      point(m.geom_bodyid[g], &m.geom_pos[3 * g], x);
      if (r.fixed) std::copy(x, x + 3, r.c);
      else r.rho += dist(x, r.last);
    }
    geom[g] = r;
  }
  return geom;
}

// The pairs the device walks: the static filter's list without the automatic pairs whose reach balls
// prove that the geoms stay further apart than their bounding spheres plus margin.  Such a pair fails
// the kernel's sphere test (or, against a plane, has no contact within margin) at every step in every
// env, so leaving it out changes no result.  The slack covers the device's fp32 poses.  Explicit
// <contact><pair>s stay (they come first and the per-env friction indexes by npair_explicit), the kept
// pairs keep their order (the contact order), and only the walked list shrinks: contact and row
// capacity, the scratch layout and the plan are the full list's.  MRS_NO_PAIR_PRUNE keeps every pair.
inline bool never_touch(const Model& m, const std::vector<Reach>& reach, int ga, int gb, double margin) {
  const auto slack = [](double r) { return r * (1 + 1e-4) + 1e-4; };
  const bool pa = m.geom_type[ga] == MRS_GEOM_PLANE, pb = m.geom_type[gb] == MRS_GEOM_PLANE;
  if (pa || pb) {
    const int pl = pa ? ga : gb, g = pa ? gb : ga;
    if (pa && pb) return false;
    if (!fixed_in_world(m, m.geom_bodyid[pl]) || !reach[g].bounded) return false;
    // the whole ball in front of the plane (normal: z column of the plane's world rotation)
    double R[9], p[3], Rg[9], n[3], o[3], q[4];
    body_world(m, m.geom_bodyid[pl], R, p);
    const double* gq = &m.geom_quat[4 * pl];
    const double qn = std::sqrt(gq[0] * gq[0] + gq[1] * gq[1] + gq[2] * gq[2] + gq[3] * gq[3]);
    for (int i = 0; i < 4; ++i) q[i] = gq[i] / qn;
    quat_to_mat(q, Rg);
    for (int i = 0; i < 3; ++i) {
      n[i] = R[3 * i] * Rg[2] + R[3 * i + 1] * Rg[5] + R[3 * i + 2] * Rg[8];
      o[i] = p[i] + R[3 * i] * m.geom_pos[3 * pl] + R[3 * i + 1] * m.geom_pos[3 * pl + 1] + R[3 * i + 2] * m.geom_pos[3 * pl + 2];
    }
    const double h = n[0] * (reach[g].c[0] - o[0]) + n[1] * (reach[g].c[1] - o[1]) + n[2] * (reach[g].c[2] - o[2]);
    return h > slack(reach[g].rho + m.geom_rbound[g] + margin);
  }
  if (!reach[ga].bounded || !reach[gb].bounded) return false;
  const double* a = reach[ga].c;
  const double* b = reach[gb].c;
  const double dc = std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
  return dc > slack(reach[ga].rho + reach[gb].rho + m.geom_rbound[ga] + m.geom_rbound[gb] + margin);
}
inline PairTables prune_pairs(const Model& m, const PairTables& all, const Overrides& o) {
  if (o.no_pair_prune) return all;
  const std::vector<Reach> reach = geom_reach(m);
  PairTables p;
  for (size_t q = 0; q < all.g1.size(); ++q) {
    // (the margin as the kernel holds it, fp32, is the bound's)
    if (q >= m.expair_geom1.size() && never_touch(m, reach, all.g1[q], all.g2[q], all.margin[q])) continue;
    p.g1.push_back(all.g1[q]); p.g2.push_back(all.g2[q]); p.dim.push_back(all.dim[q]);
    p.margin.push_back(all.margin[q]); p.gap.push_back(all.gap[q]);
    p.fric.insert(p.fric.end(), &all.fric[3 * q], &all.fric[3 * q] + 3);
    p.solref.insert(p.solref.end(), &all.solref[2 * q], &all.solref[2 * q] + 2);
    p.solimp.insert(p.solimp.end(), &all.solimp[5 * q], &all.solimp[5 * q] + 5);
  }
  return p;
}

// active equality constraints (rows first in the solver order, as mj_makeConstraint)
struct EqTables {
  std::vector<int> type, obj1, obj2;
  std::vector<double> solref, solimp, data;
};
inline EqTables equality_tables(const Model& m, DevModel& d) {
  EqTables e;
  d.neq = d.neq_rows = 0;
  if (!(m.disableflags & (MRS_DSBL_EQUALITY | MRS_DSBL_CONSTRAINT)))
    for (size_t q = 0; q < m.eq_type.size(); ++q) {
      if (!m.eq_active0[q]) continue;
      e.type.push_back(m.eq_type[q]); e.obj1.push_back(m.eq_obj1id[q]); e.obj2.push_back(m.eq_obj2id[q]);
      e.solref.insert(e.solref.end(), &m.eq_solref[2 * q], &m.eq_solref[2 * q] + 2);
      e.solimp.insert(e.solimp.end(), &m.eq_solimp[5 * q], &m.eq_solimp[5 * q] + 5);
      e.data.insert(e.data.end(), &m.eq_data[MRS_NEQDATA * q], &m.eq_data[MRS_NEQDATA * q] + MRS_NEQDATA);
      d.neq_rows += m.eq_type[q] == MRS_EQ_CONNECT ? 3 : (m.eq_type[q] == MRS_EQ_WELD ? 6 : 1);
    }
  d.neq = static_cast<int>(e.type.size());
  return e;
}

// tendons.  Fixed: wraps (qpos / dof address, coefficient) and the constant Jacobian rows (dense
// ntendon x nv).  Spatial (DevModel::nten_spatial): no wraps and a zero row here; per tendon its id and
// its segments -- consecutive sites of one branch -- as 12-float records: the sites' bodies (int bits),
// their local positions, the weight 1 / divisor of the branch's pulley.  Both: per tendon 12 constants
// (stiffness, damping, lengthspring[2], range[2], margin, frictionloss, invweight0), and the tendons
// that give friction-loss / limit rows
struct TendonTables {
  std::vector<int> adr, num, wrap_qadr, wrap_dof, fric, lim, sp_ten, sp_adr, sp_num, sp_of;
  std::vector<double> coef, J, prm;
  std::vector<float> sp_seg;
};
inline TendonTables tendon_tables(const Model& m, DevModel& d) {
  TendonTables t;
  const int ntendon = static_cast<int>(m.tendon_adr.size());
  t.J.assign(static_cast<size_t>(ntendon) * m.nv, 0.0);
  t.sp_of.assign(ntendon, -1);
  for (int n = 0; n < ntendon; ++n) {
    const int a0 = m.tendon_adr[n], a1 = a0 + m.tendon_num[n];
    t.adr.push_back(static_cast<int>(t.coef.size()));
    if (m.tendon_kind[n] == MRS_TENDON_SPATIAL) {
      t.num.push_back(0);
      t.sp_of[n] = static_cast<int>(t.sp_ten.size());
      t.sp_ten.push_back(n);
      t.sp_adr.push_back(static_cast<int>(t.sp_seg.size() / 12));
      double w = 1;
      for (int k = a0; k < a1; ++k) {
        if (m.wrap_type[k] == MRS_WRAP_PULLEY) { w = 1 / m.wrap_prm[k]; continue; }
        if (k + 1 >= a1 || m.wrap_type[k + 1] != MRS_WRAP_SITE) continue;
        const int s0 = m.wrap_objid[k], s1 = m.wrap_objid[k + 1];
        t.sp_seg.insert(t.sp_seg.end(), {int_bits(m.site_bodyid[s0]), int_bits(m.site_bodyid[s1]),
                                         static_cast<float>(m.site_pos[3 * s0]), static_cast<float>(m.site_pos[3 * s0 + 1]),
                                         static_cast<float>(m.site_pos[3 * s0 + 2]), static_cast<float>(m.site_pos[3 * s1]),
                                         static_cast<float>(m.site_pos[3 * s1 + 1]), static_cast<float>(m.site_pos[3 * s1 + 2]),
                                         static_cast<float>(w), 0.0f, 0.0f, 0.0f});
      }
      t.sp_num.push_back(static_cast<int>(t.sp_seg.size() / 12) - t.sp_adr.back());
    } else {
      t.num.push_back(a1 - a0);
      for (int k = a0; k < a1; ++k) {
        t.wrap_qadr.push_back(m.jnt_qposadr[m.wrap_objid[k]]);
        t.wrap_dof.push_back(m.jnt_dofadr[m.wrap_objid[k]]);
        t.coef.push_back(m.wrap_prm[k]);
        t.J[static_cast<size_t>(n) * m.nv + t.wrap_dof.back()] += m.wrap_prm[k];
      }
    }
    const double pr[12] = {m.tendon_stiffness[n], m.tendon_damping[n], m.tendon_lengthspring[2 * n],
                           m.tendon_lengthspring[2 * n + 1], m.tendon_range[2 * n], m.tendon_range[2 * n + 1],
                           m.tendon_margin[n], m.tendon_frictionloss[n], m.tendon_invweight0[n], 0, 0, 0};
    t.prm.insert(t.prm.end(), pr, pr + 12);
    if (!(m.disableflags & (MRS_DSBL_FRICTIONLOSS | MRS_DSBL_CONSTRAINT)) && m.tendon_frictionloss[n] > 0)
      t.fric.push_back(n);
    if (!(m.disableflags & (MRS_DSBL_LIMIT | MRS_DSBL_CONSTRAINT)) && m.tendon_limited[n]) t.lim.push_back(n);
  }
  d.ntendon = ntendon;
  d.nten_fric = static_cast<int>(t.fric.size());
  d.nten_lim = static_cast<int>(t.lim.size());
  d.nten_spatial = static_cast<int>(t.sp_ten.size());
  return t;
}

// kinematic trees (bodies sharing a root child of the world) that own dofs: their dofs are one
// contiguous range, M is block diagonal over them, and constraint rows touch at most two of them
// (mj_island's trees).  Blocked mode stores M / its factor per tree and solves the constraint rows
// sparsely over the trees they touch (csrc/hip/step.hip constraints_sparse).
struct KinTrees {
  std::vector<int> body_tree, dof_tree, dofadr, dofnum, Moff;
};
inline KinTrees kinematic_trees(const Model& m, const PairTables& pairs, DevModel& d) {
  KinTrees t;
  t.body_tree.assign(m.nbody, -1);
  t.dof_tree.assign(std::max(1, m.nv), -1);
  std::vector<int> root_tree(m.nbody, -1);
  for (int bI = 1; bI < m.nbody; ++bI) {
    if (m.body_dofnum[bI] == 0) continue;
    const int r = m.body_rootid[bI];
    if (root_tree[r] < 0) {
      root_tree[r] = static_cast<int>(t.dofadr.size());
      t.dofadr.push_back(m.body_dofadr[bI]);
      t.dofnum.push_back(0);
    }
  }
  for (int bI = 1; bI < m.nbody; ++bI) t.body_tree[bI] = root_tree[m.body_rootid[bI]];
  for (int j = 0; j < m.nv; ++j) {
    const int k = t.body_tree[m.dof_bodyid[j]];
    if (k < 0 || j != t.dofadr[k] + t.dofnum[k])
      throw UnsupportedError("dofs of a kinematic tree are not contiguous");
    t.dof_tree[j] = k;
    ++t.dofnum[k];
  }
  int off = 0;
  d.tree_nmax = 0;
  for (size_t k = 0; k < t.dofadr.size(); ++k) {
    t.Moff.push_back(off);
    off += t.dofnum[k] * t.dofnum[k];
    d.tree_nmax = std::max(d.tree_nmax, t.dofnum[k]);
  }
  d.ntree = static_cast<int>(t.dofadr.size());
  d.nMblk = off;
  // pipe width of the sparse solver: dof slots of the widest row (two trees for a contact)
  int widest = 1;
  for (int j = 0; j < m.nv; ++j) widest = std::max(widest, t.dofnum[t.dof_tree[j]]);
  for (size_t p = 0; p < pairs.g1.size(); ++p) {
    const int t1 = t.body_tree[m.geom_bodyid[pairs.g1[p]]], t2 = t.body_tree[m.geom_bodyid[pairs.g2[p]]];
    int w = (t1 >= 0 ? t.dofnum[t1] : 0) + (t2 >= 0 && t2 != t1 ? t.dofnum[t2] : 0);
    widest = std::max(widest, w);
  }
  d.pipe_w = 8;
  while (d.pipe_w < widest) d.pipe_w *= 2;
  return t;
}

// sensors by kernel path: rangefinders (the ray passes), the velocity / axis / subtree / touch types
// (step.hip sensors_more, entered only by models that have one), the others (step.hip sensors)
inline bool is_sensor_more(int t) {
  return t == MRS_SENS_TOUCH || t == MRS_SENS_VELOCIMETER || t == MRS_SENS_SUBTREECOM || t == MRS_SENS_SUBTREELINVEL ||
         (t >= MRS_SENS_FRAMEXAXIS && t <= MRS_SENS_FRAMELINACC) || t == MRS_SENS_TENDONPOS || t == MRS_SENS_TENDONVEL;
}

// the row sources: friction-loss dofs, limited joints, the sensors by path, and the contact / row
// capacity per env.  max_con_req: requested contact capacity, or (<= 0) the pairs' own maxima (8 for
// box-box and plane-mesh, 4 for the other pairs) clamped to [32, 128]
struct RowLists {
  std::vector<int> fric, lim, rf, other_sens, more_sens;
};
inline RowLists row_lists(const Model& m, const PairTables& pairs, int max_con_req, DevModel& d) {
  RowLists r;
  for (int j = 0; j < m.nv; ++j) if (m.dof_frictionloss[j] > 0) r.fric.push_back(j);
  for (int j = 0; j < m.njnt; ++j)
    if (m.jnt_limited[j] && (m.jnt_type[j] == MRS_JNT_HINGE || m.jnt_type[j] == MRS_JNT_SLIDE)) r.lim.push_back(j);
  for (int s = 0; s < m.nsensor; ++s) {
    if (m.sensor_type[s] == MRS_SENS_RANGEFINDER) r.rf.push_back(s);
    else if (is_sensor_more(m.sensor_type[s])) r.more_sens.push_back(s);
    else r.other_sens.push_back(s);
  }
  d.nsens_other = static_cast<int>(r.other_sens.size());
  d.nsens_more = static_cast<int>(r.more_sens.size());
  d.nfric = static_cast<int>(r.fric.size());
  d.nlim = static_cast<int>(r.lim.size());
  d.nrf = static_cast<int>(r.rf.size());
  int pair_max = 0;
  for (size_t p = 0; p < pairs.g1.size(); ++p) {
    const int ta = m.geom_type[pairs.g1[p]], tb = m.geom_type[pairs.g2[p]];
    pair_max += (ta == MRS_GEOM_BOX && tb == MRS_GEOM_BOX) || (ta == MRS_GEOM_PLANE && tb == MRS_GEOM_MESH) ? kMaxPairCon : 4;
  }
  const int cap = max_con_req > 0 ? max_con_req : std::min(128, std::max(32, pair_max));
  d.max_con = d.npair == 0 ? 0 : std::min(pair_max, cap);
  d.max_efc = d.neq_rows + d.nfric + d.nten_fric + 2 * (d.nlim + d.nten_lim) + 4 * d.max_con;
  return r;
}

// actuators: joint transmissions by dof / qpos address; a tendon transmission's addresses hold
// -1 - tendon (length and velocity from the step's tendon slot in LDS), its moment is gear * ten_J
// A site transmission (DevModel::nact_site) has a record in `site` (12 floats: the actuator, the site's
// body, the site's local position, the gear's force and torque halves turned into the body's frame); its
// addresses hold -1 - (ntendon + k), the slot behind the tendons' that step.hip site_act_vel fills, and
// its gear here is 1: the six gear numbers are in the moment
struct ActTables {
  std::vector<int> dof, qadr, ten;
  std::vector<float> gear, gain, bias, site;
};
inline ActTables actuator_tables(const Model& m, DevModel& d) {
  ActTables t;
  const int ntendon = static_cast<int>(m.tendon_adr.size());
  d.nact_site = d.nact_site_vel = 0;
  for (int a = 0; a < m.nu; ++a) {
    int j = m.actuator_trnid[2 * a];
    if (m.actuator_trntype[a] == MRS_TRN_SITE) {
      const int slot = ntendon + d.nact_site++;
      t.dof.push_back(-1 - slot);
      t.qadr.push_back(-1 - slot);
      t.ten.push_back(-1);
      double R[9];
      quat_to_mat(&m.site_quat[4 * j], R);
      const double* g = &m.actuator_gear[6 * a];
      t.site.insert(t.site.end(), {int_bits(a), int_bits(m.site_bodyid[j]), static_cast<float>(m.site_pos[3 * j]),
                                   static_cast<float>(m.site_pos[3 * j + 1]), static_cast<float>(m.site_pos[3 * j + 2])});
      for (int h = 0; h < 2; ++h)
        for (int i = 0; i < 3; ++i)
          t.site.push_back(static_cast<float>(R[3 * i] * g[3 * h] + R[3 * i + 1] * g[3 * h + 1] + R[3 * i + 2] * g[3 * h + 2]));
      t.site.push_back(0.0f);
      const double *gp = &m.actuator_gainprm[MRS_NGAIN * a], *bp = &m.actuator_biasprm[MRS_NBIAS * a];
      if ((m.actuator_gaintype[a] == MRS_GAIN_AFFINE && (gp[1] != 0 || gp[2] != 0)) ||
          (m.actuator_biastype[a] == MRS_BIAS_AFFINE && (bp[1] != 0 || bp[2] != 0)))
        ++d.nact_site_vel;
      t.gear.push_back(1.0f);
      for (int i = 0; i < 3; ++i) {
        t.gain.push_back(static_cast<float>(gp[i]));
        t.bias.push_back(static_cast<float>(bp[i]));
      }
      continue;
    }
    if (m.actuator_trntype[a] == MRS_TRN_TENDON) {
      t.dof.push_back(-1 - j);
      t.qadr.push_back(-1 - j);
      t.ten.push_back(j);
    } else {
      if (m.jnt_type[j] != MRS_JNT_HINGE && m.jnt_type[j] != MRS_JNT_SLIDE)
        throw UnsupportedError("actuators on free/ball joints are not supported");
      t.dof.push_back(m.jnt_dofadr[j]);
      t.qadr.push_back(m.jnt_qposadr[j]);
      t.ten.push_back(-1);
    }
    t.gear.push_back(static_cast<float>(m.actuator_gear[6 * a]));
    for (int i = 0; i < 3; ++i) {
      t.gain.push_back(static_cast<float>(m.actuator_gainprm[MRS_NGAIN * a + i]));
      t.bias.push_back(static_cast<float>(m.actuator_biasprm[MRS_NBIAS * a + i]));
    }
  }
  return t;
}

// mesh tables: the hierarchies and the face list reordered to their leaves, then the pre-gathered
// triangle records in device face order -- vertex a, b - a, c - a, formed in fp32 from the fp32 vertices
// exactly as ray_tri forms them on the device (bit-identical t)
struct MeshTables {
  std::vector<int> face, bvh_adr, bvh_num;
  std::vector<float> bvh_node, tri;
};
inline MeshTables mesh_tables(const Model& m, const Overrides& o) {
  MeshTables t;
  build_mesh_bvh(m, o, t.face, t.bvh_node, t.bvh_adr, t.bvh_num);
  t.tri.resize(9 * t.face.size() / 3);
  const int nmesh = static_cast<int>(m.mesh_faceadr.size());
  for (int k = 0; k < nmesh; ++k)
    for (int f = m.mesh_faceadr[k]; f < m.mesh_faceadr[k] + m.mesh_facenum[k]; ++f) {
      float v[3][3];
      for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 3; ++i) v[c][i] = static_cast<float>(m.mesh_vert[3 * (m.mesh_vertadr[k] + t.face[3 * f + c]) + i]);
      for (int i = 0; i < 3; ++i) {
        t.tri[9 * f + i] = v[0][i];
        t.tri[9 * f + 3 + i] = v[1][i] - v[0][i];
        t.tri[9 * f + 6 + i] = v[2][i] - v[0][i];
      }
    }
  return t;
}

// mesh geoms a camera can see (groups 0-2, alpha > 0), for the binning frame kernel; limits of its
// records: 64 geom slots, 2^18 triangles per mesh, pairs within an int
inline void raster_lists(const Model& m, DevModel& d, std::vector<int>& rg, std::vector<int>& rb) {
  long long np = 0;
  bool ok = true;
  for (int g = 0; g < m.ngeom; ++g) {
    if (m.geom_type[g] != MRS_GEOM_MESH || m.geom_group[g] < 0 || m.geom_group[g] > 2 || m.geom_rgba[4 * g + 3] == 0) continue;
    const int fn = m.mesh_facenum[m.geom_dataid[g]];
    ok &= fn < (1 << 18);
    rg.push_back(g);
    rb.push_back(static_cast<int>(np));
    np += fn;
  }
  ok &= rg.size() <= 64 && np < (1ll << 30) && m.ngeom <= kDepthGeoms;
  if (!ok) { rg.clear(); rb.clear(); np = 0; }
  d.nrast = static_cast<int>(rg.size());
  d.nrast_pair = static_cast<int>(np);
}

// lit.h's rlit block (layout in its header comment); more than kRlitMaxLights lights are refused
inline std::vector<double> lit_block(const Model& m, DevModel& d) {
  if (static_cast<int>(m.light_active.size()) > kRlitMaxLights)
    throw std::runtime_error("at most " + std::to_string(kRlitMaxLights) + " lights are supported");
  const int nl = static_cast<int>(m.light_active.size()), nm = static_cast<int>(m.mat_texid.size()),
            nt = static_cast<int>(m.tex_type.size());
  std::vector<double> r(kRlitHead + kRlitLight * nl + kRlitMat * nm + kRlitTex * nt, 0.0);
  for (int i = 0; i < 10; ++i) r[i] = m.vis_headlight[i];
  r[10] = nl;
  d.lit_sky = -1;
  for (int t = 0; t < nt && d.lit_sky < 0; ++t)
    if (m.tex_type[t] == MRS_TEX_SKYBOX) d.lit_sky = t;
  r[11] = d.lit_sky;
  for (int l = 0; l < nl; ++l) {
    double* o = r.data() + kRlitHead + kRlitLight * l;
    for (int i = 0; i < 3; ++i) {
      o[i] = m.light_pos[3 * l + i]; o[3 + i] = m.light_dir[3 * l + i];
      o[6 + i] = m.light_ambient[3 * l + i]; o[9 + i] = m.light_diffuse[3 * l + i];
      o[12 + i] = m.light_specular[3 * l + i]; o[15 + i] = m.light_attenuation[3 * l + i];
    }
    o[18] = std::cos(m.light_cutoff[l] * M_PI / 180); o[19] = m.light_exponent[l];
    o[20] = m.light_directional[l]; o[21] = m.light_castshadow[l]; o[22] = m.light_active[l];
  }
  d.lit_nlight = nl;
  d.lit_mat0 = kRlitHead + kRlitLight * nl;
  d.lit_tex0 = d.lit_mat0 + kRlitMat * nm;
  for (int k = 0; k < nm; ++k) {
    double* o = r.data() + d.lit_mat0 + kRlitMat * k;
    o[0] = m.mat_texid[k]; o[1] = m.mat_texuniform[k];
    o[2] = m.mat_texrepeat[2 * k]; o[3] = m.mat_texrepeat[2 * k + 1];
    o[4] = m.mat_specular[k]; o[5] = m.mat_shininess[k]; o[6] = m.mat_emission[k];
  }
  for (int t = 0; t < nt; ++t) {
    double* o = r.data() + d.lit_tex0 + kRlitTex * t;
    o[0] = m.tex_type[t]; o[1] = m.tex_builtin[t]; o[2] = m.tex_mark[t];
    o[3] = m.tex_width[t]; o[4] = m.tex_height[t];
    for (int i = 0; i < 3; ++i) { o[5 + i] = m.tex_rgb1[3 * t + i]; o[8 + i] = m.tex_rgb2[3 * t + i]; o[11 + i] = m.tex_markrgb[3 * t + i]; }
  }
  return r;
}

// friction-loss rows and limited joints, 4 floats each, staged in workgroup LDS (shr_fric, shr_lim):
// a friction row's impedance is that of distance 0 at margin 0, so its R and reference stiffness
// B are model constants (computed here in fp32, the order the kernel used); limits: qpos address,
// margin, range
inline void row_records(const Model& m, const RowLists& rows, float timestep, std::vector<float>& fricrec,
                        std::vector<float>& limrec) {
  auto clampf = [](float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); };
  for (int j : rows.fric) {
    const float si1 = static_cast<float>(m.dof_solimp[5 * j + 1]);
    const float dmax = clampf(si1, 0.0001f, 0.9999f);
    const float R = fric_row_R(m, j, m.dof_invweight0[j]);  // (start_rows.h: an env's inertial row computes it too)
    const float sr0 = static_cast<float>(m.dof_solref[2 * j]), sr1 = static_cast<float>(m.dof_solref[2 * j + 1]);
    float B;
    if (sr0 > 0) {
      float tc = sr0;
      if (!(m.disableflags & MRS_DSBL_REFSAFE) && tc < 2 * timestep) tc = 2 * timestep;
      B = 2 / (dmax * tc);
    } else {
      B = -sr1 / dmax;
    }
    fricrec.insert(fricrec.end(), {int_bits(j), R, B, static_cast<float>(m.dof_frictionloss[j])});
  }
  for (int j : rows.lim)
    limrec.insert(limrec.end(), {int_bits(m.jnt_qposadr[j]), static_cast<float>(m.jnt_margin[j]),
                                 static_cast<float>(m.jnt_range[2 * j]), static_cast<float>(m.jnt_range[2 * j + 1])});
}

// smooth-force tables (step.hip smooth_forces), staged in workgroup LDS: per actuator (20 floats)
// qpos / dof address, gear, ctrl limit flag and range, gain type and prm[3], bias type and prm[3],
// force limit flag and range; per dof (16 floats) its single actuator (-1 none, -2 several: the
// actuator loop runs), that actuator's gear, the joint's actuator-force limit flag and range,
// joint type, stiffness, qpos address, qpos_spring, the dof's damping, body, subtree end,
// whether any body of the subtree has gravcomp, the dof's friction-loss row (-1 none) and its
// joint's first dof.  actdyn: activation dynamics of the stateful actuators (step.hip act_input /
// act_next), read only when na > 0: per actuator (8 floats) dyntype, address in act (-1 stateless), the
// time constant max(tau, 1e-15), filterexact's step factor tau (1 - exp(-h / tau)) from fp64, the
// activation limit flag and range, actearly
struct SmoothRecords {
  std::vector<float> actrec, dofrec, actdyn;
};
inline SmoothRecords smooth_force_records(const Model& m, const ActTables& act, const TendonTables& ten,
                                          const TreeLists& trees, const RowLists& rows) {
  SmoothRecords s;
  for (int a = 0; a < m.nu; ++a) {
    std::vector<float> r = {int_bits(act.qadr[a]), int_bits(act.dof[a]), act.gear[a], int_bits(m.actuator_ctrllimited[a]),
                            static_cast<float>(m.actuator_ctrlrange[2 * a]), static_cast<float>(m.actuator_ctrlrange[2 * a + 1]),
                            int_bits(m.actuator_gaintype[a]), act.gain[3 * a], act.gain[3 * a + 1], act.gain[3 * a + 2],
                            int_bits(m.actuator_biastype[a]), act.bias[3 * a], act.bias[3 * a + 1], act.bias[3 * a + 2],
                            int_bits(m.actuator_forcelimited[a]), static_cast<float>(m.actuator_forcerange[2 * a]),
                            static_cast<float>(m.actuator_forcerange[2 * a + 1]), 0.0f, 0.0f, 0.0f};
    s.actrec.insert(s.actrec.end(), r.begin(), r.end());
  }
  // each dof's friction-loss row (its index in the friction rows, -1 none): the 16-lane register
  // solvers index the friction rows by dof (step.hip constraints)
  std::vector<int> fric_row(m.nv, -1);
  for (size_t k = 0; k < rows.fric.size(); ++k) fric_row[rows.fric[k]] = static_cast<int>(k);
  for (int j = 0; j < m.nv; ++j) {
    int ai = -1;
    float gear = 0;
    for (int a = 0; a < m.nu; ++a) {
      if (act.dof[a] == j) { ai = ai == -1 ? a : -2; gear = act.gear[a]; }
      if (act.ten[a] >= 0 && ten.J[static_cast<size_t>(act.ten[a]) * m.nv + j] != 0) ai = -2;  // the loop
      if (act.ten[a] >= 0 && ten.sp_of[act.ten[a]] >= 0) ai = -2;  // (a spatial tendon can move any dof)
    }
    const int jid = m.dof_jntid[j], b = m.dof_bodyid[j];
    int gc = 0;
    for (int x = b; x < trees.subtree_end[b]; ++x) gc |= m.body_gravcomp[x] != 0;
    std::vector<float> r = {int_bits(ai), gear, int_bits(m.jnt_actfrclimited[jid]), static_cast<float>(m.jnt_actfrcrange[2 * jid]),
                            static_cast<float>(m.jnt_actfrcrange[2 * jid + 1]), int_bits(m.jnt_type[jid]),
                            static_cast<float>(m.jnt_stiffness[jid]), int_bits(m.jnt_qposadr[jid]),
                            static_cast<float>(m.qpos_spring[m.jnt_qposadr[jid]]), static_cast<float>(m.dof_damping[j]),
                            int_bits(b), int_bits(trees.subtree_end[b]), int_bits(gc), int_bits(fric_row[j]),
                            int_bits(m.jnt_dofadr[jid]), 0.0f};
    s.dofrec.insert(s.dofrec.end(), r.begin(), r.end());
  }
  if (m.na > 0)
    for (int a = 0; a < m.nu; ++a) {
      const double tau = std::max(m.actuator_dynprm[3 * a], 1e-15);
      const std::vector<float> r = {int_bits(m.actuator_dyntype[a]), int_bits(m.actuator_actadr[a]), static_cast<float>(tau),
                                    static_cast<float>(tau * -std::expm1(-m.timestep / tau)),
                                    int_bits(m.actuator_actlimited[a]), static_cast<float>(m.actuator_actrange[2 * a]),
                                    static_cast<float>(m.actuator_actrange[2 * a + 1]), int_bits(m.actuator_actearly[a])};
      s.actdyn.insert(s.actdyn.end(), r.begin(), r.end());
    }
  return s;
}

// tree tables for the smooth dynamics (step.hip com_pos, make_M, com_vel, rne), staged in workgroup
// LDS: per body (8 floats) mass, subtree mass, root, parent, subtree end, dof address, dof count,
// pad; per (dof, ancestor-dof) pair of M (4 floats) i, j, body of i, armature when i == j
inline void tree_records(const Model& m, const TreeLists& trees, std::vector<float>& bodytab, std::vector<float>& mpairtab) {
  for (int b = 0; b < m.nbody; ++b)
    bodytab.insert(bodytab.end(), {static_cast<float>(m.body_mass[b]), static_cast<float>(m.body_subtreemass[b]),
                                   int_bits(m.body_rootid[b]), int_bits(m.body_parentid[b]), int_bits(trees.subtree_end[b]),
                                   int_bits(m.body_dofadr[b]), int_bits(m.body_dofnum[b]), 0.0f});
  for (size_t q = 0; q + 1 < trees.Mpair.size(); q += 2) {
    const int i = trees.Mpair[q], j = trees.Mpair[q + 1];
    mpairtab.insert(mpairtab.end(), {int_bits(i), int_bits(j), int_bits(m.dof_bodyid[i]),
                                     i == j ? static_cast<float>(m.dof_armature[i]) : 0.0f});
  }
}

// kinematics tables (step.hip body_pose / body_frame_out / kinematics / com_pos), staged in workgroup
// LDS with lane groups: per body (25 floats) pos[3], quat[4], ipos[3], iquat[4], inertia[3], first
// joint, joint count, mocap id + 1 (int bits), pad; per joint (13) pos[3], axis[3], qpos address, type,
// qpos0 of the address, body, dof address, the body's root (int bits), pad; per geom (9) body (int
// bits), pos[3], quat[4], pad
inline void kinematics_records(const Model& m, std::vector<float>& kb, std::vector<float>& kj, std::vector<float>& kg) {
  for (int b = 0; b < m.nbody; ++b) {
    for (int i = 0; i < 3; ++i) kb.push_back(static_cast<float>(m.body_pos[3 * b + i]));
    for (int i = 0; i < 4; ++i) kb.push_back(static_cast<float>(m.body_quat[4 * b + i]));
    for (int i = 0; i < 3; ++i) kb.push_back(static_cast<float>(m.body_ipos[3 * b + i]));
    for (int i = 0; i < 4; ++i) kb.push_back(static_cast<float>(m.body_iquat[4 * b + i]));
    for (int i = 0; i < 3; ++i) kb.push_back(static_cast<float>(m.body_inertia[3 * b + i]));
    kb.push_back(int_bits(m.body_jntadr[b]));
    kb.push_back(int_bits(m.body_jntnum[b]));
    kb.push_back(int_bits(m.body_mocapid[b] + 1));  // (0: not a mocap body, as the pad was)
    while (kb.size() % 25) kb.push_back(0.0f);
  }
  for (int j = 0; j < m.njnt; ++j) {
    for (int i = 0; i < 3; ++i) kj.push_back(static_cast<float>(m.jnt_pos[3 * j + i]));
    for (int i = 0; i < 3; ++i) kj.push_back(static_cast<float>(m.jnt_axis[3 * j + i]));
    kj.push_back(int_bits(m.jnt_qposadr[j]));
    kj.push_back(int_bits(m.jnt_type[j]));
    kj.push_back(static_cast<float>(m.qpos0[m.jnt_qposadr[j]]));
    kj.push_back(int_bits(m.jnt_bodyid[j]));
    kj.push_back(int_bits(m.jnt_dofadr[j]));
    kj.push_back(int_bits(m.body_rootid[m.jnt_bodyid[j]]));
    while (kj.size() % 13) kj.push_back(0.0f);
  }
  for (int g = 0; g < m.ngeom; ++g) {
    kg.push_back(int_bits(m.geom_bodyid[g]));
    for (int i = 0; i < 3; ++i) kg.push_back(static_cast<float>(m.geom_pos[3 * g + i]));
    for (int i = 0; i < 4; ++i) kg.push_back(static_cast<float>(m.geom_quat[4 * g + i]));
    kg.push_back(0.0f);
  }
}

// the non-ray sensors' descriptors, 16 floats each (staged in workgroup LDS at shr_sens): type,
// objtype, sensordata address, dim (int bits), cutoff, the object's qpos / dof / actuator / body
// index (int bits), the root body (int bits), then the site's or geom's local pos[3] and quat[4];
// then the records of sensors_more's types, 32 floats each: the same first 15 (the body and the
// local pose of the site / geom / body frame; the body's tree root), 15: one past the last body of
// the body's subtree (bodies of a subtree are contiguous), 16: the site's shape type (int bits),
// 17-19: its size, 20: the subtree's mass
inline std::vector<float> sensor_records(const Model& m, const RowLists& rows, const TreeLists& trees) {
  std::vector<float> sensrec;
  for (int sid : rows.other_sens) {
    const int t = m.sensor_type[sid], ot = m.sensor_objtype[sid], id = m.sensor_objid[sid];
    int a = id, root = 0;
    double lp[3] = {0, 0, 0}, lq[4] = {1, 0, 0, 0};
    if (t == MRS_SENS_JOINTPOS) a = m.jnt_qposadr[id];
    else if (t == MRS_SENS_JOINTVEL) a = m.jnt_dofadr[id];
    else if (t == MRS_SENS_ACCELEROMETER || t == MRS_SENS_FORCE || t == MRS_SENS_TORQUE || t == MRS_SENS_GYRO ||
             ((t == MRS_SENS_FRAMEPOS || t == MRS_SENS_FRAMEQUAT) && ot == MRS_OBJ_SITE)) {
      a = m.site_bodyid[id];
      for (int i = 0; i < 3; ++i) lp[i] = m.site_pos[3 * id + i];
      for (int i = 0; i < 4; ++i) lq[i] = m.site_quat[4 * id + i];
    } else if ((t == MRS_SENS_FRAMEPOS || t == MRS_SENS_FRAMEQUAT) && ot != MRS_OBJ_BODY) {  // geom
      a = m.geom_bodyid[id];
      for (int i = 0; i < 4; ++i) lq[i] = m.geom_quat[4 * id + i];
    }
    if (a >= 0 && (t == MRS_SENS_ACCELEROMETER || t == MRS_SENS_FORCE || t == MRS_SENS_TORQUE)) root = m.body_rootid[a];
    sensrec.insert(sensrec.end(), {int_bits(t), int_bits(ot), int_bits(m.sensor_adr[sid]), int_bits(m.sensor_dim[sid]),
                                   static_cast<float>(m.sensor_cutoff[sid]), int_bits(a), int_bits(root),
                                   static_cast<float>(lp[0]), static_cast<float>(lp[1]), static_cast<float>(lp[2]),
                                   static_cast<float>(lq[0]), static_cast<float>(lq[1]), static_cast<float>(lq[2]),
                                   static_cast<float>(lq[3]), int_bits(id), 0.0f});
  }
  for (int sid : rows.more_sens) {
    const int t = m.sensor_type[sid], ot = m.sensor_objtype[sid], id = m.sensor_objid[sid];
    int a = id, st = MRS_GEOM_SPHERE;
    double lp[3] = {0, 0, 0}, lq[4] = {1, 0, 0, 0}, sz[3] = {0, 0, 0};
    if (ot == MRS_OBJ_SITE) {
      a = m.site_bodyid[id];
      for (int i = 0; i < 3; ++i) lp[i] = m.site_pos[3 * id + i];
      for (int i = 0; i < 4; ++i) lq[i] = m.site_quat[4 * id + i];
      for (int i = 0; i < 3; ++i) sz[i] = m.site_size[3 * id + i];
      st = m.site_type[id];
    } else if (ot == MRS_OBJ_GEOM) {
      a = m.geom_bodyid[id];
      for (int i = 0; i < 3; ++i) lp[i] = m.geom_pos[3 * id + i];
      for (int i = 0; i < 4; ++i) lq[i] = m.geom_quat[4 * id + i];
    } else if (ot == MRS_OBJ_TENDON) {
      a = 0;  // (no body: tendonpos / tendonvel read the step's tendon slot by the tendon id, word 14)
    }
    sensrec.insert(sensrec.end(), {int_bits(t), int_bits(ot), int_bits(m.sensor_adr[sid]), int_bits(m.sensor_dim[sid]),
                                   static_cast<float>(m.sensor_cutoff[sid]), int_bits(a), int_bits(m.body_rootid[a]),
                                   static_cast<float>(lp[0]), static_cast<float>(lp[1]), static_cast<float>(lp[2]),
                                   static_cast<float>(lq[0]), static_cast<float>(lq[1]), static_cast<float>(lq[2]),
                                   static_cast<float>(lq[3]), int_bits(id), int_bits(a == 0 ? m.nbody : trees.subtree_end[a]),
                                   int_bits(st), static_cast<float>(sz[0]), static_cast<float>(sz[1]),
                                   static_cast<float>(sz[2]), static_cast<float>(m.body_subtreemass[a]),
                                   0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f});
  }
  return sensrec;
}

// ray-visible geoms (rgba alpha != 0, what mj_ray tests), 8 floats per geom: geom id, type, body (int
// bits), rbound, size[3], mesh id (int bits); and the bits of those fixed in the world (rf_static_mask,
// for models whose ray blocks are built: at most 32 ray geoms)
inline std::vector<float> ray_geom_records(const Model& m, DevModel& d) {
  std::vector<float> rgeom;
  for (int g = 0; g < m.ngeom; ++g) {
    if (m.geom_rgba[4 * g + 3] == 0) continue;
    rgeom.insert(rgeom.end(), {int_bits(g), int_bits(m.geom_type[g]), int_bits(m.geom_bodyid[g]),
                               static_cast<float>(m.geom_rbound[g]), static_cast<float>(m.geom_size[3 * g]),
                               static_cast<float>(m.geom_size[3 * g + 1]), static_cast<float>(m.geom_size[3 * g + 2]),
                               int_bits(m.geom_dataid[g])});
  }
  d.nrgeom = static_cast<int>(rgeom.size() / 8);
  d.rf_static_mask = 0;
  if (d.nrgeom <= 32 && d.nrf > 0)
    for (int i = 0; i < d.nrgeom; ++i)
      if (fixed_in_world(m, bits_int(rgeom[8 * i + 2]))) d.rf_static_mask |= 1u << i;
  return rgeom;
}

// ray blocks (kRayBlock consecutive rangefinders) for the level-1 cull.  When every ray of a block
// starts at the same point of the same body the block is bounded by a fan fixed in that body's
// frame: unit axis a, in-plane direction b and normal c (the least-spread direction of the rays),
// in-plane half-angle theta around a and out-of-plane slope eps = max |d.c| (a planar lidar fan
// has eps ~ 0).  Blocks without a common origin, or wider than +-80 degrees, test every geom.
// Record: body, flag, origin[3], a[3], b[3], c[3], cos(theta), sin(theta); then eps per block.
// Sets nrfblk, rf_common (every block a fan from one point of one body: the pass loop reuses one
// frame) and, for static lidars (rf_static_frame), moves the frames to the world frame in fp64
inline std::vector<float> ray_block_records(const Model& m, const std::vector<int>& rf, DevModel& d) {
  std::vector<float> rfblk, rfblk_eps;
  d.nrfblk = 0;
  if (d.nrgeom <= 32 && d.nrf > 0) {
    d.nrfblk = (d.nrf + kRayBlock - 1) / kRayBlock;
    for (int blk = 0; blk < d.nrfblk; ++blk) {
      const int k0 = blk * kRayBlock, k1 = std::min(d.nrf, k0 + kRayBlock);
      const int site0 = m.sensor_objid[rf[k0]], body = m.site_bodyid[site0];
      bool ok = true;
      std::vector<std::array<double, 3>> dirs;
      double axis[3] = {0, 0, 0}, cov[3][3] = {};
      for (int k = k0; k < k1; ++k) {
        const int site = m.sensor_objid[rf[k]];
        if (m.site_bodyid[site] != body) ok = false;
        for (int i = 0; i < 3; ++i)
          if (std::abs(m.site_pos[3 * site + i] - m.site_pos[3 * site0 + i]) > 1e-9) ok = false;
        const std::array<double, 3> dz = site_z_axis(m, site);
        for (int i = 0; i < 3; ++i) axis[i] += dz[i];
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) cov[i][j] += dz[i] * dz[j];
        dirs.push_back(dz);
      }
      double an = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
      double c[3] = {0, 0, 1}, bv[3] = {0, 1, 0}, theta = 0, eps = 0;
      if (an < 1e-6) ok = false;
      if (ok) {
        for (int i = 0; i < 3; ++i) axis[i] /= an;
        smallest_eigvec(cov, c);
        const double ca = c[0] * axis[0] + c[1] * axis[1] + c[2] * axis[2];
        for (int i = 0; i < 3; ++i) c[i] -= ca * axis[i];
        const double cn = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        if (cn < 1e-6) ok = false;
        else {
          for (int i = 0; i < 3; ++i) c[i] /= cn;
          bv[0] = c[1] * axis[2] - c[2] * axis[1];
          bv[1] = c[2] * axis[0] - c[0] * axis[2];
          bv[2] = c[0] * axis[1] - c[1] * axis[0];
          for (auto& dz : dirs) {
            const double da = dz[0] * axis[0] + dz[1] * axis[1] + dz[2] * axis[2];
            const double db = dz[0] * bv[0] + dz[1] * bv[1] + dz[2] * bv[2];
            const double dc = dz[0] * c[0] + dz[1] * c[1] + dz[2] * c[2];
            theta = std::max(theta, std::abs(std::atan2(db, da)));
            eps = std::max(eps, std::abs(dc));
          }
          if (theta > 1.4) ok = false;
        }
      }
      rfblk.insert(rfblk.end(), {int_bits(body), int_bits(ok ? 1 : 0), static_cast<float>(m.site_pos[3 * site0]),
                                 static_cast<float>(m.site_pos[3 * site0 + 1]), static_cast<float>(m.site_pos[3 * site0 + 2]),
                                 static_cast<float>(axis[0]), static_cast<float>(axis[1]), static_cast<float>(axis[2]),
                                 static_cast<float>(bv[0]), static_cast<float>(bv[1]), static_cast<float>(bv[2]),
                                 static_cast<float>(c[0]), static_cast<float>(c[1]), static_cast<float>(c[2]),
                                 static_cast<float>(std::cos(theta + 1e-4)), static_cast<float>(std::sin(theta + 1e-4))});
      rfblk_eps.push_back(static_cast<float>(eps + 1e-6));
    }
  }
  rfblk.insert(rfblk.end(), rfblk_eps.begin(), rfblk_eps.end());
  d.rf_common = d.nrfblk > 0 ? 1 : 0;
  for (int blk = 0; blk < d.nrfblk && d.rf_common; ++blk) {
    const float* r0 = &rfblk[0];
    const float* ri = &rfblk[16 * blk];
    if (!bits_int(ri[1]) || std::memcmp(&ri[0], &r0[0], 4) != 0 || ri[2] != r0[2] || ri[3] != r0[3] || ri[4] != r0[4]) d.rf_common = 0;
  }
  if (d.rf_static_frame)
    for (int blk = 0; blk < d.nrfblk; ++blk) {
      float* r = &rfblk[16 * blk];
      double R[9], p[3];
      body_world(m, bits_int(r[0]), R, p);
      for (int v = 0; v < 4; ++v) {  // origin (a point), then a, b, c (directions)
        const double x[3] = {r[2 + 3 * v], r[3 + 3 * v], r[4 + 3 * v]};
        for (int i = 0; i < 3; ++i)
          r[2 + 3 * v + i] = static_cast<float>(R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2] + (v == 0 ? p[i] : 0.0));
      }
    }
  return rfblk;
}

// per-ray records, 8 floats: unit direction (z column of the site rotation) and sensordata address
// first (one 16-byte load when the ray's pass shares body and origin), then body and origin in the body
// frame (the world frame for static lidars)
inline std::vector<float> ray_records(const Model& m, const std::vector<int>& rf, const DevModel& d) {
  std::vector<float> rfray;
  for (int k = 0; k < d.nrf; ++k) {
    const int site = m.sensor_objid[rf[k]];
    const std::array<double, 3> dz = site_z_axis(m, site);
    double dir[3] = {dz[0], dz[1], dz[2]}, org[3] = {m.site_pos[3 * site], m.site_pos[3 * site + 1], m.site_pos[3 * site + 2]};
    if (d.rf_static_frame) {
      double R[9], p[3];
      body_world(m, m.site_bodyid[site], R, p);
      const double d0[3] = {dir[0], dir[1], dir[2]}, o0[3] = {org[0], org[1], org[2]};
      for (int i = 0; i < 3; ++i) {
        dir[i] = R[3 * i] * d0[0] + R[3 * i + 1] * d0[1] + R[3 * i + 2] * d0[2];
        org[i] = p[i] + R[3 * i] * o0[0] + R[3 * i + 1] * o0[1] + R[3 * i + 2] * o0[2];
      }
    }
    rfray.insert(rfray.end(), {static_cast<float>(dir[0]), static_cast<float>(dir[1]), static_cast<float>(dir[2]),
                               int_bits(m.sensor_adr[rf[k]]), int_bits(m.site_bodyid[site]),
                               static_cast<float>(org[0]), static_cast<float>(org[1]), static_cast<float>(org[2])});
  }
  return rfray;
}

// ------------------------------------------------------------------ the whole model
// The order of the add calls is the layout of the two blocks.
inline DevTables build_tables(const Model& m, int max_con_req, const Overrides& o) {
  if (m.nv > 64) throw UnsupportedError("nv > 64 is not supported by the one-wave-per-env kernel");
  DevTables T;
  DevModel& d = T.dm;
  using D = DevModel;
  model_counts(m, o, d);
  const TreeLists trees = tree_lists(m, o, d);
  // every count below (contact and row capacity, pipe width) is the full list's; the device tables,
  // DevModel::npair and the host copies are the walked list's
  const PairTables all_pairs = collision_pairs(m, d);
  const PairTables pairs = prune_pairs(m, all_pairs, o);
  T.pairs_pruned = static_cast<int>(all_pairs.g1.size() - pairs.g1.size());
  for (size_t q = 0; q < all_pairs.g1.size(); ++q) {
    const int t1 = m.geom_type[all_pairs.g1[q]], t2 = m.geom_type[all_pairs.g2[q]];
    auto conv = [](int t) { return t == MRS_GEOM_ELLIPSOID || t == MRS_GEOM_CYLINDER || t == MRS_GEOM_MESH; };
    if (t1 != MRS_GEOM_PLANE && t2 != MRS_GEOM_PLANE && (conv(t1) || conv(t2))) T.convex_pairs = true;
  }
  T.pair_g1 = pairs.g1;
  T.pair_g2 = pairs.g2;
  T.pair_dim = pairs.dim;
  T.pair_mu.resize(pairs.g1.size());
  for (size_t q = 0; q < pairs.g1.size(); ++q) T.pair_mu[q] = pairs.fric[3 * q];
  const EqTables eq = equality_tables(m, d);
  const TendonTables ten = tendon_tables(m, d);
  // rows outside the blocked-mode sparse solver's kinds (equality, tendon friction / limits): the
  // dense row path runs instead
  d.xrows = d.neq + d.nten_fric + d.nten_lim;
  const KinTrees kt = kinematic_trees(m, all_pairs, d);
  const RowLists rows = row_lists(m, all_pairs, max_con_req, d);
  d.npair = static_cast<int>(pairs.g1.size());
  const ActTables act = actuator_tables(m, d);

  T.addi(&D::body_parentid, m.body_parentid); T.addi(&D::body_rootid, m.body_rootid);
  T.addi(&D::body_jntnum, m.body_jntnum); T.addi(&D::body_jntadr, m.body_jntadr);
  T.addi(&D::body_dofnum, m.body_dofnum); T.addi(&D::body_dofadr, m.body_dofadr);
  T.addi(&D::body_subtree_end, trees.subtree_end); T.addi(&D::level_adr, trees.level_adr);
  T.addi(&D::level_num, trees.level_num); T.addi(&D::level_body, trees.level_body); T.addi(&D::jump, trees.jump);
  T.addf(&D::body_pos, m.body_pos); T.addf(&D::body_quat, m.body_quat); T.addf(&D::body_ipos, m.body_ipos);
  T.addf(&D::body_iquat, m.body_iquat); T.addf(&D::body_mass, m.body_mass);
  T.addf(&D::body_subtreemass, m.body_subtreemass); T.addf(&D::body_inertia, m.body_inertia);
  T.addf(&D::body_gravcomp, m.body_gravcomp); T.addf(&D::body_invweight0, m.body_invweight0);
  T.addi(&D::jnt_type, m.jnt_type); T.addi(&D::jnt_qposadr, m.jnt_qposadr); T.addi(&D::jnt_dofadr, m.jnt_dofadr);
  T.addi(&D::jnt_bodyid, m.jnt_bodyid); T.addi(&D::jnt_actfrclimited, m.jnt_actfrclimited);
  T.addf(&D::jnt_pos, m.jnt_pos); T.addf(&D::jnt_axis, m.jnt_axis); T.addf(&D::jnt_stiffness, m.jnt_stiffness);
  T.addf(&D::jnt_range, m.jnt_range); T.addf(&D::jnt_margin, m.jnt_margin); T.addf(&D::jnt_solref, m.jnt_solref);
  T.addf(&D::jnt_solimp, m.jnt_solimp); T.addf(&D::jnt_actfrcrange, m.jnt_actfrcrange);
  T.addi(&D::dof_bodyid, m.dof_bodyid); T.addi(&D::dof_jntid, m.dof_jntid);
  T.addf(&D::dof_armature, m.dof_armature); T.addf(&D::dof_damping, m.dof_damping);
  T.addf(&D::dof_frictionloss, m.dof_frictionloss); T.addf(&D::dof_solref, m.dof_solref);
  T.addf(&D::dof_solimp, m.dof_solimp); T.addf(&D::dof_invweight0, m.dof_invweight0);
  T.addf(&D::qpos0, m.qpos0); T.addf(&D::qpos_spring, m.qpos_spring);
  T.addi(&D::Mpair, trees.Mpair);
  T.addi(&D::body_tree, kt.body_tree); T.addi(&D::dof_tree, kt.dof_tree); T.addi(&D::tree_dofadr, kt.dofadr);
  T.addi(&D::tree_dofnum, kt.dofnum); T.addi(&D::tree_Moff, kt.Moff);
  T.addi(&D::geom_type, m.geom_type); T.addi(&D::geom_bodyid, m.geom_bodyid); T.addi(&D::geom_group, m.geom_group);
  T.addi(&D::geom_dataid, m.geom_dataid);
  const MeshTables mesh = mesh_tables(m, o);
  T.addi(&D::mesh_vertadr, m.mesh_vertadr); T.addi(&D::mesh_faceadr, m.mesh_faceadr); T.addi(&D::mesh_facenum, m.mesh_facenum);
  T.addi(&D::mesh_hulladr, m.mesh_hulladr); T.addi(&D::mesh_hullnum, m.mesh_hullnum); T.addi(&D::mesh_face, mesh.face);
  T.addi(&D::mesh_bvhadr, mesh.bvh_adr); T.addi(&D::mesh_bvhnum, mesh.bvh_num); T.addf(&D::mesh_bvh, mesh.bvh_node);
  T.addi(&D::mesh_hull, m.mesh_hull); T.addf(&D::mesh_vert, m.mesh_vert);
  T.addi(&D::mesh_polyadr, m.mesh_polyadr); T.addi(&D::mesh_polynum, m.mesh_polynum);
  T.addi(&D::mesh_polyvertadr, m.mesh_polyvertadr); T.addi(&D::mesh_polyvertnum, m.mesh_polynum_v);
  T.addi(&D::mesh_polyvert, m.mesh_polyvert); T.addf(&D::mesh_polynormal, m.mesh_polynormal);
  T.addf(&D::mesh_tri, mesh.tri);
  std::vector<int> rast_geom, rast_base;
  raster_lists(m, d, rast_geom, rast_base);
  T.addi(&D::rast_geom, rast_geom); T.addi(&D::rast_base, rast_base);
  T.addf(&D::geom_size, m.geom_size); T.addf(&D::geom_pos, m.geom_pos); T.addf(&D::geom_quat, m.geom_quat);
  T.addf(&D::geom_rbound, m.geom_rbound); T.addf(&D::geom_rgba, m.geom_rgba);
  T.addf(&D::rlit, lit_block(m, d));
  std::vector<int> matid(m.ngeom, -1);
  for (int g = 0; g < m.ngeom && g < static_cast<int>(m.geom_matid.size()); ++g) matid[g] = m.geom_matid[g];
  T.addi(&D::geom_matid, matid);
  T.addi(&D::pair_g1, pairs.g1); T.addi(&D::pair_g2, pairs.g2); T.addi(&D::pair_dim, pairs.dim);
  T.addi(&D::ten_adr, ten.adr); T.addi(&D::ten_num, ten.num); T.addi(&D::wrap_qadr, ten.wrap_qadr);
  T.addi(&D::wrap_dof, ten.wrap_dof); T.addf(&D::wrap_coef, ten.coef); T.addf(&D::ten_J, ten.J);
  T.addf(&D::ten_prm, ten.prm); T.addi(&D::ten_fric, ten.fric); T.addi(&D::ten_lim, ten.lim);
  T.addf(&D::ten_solref_lim, m.tendon_solref_lim); T.addf(&D::ten_solimp_lim, m.tendon_solimp_lim);
  T.addf(&D::ten_solref_fri, m.tendon_solref_fri); T.addf(&D::ten_solimp_fri, m.tendon_solimp_fri);
  T.addi(&D::act_ten, act.ten);
  T.addi(&D::eq_type, eq.type); T.addi(&D::eq_obj1id, eq.obj1); T.addi(&D::eq_obj2id, eq.obj2);
  T.addf(&D::eq_solref, eq.solref); T.addf(&D::eq_solimp, eq.solimp); T.addf(&D::eq_data, eq.data);
  T.addf(&D::pair_margin, pairs.margin); T.addf(&D::pair_gap, pairs.gap); T.addf(&D::pair_friction, pairs.fric);
  T.addf(&D::pair_solref, pairs.solref); T.addf(&D::pair_solimp, pairs.solimp);
  T.addi(&D::site_bodyid, m.site_bodyid); T.addf(&D::site_pos, m.site_pos); T.addf(&D::site_quat, m.site_quat);
  T.addi(&D::cam_bodyid, m.cam_bodyid); T.addf(&D::cam_pos, m.cam_pos); T.addf(&D::cam_quat, m.cam_quat);
  T.addi(&D::act_dof, act.dof); T.addi(&D::act_qadr, act.qadr);
  T.addi(&D::act_gaintype, m.actuator_gaintype); T.addi(&D::act_biastype, m.actuator_biastype);
  T.addi(&D::act_ctrllimited, m.actuator_ctrllimited); T.addi(&D::act_forcelimited, m.actuator_forcelimited);
  T.addf(&D::act_gear, act.gear); T.addf(&D::act_gainprm, act.gain); T.addf(&D::act_biasprm, act.bias);
  T.addf(&D::act_ctrlrange, m.actuator_ctrlrange); T.addf(&D::act_forcerange, m.actuator_forcerange);
  T.addi(&D::sensor_type, m.sensor_type); T.addi(&D::sensor_objtype, m.sensor_objtype);
  T.addi(&D::sensor_objid, m.sensor_objid); T.addi(&D::sensor_adr, m.sensor_adr); T.addi(&D::sensor_dim, m.sensor_dim);
  T.addf(&D::sensor_cutoff, m.sensor_cutoff);
  T.addi(&D::fric_dof, rows.fric); T.addi(&D::lim_jnt, rows.lim); T.addi(&D::rf_sensor, rows.rf);
  T.addi(&D::sens_other, rows.other_sens);

  std::vector<float> fricrec, limrec, bodytab, mpairtab, kb, kj, kg;
  row_records(m, rows, d.timestep, fricrec, limrec);
  T.addf(&D::fricrec, fricrec);
  T.addf(&D::limrec, limrec);
  const SmoothRecords smooth = smooth_force_records(m, act, ten, trees, rows);
  T.addf(&D::actrec, smooth.actrec);
  T.addf(&D::actdyn, smooth.actdyn);
  T.addf(&D::dofrec, smooth.dofrec);
  tree_records(m, trees, bodytab, mpairtab);
  T.addf(&D::bodytab, bodytab);
  T.addf(&D::mpairtab, mpairtab);
  kinematics_records(m, kb, kj, kg);
  T.addf(&D::kinbody, kb);
  T.addf(&D::kinjnt, kj);
  T.addf(&D::kingeom, kg);
  T.addf(&D::sensrec, sensor_records(m, rows, trees));
  // static lidars: when every rangefinder sits on a body fixed in the world, that body's world pose
  // never changes, so the ray blocks' fan frames and the rays' origins / directions go to the world
  // frame (fp64) and the step kernel skips the per-step body rotation (rf_static_frame)
  T.rf = rows.rf;
  T.rf_fixed = d.nrf > 0;
  for (int s : T.rf) T.rf_fixed = T.rf_fixed && fixed_in_world(m, m.site_bodyid[m.sensor_objid[s]]);
  d.rf_static_frame = T.rf_fixed && !o.no_static_frame ? 1 : 0;
  T.addf(&D::rgeom, ray_geom_records(m, d));
  T.addf(&D::rfblk, ray_block_records(m, T.rf, d));
  T.addf(&D::rfray, ray_records(m, T.rf, d));
  // spatial tendons, after every table a model without one has (their offsets stay what they were)
  if (d.nten_spatial > 0) {
    T.addi(&D::tsp_ten, ten.sp_ten); T.addi(&D::tsp_adr, ten.sp_adr); T.addi(&D::tsp_num, ten.sp_num);
    T.addi(&D::ten_sp, ten.sp_of); T.addf(&D::tsp_seg, ten.sp_seg);
  }
  // site actuators, likewise after every table a model without one has
  if (d.nact_site > 0) T.addf(&D::sact, act.site);
  return T;
}

// ------------------------------------------------------------------ the shared tables as one image
// floats of the image a launch copies: the staged tables end at shr_flag (the helper waves' signal words
// after them are the kernel's own), in blocked mode at shr_act
inline int shared_image_floats(const DevModel& d) { return d.blocked ? d.shr_act : d.shr_flag; }

// The workgroup-shared tables of plan d (its shr_* offsets, plan.h shared_layout) packed as the launch
// stages them (DevModel::shr_image): each table at its offset, as long as the gap to the next one --
// rfray as floats 0..3 of each ray's 8 (direction, sensordata address; none without rf_common), jump as
// int bits, the static ray hits' extent zero (the producer pass writes it on the device).  Zero-padded
// to a multiple of 4 floats
inline std::vector<float> pack_shared_image(const DevTables& T, const DevModel& d) {
  using D = DevModel;
  const int n = shared_image_floats(d);
  std::vector<float> img(static_cast<size_t>((n + 3) & ~3), 0.0f);
  // (a blocked plan's tables end at shr_act: the extents from there on are outside the image)
  auto put = [&](int off, int end, const float* src) {
    for (int k = off; k < end && k < n; ++k) img[k] = src[k - off];
  };
  put(0, d.shr_rf, T.table(&D::rgeom));
  const float* rfray = T.table(&D::rfray);
  for (int k = d.shr_rf; k < d.shr_rfst; ++k) {
    const int q = k - d.shr_rf;
    img[k] = rfray[8 * (q >> 2) + (q & 3)];
  }
  put(d.shr_blk, d.shr_sens, T.table(&D::rfblk));
  put(d.shr_sens, d.shr_fric, T.table(&D::sensrec));
  put(d.shr_fric, d.shr_lim, T.table(&D::fricrec));
  put(d.shr_lim, d.shr_act, T.table(&D::limrec));
  put(d.shr_act, d.shr_dof, T.table(&D::actrec));
  put(d.shr_dof, d.shr_body, T.table(&D::dofrec));
  put(d.shr_body, d.shr_mpair, T.table(&D::bodytab));
  put(d.shr_mpair, d.shr_jump, T.table(&D::mpairtab));
  const int* jump = T.itable(&D::jump);
  for (int k = d.shr_jump; k < d.shr_kbody && k < n; ++k) img[k] = int_bits(jump[k - d.shr_jump]);
  put(d.shr_kbody, d.shr_kjnt, T.table(&D::kinbody));
  put(d.shr_kjnt, d.shr_kgeom, T.table(&D::kinjnt));
  put(d.shr_kgeom, d.shr_flag, T.table(&D::kingeom));
  return img;
}

}  // namespace mrs
