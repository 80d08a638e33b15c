// Batch of environments resident on one GPU: model packing, memory layouts, state transfer,
// step/forward launches and the depth-camera kernel.  Host side of the C ABI in include/mrs.h.
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
#include "devmodel.h"
#include "devtables.h"
#include "plan.h"
#include "raymesh.h"
#include "rayfilter.h"
#include "lit.h"
#include "start_rows.h"

namespace mrs {

hipError_t launch_step(const DevModel* d_model, int lds_floats, int shared_floats, const DevState& st, int n_envs,
                       int n_steps, bool forward_only, int group, bool primal, bool ext, bool params, bool dyn,
                       hipStream_t stream);

namespace {

#define HIP_CHECK(x)                                                                         \
  do {                                                                                       \
    hipError_t err_ = (x);                                                                   \
    if (err_ != hipSuccess)                                                                  \
      throw DeviceError(std::string(#x) + " failed: " + hipGetErrorString(err_));            \
  } while (0)

// ------------------------------------------------------------------ depth camera kernel
// One thread per pixel, one env per blockIdx.y; the env's geom poses are staged in LDS.
// Eye-space depth: ray through the pixel centre with camera-frame direction (x, y, -1), so the ray
// parameter of the nearest hit is the eye-space z that OpenGL + the plugin's linearisation
// (src/mujoco_cameras.cpp:222-235) produce; rows in ROS order (flip of :229-240 applied).
constexpr int kMaxRenderGeoms = 256;
// the model's meshes for the render kernels (mrs_model.h mesh arrays, device copies)
struct MeshRef {
  const float* vert;
  const int *face, *dataid, *vertadr, *faceadr, *facenum;
  const float* bvh;           // bounding volume hierarchies (8 floats per node, build_mesh_bvh)
  const int *bvhadr, *bvhnum;  // per mesh: first node, node count (0: no hierarchy, every triangle)
  const float* tri;            // pre-gathered triangle records (DevModel::mesh_tri)
};

// analytic ray primitive (same restatement of engine_ray as the step kernel's rangefinder)
__device__ float ray_prim(int type, const float* s, const float lp[3], const float lv[3]) {
  auto quad = [](float a, float b, float c, float x[2]) {
    float det = b * b - a * c;
    if (det < 1e-15f) { x[0] = x[1] = -1; return -1.0f; }
    det = sqrtf(det);
    x[0] = (-b - det) / a;
    x[1] = (-b + det) / a;
    if (x[0] >= 0) return x[0];
    if (x[1] >= 0) return x[1];
    return -1.0f;
  };
  auto d3 = [](const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
  float x[2];
  switch (type) {
    case MRS_GEOM_PLANE: {
      if (lv[2] >= 0 || lv[2] * lv[2] <= 1e-12f * d3(lv, lv)) return -1;
      float t = -lp[2] / lv[2];
      if (t < 0) return -1;
      float p0 = lp[0] + t * lv[0], p1 = lp[1] + t * lv[1];
      if ((s[0] <= 0 || fabsf(p0) <= s[0]) && (s[1] <= 0 || fabsf(p1) <= s[1])) return t;
      return -1;
    }
    case MRS_GEOM_SPHERE: return quad(d3(lv, lv), d3(lv, lp), d3(lp, lp) - s[0] * s[0], x);
    case MRS_GEOM_CAPSULE: {
      float best = -1;
      float a = lv[0] * lv[0] + lv[1] * lv[1];
      if (a > 1e-15f) {
        quad(a, lv[0] * lp[0] + lv[1] * lp[1], lp[0] * lp[0] + lp[1] * lp[1] - s[0] * s[0], x);
        for (int i = 0; i < 2; ++i)
          if (x[i] >= 0 && fabsf(lp[2] + x[i] * lv[2]) <= s[1] && (best < 0 || x[i] < best)) best = x[i];
      }
      for (int e = -1; e <= 1; e += 2) {
        float q[3] = {lp[0], lp[1], lp[2] - e * s[1]};
        quad(d3(lv, lv), d3(lv, q), d3(q, q) - s[0] * s[0], x);
        for (int i = 0; i < 2; ++i)
          if (x[i] >= 0 && e * (lp[2] + x[i] * lv[2] - e * s[1]) >= 0 && (best < 0 || x[i] < best)) best = x[i];
      }
      return best;
    }
    case MRS_GEOM_ELLIPSOID: {
      float q[3] = {lp[0] / s[0], lp[1] / s[1], lp[2] / s[2]}, v[3] = {lv[0] / s[0], lv[1] / s[1], lv[2] / s[2]};
      return quad(d3(v, v), d3(v, q), d3(q, q) - 1, x);
    }
    case MRS_GEOM_CYLINDER: {
      float best = -1;
      float a = lv[0] * lv[0] + lv[1] * lv[1];
      if (a > 1e-15f) {
        quad(a, lv[0] * lp[0] + lv[1] * lp[1], lp[0] * lp[0] + lp[1] * lp[1] - s[0] * s[0], x);
        for (int i = 0; i < 2; ++i)
          if (x[i] >= 0 && fabsf(lp[2] + x[i] * lv[2]) <= s[1] && (best < 0 || x[i] < best)) best = x[i];
      }
      if (fabsf(lv[2]) > 1e-15f)
        for (int e = -1; e <= 1; e += 2) {
          float t = (e * s[1] - lp[2]) / lv[2];
          if (t < 0) continue;
          float p0 = lp[0] + t * lv[0], p1 = lp[1] + t * lv[1];
          if (p0 * p0 + p1 * p1 <= s[0] * s[0] && (best < 0 || t < best)) best = t;
        }
      return best;
    }
    case MRS_GEOM_BOX: {
      float best = -1;
      for (int i = 0; i < 3; ++i) {
        if (fabsf(lv[i]) <= 1e-15f) continue;
        int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        for (int side = -1; side <= 1; side += 2) {
          float t = (side * s[i] - lp[i]) / lv[i];
          if (t < 0) continue;
          float p1 = lp[i1] + t * lv[i1], p2 = lp[i2] + t * lv[i2];
          if (fabsf(p1) <= s[i1] && fabsf(p2) <= s[i2] && (best < 0 || t < best)) best = t;
        }
      }
      return best;
    }
  }
  return -1;
}

#include "rayquery.h"

// ---- colour: the lit model of lit.h (oracle.c lit_color restates it in fp64); local_normal gives
// the geom-frame surface normal (unnormalised) at a hit point p
__device__ __forceinline__ void local_normal(int type, const float* s, const float p[3], float n[3]) {
  n[0] = 0; n[1] = 0; n[2] = 1;
  switch (type) {
    case MRS_GEOM_SPHERE: n[0] = p[0]; n[1] = p[1]; n[2] = p[2]; break;
    case MRS_GEOM_CAPSULE: n[0] = p[0]; n[1] = p[1]; n[2] = p[2] - fminf(fmaxf(p[2], -s[1]), s[1]); break;
    case MRS_GEOM_ELLIPSOID: n[0] = p[0] / (s[0] * s[0]); n[1] = p[1] / (s[1] * s[1]); n[2] = p[2] / (s[2] * s[2]); break;
    case MRS_GEOM_CYLINDER: {
      const float rr = sqrtf(p[0] * p[0] + p[1] * p[1]);
      if (fabsf(p[2]) - s[1] > rr - s[0]) { n[0] = 0; n[1] = 0; n[2] = p[2] >= 0 ? 1.0f : -1.0f; }
      else { n[0] = p[0]; n[1] = p[1]; n[2] = 0; }
      break;
    }
    case MRS_GEOM_BOX: {
      int k = 0;
      float best = fabsf(p[0]) / s[0];
      for (int i = 1; i < 3; ++i)
        if (fabsf(p[i]) / s[i] > best) { best = fabsf(p[i]) / s[i]; k = i; }
      n[0] = 0; n[1] = 0; n[2] = 0;
      n[k] = p[k] >= 0 ? 1.0f : -1.0f;
      break;
    }
    default: break;
  }
}

// One workgroup renders a 16x16-pixel tile of one env.  The tile's pixel rays lie inside a cone
// (apex at the camera, axis through the tile centre, half-angle to the widest corner ray); a geom
// whose bounding sphere misses that cone, or a plane no ray of the cone can reach, is skipped by the
// whole tile, and the pixels test only the remaining candidates.  Culling only removes geoms no pixel
// ray can hit, so every pixel keeps the nearest hit over all geoms.
template <bool kRGB>
__global__ __launch_bounds__(256) void depth_kernel(const int* geom_type, const int* geom_group,
                                                    const float* geom_size, const float* geom_rbound,
                                                    const float* geom_rgba, int ngeom, const float* geom_xpos,
                                                    const float* geom_xmat, const float* cam_xpos,
                                                    const float* cam_xmat, int ncam, int cam, int env0, int W,
                                                    int H, float f, float znear, float zfar, float* out,
                                                    unsigned char* rgb, MeshRef mesh, LitRef lr) {
  __shared__ float gp[kMaxRenderGeoms * 3];
  __shared__ LitFrame LF;
  __shared__ float gm[kMaxRenderGeoms * 9];
  __shared__ float cpos[3], cmat[9];
  __shared__ int cand[kMaxRenderGeoms];
  __shared__ int ncand;
  const int env = env0 + blockIdx.y;
  const size_t eo = (size_t)env;
  for (int i = threadIdx.x; i < 3 * ngeom; i += blockDim.x) gp[i] = geom_xpos[eo * 3 * ngeom + i];
  for (int i = threadIdx.x; i < 9 * ngeom; i += blockDim.x) gm[i] = geom_xmat[eo * 9 * ngeom + i];
  if (threadIdx.x < 3) cpos[threadIdx.x] = cam_xpos[(eo * ncam + cam) * 3 + threadIdx.x];
  if (threadIdx.x < 9) cmat[threadIdx.x] = cam_xmat[(eo * ncam + cam) * 9 + threadIdx.x];
  if (threadIdx.x == 0) ncand = 0;
  if (kRGB && threadIdx.x == 255)
    lit_stage(LF, lr, cam_xpos + (eo * ncam + cam) * 3, cam_xmat + (eo * ncam + cam) * 9);
  const int tiles_x = (W + 15) / 16;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  __syncthreads();
  if (threadIdx.x < ngeom) {
    const int g = threadIdx.x;
    const int grp = geom_group[g];
    bool keep = !(grp < 0 || grp > 2 || geom_rgba[4 * g + 3] == 0);
    if (keep) {
      // tile cone in the camera frame, then world: axis through the tile centre, cos of the widest
      // corner angle (pixel centres of the tile's extreme rows/columns)
      const float c0 = tx * 16 + 0.5f, c1 = fminf(tx * 16 + 15.0f, W - 1.0f) + 0.5f;
      const float r0 = ty * 16 + 0.5f, r1 = fminf(ty * 16 + 15.0f, H - 1.0f) + 0.5f;
      float ac[3] = {(0.5f * (c0 + c1) - 0.5f * W) / f, (0.5f * H - 0.5f * (r0 + r1)) / f, -1.0f};
      const float an = sqrtf(ac[0] * ac[0] + ac[1] * ac[1] + 1.0f);
      ac[0] /= an; ac[1] /= an; ac[2] /= an;
      float cth = 1.0f;
      for (int k = 0; k < 4; ++k) {
        const float cc = (k & 1) ? c1 : c0, rr = (k & 2) ? r1 : r0;
        const float dx = (cc - 0.5f * W) / f, dy = (0.5f * H - rr) / f;
        const float dn = sqrtf(dx * dx + dy * dy + 1.0f);
        cth = fminf(cth, (dx * ac[0] + dy * ac[1] - ac[2]) / dn);
      }
      cth = fmaxf(-1.0f, cth - 1e-4f);
      const float sth = sqrtf(fmaxf(0.0f, 1.0f - cth * cth));
      const float a[3] = {cmat[0] * ac[0] + cmat[1] * ac[1] + cmat[2] * ac[2],
                          cmat[3] * ac[0] + cmat[4] * ac[1] + cmat[5] * ac[2],
                          cmat[6] * ac[0] + cmat[7] * ac[1] + cmat[8] * ac[2]};
      const float v[3] = {gp[3 * g] - cpos[0], gp[3 * g + 1] - cpos[1], gp[3 * g + 2] - cpos[2]};
      if (geom_type[g] == MRS_GEOM_PLANE) {
        // origin in front of the plane and some direction of the cone with d.n < 0:
        // min over the cone of d.n = cos(angle(a, n) + theta)
        const float n[3] = {gm[9 * g + 2], gm[9 * g + 5], gm[9 * g + 8]};
        const float an2 = a[0] * n[0] + a[1] * n[1] + a[2] * n[2];
        const float mind = an2 * cth - sqrtf(fmaxf(0.0f, 1.0f - an2 * an2)) * sth;
        keep = -(v[0] * n[0] + v[1] * n[1] + v[2] * n[2]) > 0 && mind < 1e-6f;
      } else {
        const float rb = geom_rbound[g] * 1.001f + 1e-4f;
        const float l2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        if (l2 > rb * rb) {
          // angle(v, a) <= theta + asin(rb/|v|)  <=>  v.a >= |v| cos(theta) cos(beta) - rb sin(theta)
          const float l = sqrtf(l2);
          const float va = v[0] * a[0] + v[1] * a[1] + v[2] * a[2];
          keep = va >= cth * sqrtf(l2 - rb * rb) - sth * rb - 1e-6f * l;
        }
      }
    }
    if (keep) cand[atomicAdd(&ncand, 1)] = g;
  }
  __syncthreads();
  const int row = ty * 16 + threadIdx.x / 16, col = tx * 16 + threadIdx.x % 16;
  if (row >= H || col >= W) return;
  const int pix = row * W + col;
  const float dc[3] = {(col + 0.5f - 0.5f * W) / f, (0.5f * H - row - 0.5f) / f, -1.0f};
  const float vec[3] = {cmat[0] * dc[0] + cmat[1] * dc[1] + cmat[2] * dc[2],
                        cmat[3] * dc[0] + cmat[4] * dc[1] + cmat[5] * dc[2],
                        cmat[6] * dc[0] + cmat[7] * dc[1] + cmat[8] * dc[2]};
  const float vv = vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2];
  float best = -1;
  int bestg = -1;
  const int nc = ncand;
  for (int i = 0; i < nc; ++i) {
    const int g = cand[i];
    const float* p = gp + 3 * g;
    const float* mm = gm + 9 * g;
    const float dv[3] = {cpos[0] - p[0], cpos[1] - p[1], cpos[2] - p[2]};
    const int t = geom_type[g];
    if (t != MRS_GEOM_PLANE) {
      // bounding-sphere reject: closest approach of the ray to the geom centre
      const float dvv = dv[0] * vec[0] + dv[1] * vec[1] + dv[2] * vec[2];
      const float dd = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];
      const float rb = geom_rbound[g];
      if (dd - dvv * dvv / vv > rb * rb) continue;
    }
    const float lp[3] = {mm[0] * dv[0] + mm[3] * dv[1] + mm[6] * dv[2], mm[1] * dv[0] + mm[4] * dv[1] + mm[7] * dv[2],
                         mm[2] * dv[0] + mm[5] * dv[1] + mm[8] * dv[2]};
    const float lv[3] = {mm[0] * vec[0] + mm[3] * vec[1] + mm[6] * vec[2],
                         mm[1] * vec[0] + mm[4] * vec[1] + mm[7] * vec[2],
                         mm[2] * vec[0] + mm[5] * vec[1] + mm[8] * vec[2]};
    float tt;
    if (t == MRS_GEOM_MESH) {
      const int id = mesh.dataid[g];
      int tri;
      tt = ray_mesh(mesh.tri + 9 * mesh.faceadr[id], mesh.facenum[id], geom_size + 3 * g, lp, lv,
                    mesh.bvh + 8 * mesh.bvhadr[id], mesh.bvhnum[id], &tri);
    } else {
      tt = ray_prim(t, geom_size + 3 * g, lp, lv);
    }
    if (tt >= znear && (best < 0 || tt < best)) { best = tt; bestg = g; }
  }
  const bool hit = !(best < 0 || best > zfar);
  out[(size_t)blockIdx.y * W * H + pix] = hit ? best : zfar;
  if constexpr (kRGB) {
    unsigned char* px = rgb + ((size_t)blockIdx.y * W * H + pix) * 3;
    if (!hit) { lit_sky(LF, dc[0], dc[1], px); return; }
    const float* p = gp + 3 * bestg;
    const float* mm = gm + 9 * bestg;
    const float dv[3] = {cpos[0] - p[0], cpos[1] - p[1], cpos[2] - p[2]};
    float q[3], nl[3], nw[3], nc[3];
    for (int i = 0; i < 3; ++i)
      q[i] = mm[i] * dv[0] + mm[3 + i] * dv[1] + mm[6 + i] * dv[2] +
             best * (mm[i] * vec[0] + mm[3 + i] * vec[1] + mm[6 + i] * vec[2]);
    if (geom_type[bestg] == MRS_GEOM_MESH) {  // the hit triangle's normal, facing the ray
      const int id = mesh.dataid[bestg];
      const float* mv = mesh.vert + 3 * mesh.vertadr[id];
      const int* mf = mesh.face + 3 * mesh.faceadr[id];
      float lp[3], lv[3];
      for (int i = 0; i < 3; ++i) {
        lp[i] = mm[i] * dv[0] + mm[3 + i] * dv[1] + mm[6 + i] * dv[2];
        lv[i] = mm[i] * vec[0] + mm[3 + i] * vec[1] + mm[6 + i] * vec[2];
      }
      int tri = 0;
      ray_mesh(mesh.tri + 9 * mesh.faceadr[id], mesh.facenum[id], geom_size + 3 * bestg, lp, lv,
               mesh.bvh + 8 * mesh.bvhadr[id], mesh.bvhnum[id], &tri);
      mesh_tri_normal(mv, mf, tri, lv, nl);
    } else {
      local_normal(geom_type[bestg], geom_size + 3 * bestg, q, nl);
    }
    for (int i = 0; i < 3; ++i) nw[i] = mm[3 * i] * nl[0] + mm[3 * i + 1] * nl[1] + mm[3 * i + 2] * nl[2];
    for (int j = 0; j < 3; ++j) nc[j] = cmat[j] * nw[0] + cmat[3 + j] * nw[1] + cmat[6 + j] * nw[2];
    float rgba3[3] = {geom_rgba[4 * bestg], geom_rgba[4 * bestg + 1], geom_rgba[4 * bestg + 2]};
    // shadow rays in the world frame: every geom of groups 0-2 with alpha > 0, bounding-sphere reject
    auto occ = [&](const float* o, const float* L, float dist) {
      float ow[3], lw[3];
      for (int i = 0; i < 3; ++i) {
        ow[i] = cpos[i] + cmat[3 * i] * o[0] + cmat[3 * i + 1] * o[1] + cmat[3 * i + 2] * o[2];
        lw[i] = cmat[3 * i] * L[0] + cmat[3 * i + 1] * L[1] + cmat[3 * i + 2] * L[2];
      }
      for (int g = 0; g < ngeom; ++g) {
        const int grp = geom_group[g];
        if (grp < 0 || grp > 2 || geom_rgba[4 * g + 3] == 0) continue;
        const float* gpp = gp + 3 * g;
        const float* gmm = gm + 9 * g;
        const float d[3] = {ow[0] - gpp[0], ow[1] - gpp[1], ow[2] - gpp[2]};
        const int t = geom_type[g];
        if (t != MRS_GEOM_PLANE) {
          const float rb = geom_rbound[g] * 1.001f + 1e-4f;
          const float pr = -(d[0] * lw[0] + d[1] * lw[1] + d[2] * lw[2]);
          const float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
          if (dd > rb * rb && (pr < 0 || dd - pr * pr > rb * rb)) continue;
        }
        float lp[3], lv[3];
        for (int i = 0; i < 3; ++i) {
          lp[i] = gmm[i] * d[0] + gmm[3 + i] * d[1] + gmm[6 + i] * d[2];
          lv[i] = gmm[i] * lw[0] + gmm[3 + i] * lw[1] + gmm[6 + i] * lw[2];
        }
        float th;
        if (t == MRS_GEOM_MESH) {
          const int id = mesh.dataid[g];
          int tri;
          th = ray_mesh(mesh.tri + 9 * mesh.faceadr[id], mesh.facenum[id], geom_size + 3 * g, lp, lv,
                        mesh.bvh + 8 * mesh.bvhadr[id], mesh.bvhnum[id], &tri);
        } else {
          th = ray_prim(t, geom_size + 3 * g, lp, lv);
        }
        if (th >= 0 && th < dist) return true;
      }
      return false;
    };
    lit_pixel(LF, lr, bestg, rgba3, geom_type[bestg], geom_size + 3 * bestg, q, dc[0], dc[1], best, nc, occ, px);
  }
}

// ---- depth kernel v2 (ngeom <= 64): one workgroup renders a whole frame of one env.  The
// workgroup stages, once per frame, each visible geom's data in LDS: the camera origin in the geom
// frame lp = R'(c - p) and A = R' C (C: camera rotation), so the geom-frame direction of the pixel
// ray (x, y, -1) is lv = A (x, y, -1) -- three FMAs per component per pixel -- and, for the cull,
// the geom's centre and axes in the camera frame with the half extents of an oriented box around it.
// Each wave walks tiles of 64 x 16 pixels: lane = column (every store is 256 contiguous bytes), 16 rows
// per lane.  Per tile, lane g tests geom g against the tile's pyramid of rays (four planes through
// the camera): an oriented box wholly outside one plane, or a plane no corner ray descends onto, is
// skipped; one ballot gives the candidates and the pixel loop visits only those (wave-uniform geom,
// so the primitive test does not diverge by type).  Boxes use the slab test: the same face
// parameters (+-s - lp) / lv as the face-by-face test, nearest non-negative crossing.
#ifndef MRS_DEPTH_TILE_H
#define MRS_DEPTH_TILE_H 16  // measured C4 (2048 frames): 4 rows 2.08 ms, 8 rows 1.70, 16 rows 1.68, 32 rows 2.13
#endif
#ifndef MRS_DEPTH_CHUNK
#define MRS_DEPTH_CHUNK 8  // rows of a tile evaluated together (registers: the chunk's rows only; measured C4 frames alone 1.66 ms at 8, 1.77 at 4 and 16)
#endif
constexpr int kDepthTileW = 64, kDepthTileH = MRS_DEPTH_TILE_H, kDepthGeoms = 64, kDepthChunk = MRS_DEPTH_CHUNK;
static_assert(kDepthTileH % kDepthChunk == 0, "a tile is a whole number of row chunks");
struct DepthGeom {  // 30 words in LDS
  float lp[3], A[9], size[3];  // row i of A = R'C is also the geom's axis i in the camera frame
  float cc[3], ext[3];         // cull: centre in the camera frame, oriented-box half extents
  float rgba[3];               // colour (RGB output)
  int type, vis, dataid;
  int cast;                    // casts shadows (groups 0-2, alpha > 0; no frustum cull)
};
__device__ __forceinline__ float ray_box_slab(const float* s, const float lp[3], const float lv[3]) {
  float tmin = -3.0e38f, tmax = 3.0e38f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float inv = __builtin_amdgcn_rcpf(lv[i]);
    const bool par = fabsf(lv[i]) <= 1e-15f;
    const float t1 = (-s[i] - lp[i]) * inv, t2 = (s[i] - lp[i]) * inv;
    // a ray parallel to a slab is inside it for all t or for none
    const bool inside = fabsf(lp[i]) <= s[i];
    const float lo = par ? (inside ? -3.0e38f : 3.0e38f) : fminf(t1, t2);
    const float hi = par ? (inside ? 3.0e38f : -3.0e38f) : fmaxf(t1, t2);
    tmin = fmaxf(tmin, lo);
    tmax = fminf(tmax, hi);
  }
  if (tmax < tmin || tmax < 0) return -1;
  return tmin >= 0 ? tmin : tmax;
}
// one visible-geom record of a frame (lane g of the frame's workgroup): the camera origin and the pixel
// ray directions in the geom frame, the geom's culling box in the camera frame, its colour and type
__device__ __forceinline__ void stage_depth_geom(DepthGeom* G, const int* geom_type, const int* geom_group,
                                                 const float* geom_size, const float* geom_rgba, int ngeom,
                                                 const float* geom_xpos, const float* geom_xmat, const float* cp,
                                                 const float* cm, size_t eo, float znear, float zfar, MeshRef mesh) {
  if (threadIdx.x < ngeom) {
    const int g = threadIdx.x;
    const float cpos[3] = {cp[0], cp[1], cp[2]};
    float C[9];
    for (int i = 0; i < 9; ++i) C[i] = cm[i];
    DepthGeom& o = G[g];
    const int grp = geom_group[g];
    o.vis = !(grp < 0 || grp > 2 || geom_rgba[4 * g + 3] == 0);
    o.cast = o.vis;
    const float* p = geom_xpos + eo * 3 * ngeom + 3 * g;
    const float* R = geom_xmat + eo * 9 * ngeom + 9 * g;
    const float d[3] = {cpos[0] - p[0], cpos[1] - p[1], cpos[2] - p[2]};
    for (int i = 0; i < 3; ++i) o.lp[i] = R[i] * d[0] + R[3 + i] * d[1] + R[6 + i] * d[2];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) o.A[3 * i + j] = R[i] * C[j] + R[3 + i] * C[3 + j] + R[6 + i] * C[6 + j];
    for (int i = 0; i < 3; ++i) {
      o.size[i] = geom_size[3 * g + i];
      o.cc[i] = -(C[i] * d[0] + C[3 + i] * d[1] + C[6 + i] * d[2]);
    }
    o.type = geom_type[g];
    o.dataid = o.type == MRS_GEOM_MESH ? mesh.dataid[g] : -1;
    for (int c = 0; c < 3; ++c) o.rgba[c] = geom_rgba[4 * g + c];
    const float s0 = o.size[0], s1 = o.size[1], s2 = o.size[2];
    float e[3] = {s0, s0, s0};
    switch (o.type) {
      case MRS_GEOM_BOX: case MRS_GEOM_ELLIPSOID: case MRS_GEOM_MESH: e[0] = s0; e[1] = s1; e[2] = s2; break;
      case MRS_GEOM_CAPSULE: e[2] = s1 + s0; break;
      case MRS_GEOM_CYLINDER: e[2] = s1; break;
      default: break;
    }
    for (int i = 0; i < 3; ++i) o.ext[i] = e[i] * 1.001f + 1e-4f;
    if (o.type == MRS_GEOM_PLANE && !(o.lp[2] > 0)) o.vis = 0;  // camera behind the plane
    if (o.type != MRS_GEOM_PLANE) {
      // view-axis extent of the oriented box: a geom wholly nearer than znear (e.g. the robot's own
      // body behind the camera) or wholly beyond zfar gives no pixel its depth -- hits nearer than
      // znear are discarded and hits beyond zfar read as zfar -- so it is dropped for the frame
      float rz = 0;
      for (int i = 0; i < 3; ++i) rz += o.ext[i] * fabsf(o.A[3 * i + 2]);
      const float zc = -o.cc[2];  // eye depth of the centre
      if (zc + rz < znear || zc - rz > zfar) o.vis = 0;
    }
  }
}
// shadow ray of the camera-frame kernels (lit_pixel's occluded): does a shadow-casting geom cross
// o + s L, 0 <= s < dist?  Geom-frame ray through the staged lp and A (a camera-frame point o maps to
// lp + A o); a bounding-sphere reject on the culling box first.  Oracle: ray_scene over groups 0-2.
template <bool kMesh = true>
__device__ inline bool occluded_staged(const DepthGeom* G, int ngeom, const MeshRef& mesh, const float o[3],
                                       const float L[3], float dist) {
  for (int k = 0; k < ngeom; ++k) {
    const DepthGeom& h = G[k];
    if (!h.cast) continue;
    if (h.type != MRS_GEOM_PLANE) {
      const float v[3] = {h.cc[0] - o[0], h.cc[1] - o[1], h.cc[2] - o[2]};
      const float r2 = h.ext[0] * h.ext[0] + h.ext[1] * h.ext[1] + h.ext[2] * h.ext[2];
      const float pr = v[0] * L[0] + v[1] * L[1] + v[2] * L[2];
      const float vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
      if (vv > r2 && (pr < 0 || vv - pr * pr > r2)) continue;  // origin outside, sphere behind or beside
    }
    float lp[3], lv[3];
    for (int i = 0; i < 3; ++i) {
      lp[i] = h.lp[i] + h.A[3 * i] * o[0] + h.A[3 * i + 1] * o[1] + h.A[3 * i + 2] * o[2];
      lv[i] = h.A[3 * i] * L[0] + h.A[3 * i + 1] * L[1] + h.A[3 * i + 2] * L[2];
    }
    float t;
    if (h.type == MRS_GEOM_BOX) t = ray_box_slab(h.size, lp, lv);
    else if (kMesh && h.type == MRS_GEOM_MESH) {
      int tri;
      t = ray_mesh(mesh.tri + 9 * mesh.faceadr[h.dataid], mesh.facenum[h.dataid], h.size, lp, lv,
                   mesh.bvh + 8 * mesh.bvhadr[h.dataid], mesh.bvhnum[h.dataid], &tri);
    } else t = ray_prim(h.type, h.size, lp, lv);
    if (t >= 0 && t < dist) return true;
  }
  return false;
}
#ifdef MRS_DEPTH_STATS
// diagnostics build: tiles, candidate visits and visits whose geom is the nearest hit of some pixel of
// the tile, summed over every frame (printed when the batch is freed)
__device__ unsigned long long g_depth_stats[4];
#endif
#ifndef MRS_DEPTH_MINBLK
#define MRS_DEPTH_MINBLK 1
#endif
// kMesh: the frame has mesh geoms (their per-pixel hierarchy walk, MRS_DEPTH_V2); frames without
// them take the instance without that code, whose registers allow more resident workgroups
template <bool kRGB, bool kMesh>
__global__ __launch_bounds__(256, MRS_DEPTH_MINBLK) void depth_kernel_v2(const int* geom_type, const int* geom_group,
                                                       const float* geom_size, const float* geom_rgba, int ngeom,
                                                       const float* geom_xpos, const float* geom_xmat,
                                                       const float* cam_xpos, const float* cam_xmat, int ncam, int cam,
                                                       int env0, int W, int H, float f, float znear, float zfar,
                                                       float* out, unsigned char* rgb, MeshRef mesh, LitRef lr) {
  __shared__ DepthGeom G[kDepthGeoms];
  __shared__ LitFrame LF;
  const int env = env0 + blockIdx.x;
  const size_t eo = static_cast<size_t>(env);
  const float* cp = cam_xpos + (eo * ncam + cam) * 3;
  const float* cm = cam_xmat + (eo * ncam + cam) * 9;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  stage_depth_geom(G, geom_type, geom_group, geom_size, geom_rgba, ngeom, geom_xpos, geom_xmat, cp, cm, eo, znear, zfar, mesh);
  if (kRGB && threadIdx.x == 64) lit_stage(LF, lr, cp, cm);
  __syncthreads();
  const int tiles_x = (W + kDepthTileW - 1) / kDepthTileW, tiles_y = (H + kDepthTileH - 1) / kDepthTileH;
  float* img = out + static_cast<size_t>(blockIdx.x) * W * H;
  for (int tile = wave; tile < tiles_x * tiles_y; tile += 4) {
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    // extreme pixel-centre ray slopes of the tile (camera frame: x right, y up, -z forward)
    const float x0 = (tx * kDepthTileW + 0.5f - 0.5f * W) / f;
    const float x1 = (fminf(tx * kDepthTileW + kDepthTileW - 1.0f, W - 1.0f) + 0.5f - 0.5f * W) / f;
    const float y1 = (0.5f * H - ty * kDepthTileH - 0.5f) / f;
    const float y0 = (0.5f * H - fminf(ty * kDepthTileH + kDepthTileH - 1.0f, H - 1.0f) - 0.5f) / f;
    bool keep = false;
    if (lane < ngeom && G[lane].vis) {
      const DepthGeom& o = G[lane];
      if (o.type == MRS_GEOM_PLANE) {
        // some corner ray (the minimum of the linear d.n over the tile) must descend onto the plane
        const float n[3] = {o.A[6], o.A[7], o.A[8]};
        const float bx = fminf(x0 * n[0], x1 * n[0]), by = fminf(y0 * n[1], y1 * n[1]);
        keep = bx + by - n[2] < 1e-6f;
      } else {
        // oriented box vs the four side planes n.p >= 0 of the tile pyramid (unnormalised normals:
        // left (1, 0, x0), right (-1, 0, -x1), bottom (0, 1, y0), top (0, -1, -y1))
        auto outside = [&](float nx, float ny, float nz) {
          const float c = nx * o.cc[0] + ny * o.cc[1] + nz * o.cc[2];
          float r = 0;
          for (int i = 0; i < 3; ++i)
            r += o.ext[i] * fabsf(nx * o.A[3 * i] + ny * o.A[3 * i + 1] + nz * o.A[3 * i + 2]);
          return c + r < -1e-5f * (fabsf(c) + r);
        };
        keep = !(outside(1, 0, x0) || outside(-1, 0, -x1) || outside(0, 1, y0) || outside(0, -1, -y1));
      }
    }
    unsigned long long cand = __ballot(keep);
    const int col = tx * kDepthTileW + lane;
    const float dx = (col + 0.5f - 0.5f * W) / f;
    const unsigned long long cand_tile = cand;
    // the tile's rows in chunks of kDepthChunk under the tile's one cull: only a chunk's rows are
    // live in registers (the fully unrolled 16-row tile held ~160 VGPRs, 3 workgroups per CU)
#pragma unroll 1
    for (int r0 = 0; r0 < kDepthTileH; r0 += kDepthChunk) {
    float best[kDepthChunk], dy[kDepthChunk];
    int bestg[kDepthChunk];
#pragma unroll
    for (int k = 0; k < kDepthChunk; ++k) {
      best[k] = -1;
      bestg[k] = 0;
      dy[k] = (0.5f * H - (ty * kDepthTileH + r0 + k) - 0.5f) / f;
    }
    cand = cand_tile;
    while (cand) {
      const int g = __builtin_ctzll(cand);
      cand &= cand - 1;
      const DepthGeom& o = G[g];
      const float lp[3] = {o.lp[0], o.lp[1], o.lp[2]}, sz[3] = {o.size[0], o.size[1], o.size[2]};
      float A[9];
      for (int i = 0; i < 9; ++i) A[i] = o.A[i];
      const int type = o.type;
#pragma unroll
      for (int k = 0; k < kDepthChunk; ++k) {
        float lv[3];
        pixel_ray(A, dx, dy[k], lv);
        float t;
        if (type == MRS_GEOM_BOX) t = ray_box_slab(sz, lp, lv);
        else if (kMesh && type == MRS_GEOM_MESH)
        {
          int tri;
          t = ray_mesh(mesh.tri + 9 * mesh.faceadr[o.dataid], mesh.facenum[o.dataid], sz, lp, lv,
                       mesh.bvh + 8 * mesh.bvhadr[o.dataid], mesh.bvhnum[o.dataid], &tri);
        }
        else t = ray_prim(type, sz, lp, lv);
        if (t >= znear && (best[k] < 0 || t < best[k])) { best[k] = t; bestg[k] = g; }
      }
    }
#ifdef MRS_DEPTH_STATS
    if (r0 == 0) {
      unsigned long long cc = cand_tile, won = 0;
      const int ncand = __popcll(cc);
      while (cc) {
        const int g = __builtin_ctzll(cc);
        cc &= cc - 1;
        bool w = false;
        for (int k = 0; k < kDepthChunk; ++k) w |= best[k] >= 0 && best[k] <= zfar && bestg[k] == g;
        if (__any(w)) ++won;
      }
      if (lane == 0) {
        atomicAdd(&g_depth_stats[0], 1ull);
        atomicAdd(&g_depth_stats[1], static_cast<unsigned long long>(ncand));
        atomicAdd(&g_depth_stats[2], won);
      }
    }
#endif
    if (col < W) {
#pragma unroll
      for (int k = 0; k < kDepthChunk; ++k) {
        const int row = ty * kDepthTileH + r0 + k;
        if (row < H) img[static_cast<size_t>(row) * W + col] = (best[k] < 0 || best[k] > zfar) ? zfar : best[k];
      }
      if constexpr (kRGB) {
        unsigned char* frame = rgb + static_cast<size_t>(blockIdx.x) * W * H * 3;
        for (int k = 0; k < kDepthChunk; ++k) {
          const int row = ty * kDepthTileH + r0 + k;
          if (row >= H) break;
          unsigned char* px = frame + (static_cast<size_t>(row) * W + col) * 3;
          if (best[k] < 0 || best[k] > zfar) { lit_sky(LF, dx, dy[k], px); continue; }
          const int g = bestg[k];
          const DepthGeom& o = G[g];
          // hit point in the geom frame lp + t lv; normal back to the camera frame through A's rows
          float q[3], nl[3], nc[3], lv[3];
          pixel_ray(o.A, dx, dy[k], lv);
          for (int i = 0; i < 3; ++i) q[i] = o.lp[i] + best[k] * lv[i];
          if (kMesh && o.type == MRS_GEOM_MESH) {  // the hit triangle's normal, facing the ray
            const float* mv = mesh.vert + 3 * mesh.vertadr[o.dataid];
            const int* mf = mesh.face + 3 * mesh.faceadr[o.dataid];
            int tri = 0;
            ray_mesh(mesh.tri + 9 * mesh.faceadr[o.dataid], mesh.facenum[o.dataid], o.size, o.lp, lv,
                     mesh.bvh + 8 * mesh.bvhadr[o.dataid], mesh.bvhnum[o.dataid], &tri);
            mesh_tri_normal(mv, mf, tri, lv, nl);
          } else {
            local_normal(o.type, o.size, q, nl);
          }
          for (int j = 0; j < 3; ++j) nc[j] = nl[0] * o.A[j] + nl[1] * o.A[3 + j] + nl[2] * o.A[6 + j];
          lit_pixel(LF, lr, g, o.rgba, o.type, o.size, q, dx, dy[k], best[k], nc,
                    [&](const float* so, const float* sl, float sd) { return occluded_staged<kMesh>(G, ngeom, mesh, so, sl, sd); },
                    px);
        }
      }
    }
    }
  }
}

// ---- frames of scenes with mesh geoms: triangle binning + per-pixel exact hits (depth_kernel_mesh).
// A per-pixel BVH walk (depth_kernel_v2's mesh path) is a chain of dependent node loads per pixel;
// here one workgroup renders one env frame in bands of kBandH rows:
//  1. every triangle of every visible mesh geom is put in camera coordinates once (lane per
//     triangle) and given its conservative pixel box (projected vertices, 1 pixel of margin);
//     triangles off screen, wholly nearer than znear or beyond zfar are dropped;
//  2. the kept triangles are sorted by first band (counting sort: per-band counters in LDS, the list
//     of (triangle, box) records in the frame's global scratch);
//  3. per band: each kept triangle overlapping the band tests the pixel rays of its box inside the
//     band with exactly raymesh.h ray_tri's arithmetic and keeps the nearest per pixel by an LDS
//     64-bit atomic min of (t bits, geom, triangle) -- so the depth of every pixel is bit-identical to
//     the every-triangle loop -- then every pixel of the band adds the primitive geoms (the band's
//     pyramid culls them as depth_kernel_v2's tile does), picks the nearest (ties to the lower geom
//     index, as the serial loop) and writes depth and colour.
// Triangles at or behind the camera plane, or spanning more than kMaxSpan bands, go to a side list
// tested in every band they overlap.
constexpr int kBandH = 8, kMaxBands = 128, kMaxSpan = 4;
constexpr int kRasterFaceBits = 18;  // triangle index bits in a record (mesh geom slot above)

// ray_tri (raymesh.h) with the triangle's vertex a and edges e1, e2 already loaded: the same
// expressions in the same order, so t is bit-identical
__device__ __forceinline__ float ray_tri_v(const float a[3], const float e1[3], const float e2[3], const float lp[3],
                                           const float lv[3]) {
  return mt_core(a, e1, e2, lp, lv);
}

struct TriLoad { float a[3], e1[3], e2[3]; };
__device__ __forceinline__ TriLoad load_tri(const float* rec, int f) {
  TriLoad o;
  for (int i = 0; i < 3; ++i) {
    o.a[i] = rec[9 * f + i];
    o.e1[i] = rec[9 * f + 3 + i];
    o.e2[i] = rec[9 * f + 6 + i];
  }
  return o;
}

// triangle f of mesh geom slot k: its conservative pixel box; 0 dropped, 1 kept, 2 side list
__device__ __forceinline__ int tri_box(const DepthGeom& o, const float* mv, const int* mf, int f, int W, int H, float fpx,
                                       float znear, float zfar, int& c0, int& c1, int& r0, int& r1) {
  const int id[3] = {3 * mf[3 * f], 3 * mf[3 * f + 1], 3 * mf[3 * f + 2]};
  float cmin = 3.0e38f, cmax = -3.0e38f, rmin = 3.0e38f, rmax = -3.0e38f, zmin = 3.0e38f, zmax = -3.0e38f;
  bool behind = false;
  for (int v = 0; v < 3; ++v) {
    const float q[3] = {mv[id[v]] - o.lp[0], mv[id[v] + 1] - o.lp[1], mv[id[v] + 2] - o.lp[2]};
    float c[3];
    for (int j = 0; j < 3; ++j) c[j] = o.A[j] * q[0] + o.A[3 + j] * q[1] + o.A[6 + j] * q[2];
    const float depth = -c[2];
    zmin = fminf(zmin, depth);
    zmax = fmaxf(zmax, depth);
    if (depth < 1e-4f) { behind = true; continue; }
    const float inv = fpx / depth;
    const float col = c[0] * inv + 0.5f * W - 0.5f, row = 0.5f * H - 0.5f - c[1] * inv;
    cmin = fminf(cmin, col); cmax = fmaxf(cmax, col);
    rmin = fminf(rmin, row); rmax = fmaxf(rmax, row);
  }
  // (1e-4 relative slack on the view-depth cull: t along the pixel ray equals the eye depth)
  if (zmax < znear * (1 - 1e-4f) || zmin > zfar * (1 + 1e-4f)) return 0;
  if (behind) { c0 = 0; c1 = W - 1; r0 = 0; r1 = H - 1; return 2; }
  c0 = max(0, static_cast<int>(ceilf(cmin)) - 1);
  c1 = min(W - 1, static_cast<int>(floorf(cmax)) + 1);
  r0 = max(0, static_cast<int>(ceilf(rmin)) - 1);
  r1 = min(H - 1, static_cast<int>(floorf(rmax)) + 1);
  if (c0 > c1 || r0 > r1) return 0;
  return (r1 / kBandH - r0 / kBandH) > kMaxSpan ? 2 : 1;
}

template <bool kRGB>
__global__ __launch_bounds__(256) void depth_kernel_mesh(const int* geom_type, const int* geom_group,
                                                         const float* geom_size, const float* geom_rgba, int ngeom,
                                                         const float* geom_xpos, const float* geom_xmat,
                                                         const float* cam_xpos, const float* cam_xmat, int ncam, int cam,
                                                         int env0, int W, int H, float f, float znear, float zfar,
                                                         float* out, unsigned char* rgb, MeshRef mesh, const int* mgeom,
                                                         const int* mbase, int nmg, int npair,
                                                         unsigned long long* lists, LitRef lr) {
  __shared__ DepthGeom G[kDepthGeoms];
  __shared__ LitFrame LF;
  __shared__ int cnt[kMaxBands + 1], cur[kMaxBands], mg[kDepthGeoms], mb[kDepthGeoms + 1];
  __shared__ int nside, maxspan;
  extern __shared__ unsigned long long band[];  // W x kBandH (t bits << 32 | geom << 24 | triangle)
  const int env = env0 + blockIdx.x;
  const size_t eo = static_cast<size_t>(env);
  const float* cp = cam_xpos + (eo * ncam + cam) * 3;
  const float* cm = cam_xmat + (eo * ncam + cam) * 9;
  const int lane = threadIdx.x & 63, tid = threadIdx.x;
  stage_depth_geom(G, geom_type, geom_group, geom_size, geom_rgba, ngeom, geom_xpos, geom_xmat, cp, cm, eo, znear, zfar, mesh);
  const int nb = (H + kBandH - 1) / kBandH;
  for (int i = tid; i <= nb; i += 256) cnt[i] = 0;
  for (int i = tid; i < nb; i += 256) cur[i] = 0;
  for (int i = tid; i < nmg; i += 256) { mg[i] = mgeom[i]; mb[i] = mbase[i]; }
  if (tid == 0) { mb[nmg] = npair; nside = 0; maxspan = 0; }
  if (kRGB && tid == 64) lit_stage(LF, lr, cp, cm);
  __syncthreads();
  unsigned long long* list = lists + static_cast<size_t>(blockIdx.x) * npair;
  // 1-2: count, then fill the band-sorted list (the side list fills the frame's list from its end)
  for (int pass = 0; pass < 2; ++pass) {
    int k = 0;
    for (int p = tid; p < npair; p += 256) {
      while (p >= mb[k + 1]) ++k;
      const DepthGeom& o = G[mg[k]];
      if (!o.vis) continue;
      const float* mv = mesh.vert + 3 * mesh.vertadr[o.dataid];
      const int* mf = mesh.face + 3 * mesh.faceadr[o.dataid];
      const int fi = p - mb[k];
      int c0, c1, r0, r1;
      const int kind = tri_box(o, mv, mf, fi, W, H, f, znear, zfar, c0, c1, r0, r1);
      if (kind == 0) continue;
      const int b0 = r0 / kBandH;
      if (pass == 0) {
        if (kind == 1) { atomicAdd(&cnt[b0], 1); atomicMax(&maxspan, r1 / kBandH - b0); }
        else atomicAdd(&nside, 1);
      } else {
        // record: triangle (24 bits: slot << kRasterFaceBits | index), c0 (11), c1 - c0 (11), r0 (10),
        // r1 - r0 (8; 255: to the last row, conservative for the side list)
        const unsigned long long rec = static_cast<unsigned long long>((k << kRasterFaceBits) | fi) |
                                       (static_cast<unsigned long long>(c0) << 24) |
                                       (static_cast<unsigned long long>(c1 - c0) << 35) |
                                       (static_cast<unsigned long long>(r0) << 46) |
                                       (static_cast<unsigned long long>(min(r1 - r0, 255)) << 56);
        if (kind == 1) list[cnt[b0] + atomicAdd(&cur[b0], 1)] = rec;
        else list[npair - 1 - atomicAdd(&nside, 1)] = rec;
      }
    }
    __syncthreads();
    if (pass == 0) {
      if (tid == 0) {  // exclusive prefix over the bands (cnt[b] becomes the band's first record)
        int acc = 0;
        for (int b = 0; b <= nb; ++b) { const int c = b < nb ? cnt[b] : 0; cnt[b] = acc; acc += c; }
        nside = 0;  // refilled by the fill pass
      }
      __syncthreads();
    }
  }
  __threadfence_block();
  __syncthreads();
  const int ms = maxspan, ns = nside;
  float* img = out + static_cast<size_t>(blockIdx.x) * W * H;
  unsigned char* frame = rgb ? rgb + static_cast<size_t>(blockIdx.x) * W * H * 3 : nullptr;
  const float x0 = (0.5f - 0.5f * W) / f, x1 = (W - 1.0f + 0.5f - 0.5f * W) / f;
  for (int b = 0; b < nb; ++b) {
    const int rb = b * kBandH, re = min(H, rb + kBandH);
    const int npx = (re - rb) * W;
    for (int i = tid; i < npx; i += 256) band[i] = ~0ull;
    __syncthreads();
    // 3a. triangles overlapping the band: band-sorted records of bands b - maxspan .. b, then the side list
    const int lo = cnt[max(0, b - ms)], hi = cnt[b + 1];
    const int nwork = hi - lo + ns;
    for (int w = tid; w < nwork; w += 256) {
      const unsigned long long rec = w < hi - lo ? list[lo + w] : list[npair - ns + (w - (hi - lo))];
      const int r0 = static_cast<int>((rec >> 46) & 0x3ff), dr = static_cast<int>(rec >> 56);
      const int r1 = dr == 255 ? H - 1 : r0 + dr;
      const int ra = max(r0, rb), rz = min(r1, re - 1);
      if (ra > rz) continue;
      const int c0 = static_cast<int>((rec >> 24) & 0x7ff), c1 = c0 + static_cast<int>((rec >> 35) & 0x7ff);
      const int kf = static_cast<int>(rec & 0xffffff), k = kf >> kRasterFaceBits, fi = kf & ((1 << kRasterFaceBits) - 1);
      const int g = mg[k];
      const DepthGeom& o = G[g];
      const TriLoad tr = load_tri(mesh.tri + 9 * mesh.faceadr[o.dataid], fi);
      const float lp[3] = {o.lp[0], o.lp[1], o.lp[2]};
      float A[9];
      for (int i = 0; i < 9; ++i) A[i] = o.A[i];
      const unsigned low = (static_cast<unsigned>(g) << 24) | static_cast<unsigned>(fi);
      for (int r = ra; r <= rz; ++r) {
        const float dy = (0.5f * H - r - 0.5f) / f;
        for (int c = c0; c <= c1; ++c) {
          const float dx = (c + 0.5f - 0.5f * W) / f;
          float lv[3];
        pixel_ray(A, dx, dy, lv);
          const float t = ray_tri_v(tr.a, tr.e1, tr.e2, lp, lv);
          if (t >= znear)
            atomicMin(&band[(r - rb) * W + c], (static_cast<unsigned long long>(__float_as_uint(t)) << 32) | low);
        }
      }
    }
    // 3b. primitive geoms of the band (pyramid cull as depth_kernel_v2's tile), then every pixel
    const float y1 = (0.5f * H - rb - 0.5f) / f, y0 = (0.5f * H - (re - 1) - 0.5f) / f;
    bool keep = false;
    if (lane < ngeom && G[lane].vis && G[lane].type != MRS_GEOM_MESH) {
      const DepthGeom& o = G[lane];
      if (o.type == MRS_GEOM_PLANE) {
        const float n[3] = {o.A[6], o.A[7], o.A[8]};
        const float bx = fminf(x0 * n[0], x1 * n[0]), by = fminf(y0 * n[1], y1 * n[1]);
        keep = bx + by - n[2] < 1e-6f;
      } else {
        auto outside = [&](float nx, float ny, float nz) {
          const float c = nx * o.cc[0] + ny * o.cc[1] + nz * o.cc[2];
          float r = 0;
          for (int i = 0; i < 3; ++i) r += o.ext[i] * fabsf(nx * o.A[3 * i] + ny * o.A[3 * i + 1] + nz * o.A[3 * i + 2]);
          return c + r < -1e-5f * (fabsf(c) + r);
        };
        keep = !(outside(1, 0, x0) || outside(-1, 0, -x1) || outside(0, 1, y0) || outside(0, -1, -y1));
      }
    }
    const unsigned long long prim = __ballot(keep);
    __syncthreads();
    for (int i = tid; i < npx; i += 256) {
      const int r = rb + i / W, c = i % W;
      const float dx = (c + 0.5f - 0.5f * W) / f, dy = (0.5f * H - r - 0.5f) / f;
      float best = -1;
      int bestg = 0;
      unsigned long long cand = prim;
      while (cand) {
        const int g = __builtin_ctzll(cand);
        cand &= cand - 1;
        const DepthGeom& o = G[g];
        const float lp[3] = {o.lp[0], o.lp[1], o.lp[2]}, sz[3] = {o.size[0], o.size[1], o.size[2]};
        float lv[3];
        pixel_ray(o.A, dx, dy, lv);
        const float t = o.type == MRS_GEOM_BOX ? ray_box_slab(sz, lp, lv) : ray_prim(o.type, sz, lp, lv);
        if (t >= znear && (best < 0 || t < best)) { best = t; bestg = g; }
      }
      const unsigned long long key = band[i];
      int tri = -1;
      if (key != ~0ull) {
        const float tm = __uint_as_float(static_cast<unsigned>(key >> 32));
        const int gm = static_cast<int>((key >> 24) & 0x3f);
        if (best < 0 || tm < best || (tm == best && gm < bestg)) {
          best = tm; bestg = gm; tri = static_cast<int>(key & 0xffffff);
        }
      }
      img[static_cast<size_t>(r) * W + c] = (best < 0 || best > zfar) ? zfar : best;
      if constexpr (kRGB) {
        unsigned char* px = frame + (static_cast<size_t>(r) * W + c) * 3;
        if (best < 0 || best > zfar) { lit_sky(LF, dx, dy, px); continue; }
        const DepthGeom& o = G[bestg];
        float lv[3], q[3];
        pixel_ray(o.A, dx, dy, lv);
        for (int k = 0; k < 3; ++k) q[k] = o.lp[k] + best * lv[k];
        float nl[3], nc[3];
        if (tri >= 0) {
          mesh_tri_normal(mesh.vert + 3 * mesh.vertadr[o.dataid], mesh.face + 3 * mesh.faceadr[o.dataid], tri, lv, nl);
        } else {
          local_normal(o.type, o.size, q, nl);
        }
        for (int j = 0; j < 3; ++j) nc[j] = nl[0] * o.A[j] + nl[1] * o.A[3 + j] + nl[2] * o.A[6 + j];
        lit_pixel(LF, lr, bestg, o.rgba, o.type, o.size, q, dx, dy, best, nc,
                  [&](const float* so, const float* sl, float sd) { return occluded_staged(G, ngeom, mesh, so, sl, sd); },
                  px);
      }
    }
    __syncthreads();
  }
}

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

}  // namespace

// ------------------------------------------------------------------ Batch implementation
struct BatchImpl {
  const Model* model = nullptr;
  int n = 0, device = 0;
  int group = 64;  // lanes per environment in the step kernel (64/group envs per wavefront)
  int g16_one_wg = 0;  // G = 16 with one workgroup per CU (tables past the two-per-CU budget)
  int wpb16 = WavesPerBlock<16>::value;  // waves per workgroup of the G = 16 kernels (DevState::wpb16)
  int helpers = 0;  // helper waves (DevState::ray_helpers), decided with the layout (build_devmodel)
  DevModel dm{};
  DevModel* d_dm = nullptr;  // device copy of dm
  LdsLayout& L = dm.L;
  ScratchLayout& S = dm.S;
  DevState st{};
  // a caller's device buffer [n][nu] the step launches read ctrl from (batch_bind_ctrl_device; null:
  // st.ctrl, the batch's own buffer)
  const float* ctrl_bound = nullptr;
  // the model's start states (start_rows.h): batch_reset copies a row of them from here, and tab_* is
  // their upload, which the masked reset (reset_masked_kernel) reads, next to the runtime pool [pool_n]
  // of batch_set_start_states (capacity pool_cap rows)
  StartRows start;
  // the envs' mass / inertia / armature as the caller wrote them, fp64 [n][4 nbody + nv] (empty until the
  // first set_inertial): what a later set of one quantity re-derives the others from, and get_inertial reads
  std::vector<double> inr_host;
  float *tab_qpos = nullptr, *tab_qvel = nullptr, *tab_ctrl = nullptr, *tab_act = nullptr;
  float *tab_mpos = nullptr, *tab_mquat = nullptr;  // the mocap poses' rows (row 0: the bodies' pos / quat)
  double* tab_time = nullptr;
  float *pool_qpos = nullptr, *pool_qvel = nullptr;
  int pool_n = 0, pool_cap = 0;
  // device staging of batch_reset_masked's host mask and keys ([n] each, made on first use)
  unsigned char* mask_stage = nullptr;
  int* key_stage = nullptr;
  void* dblock_f = nullptr;
  void* dblock_i = nullptr;
  std::vector<void*> allocs;
  hipStream_t own_stream = nullptr, stream = nullptr;
  hipEvent_t ev0[2] = {nullptr, nullptr}, ev1[2] = {nullptr, nullptr};
  bool ev_valid[2] = {false, false};
  // launches bracketed by the batch's own HIP events for batch_last_kernel_ms: bit 0 step launches, bit 1
  // frames (batch_set_timing).  A timed step launch costs ~10 us (C3: 0.420 vs 0.410 ms per 10-step
  // launch), so step launches are timed only on request
  int timing = 2;
  std::vector<float> staging;
  std::vector<int> pair_g1, pair_g2;  // host copy of the static collision pairs (contact export)
  std::vector<int> pair_dim;          // their condim and sliding friction (batch_get_contact_forces)
  std::vector<float> pair_mu;
  int dyn_asked = 0;  // the dynamics outputs asked for so far (1 << MRS_DYNOUT_*; ensure_dyn, batch_set_jac_sites)
  // camera pipeline (batch_render_async): pose snapshot + side stream, as the reference's rendering
  // thread renders its mjv_copyData snapshot while PhysicsLoop steps on (src/mujoco_cameras.cpp:204-215)
  hipStream_t rstream = nullptr;
  hipEvent_t snap_ev = nullptr, rend_ev = nullptr;
  bool rend_pending = false;
  float *snap_gpos = nullptr, *snap_gmat = nullptr, *snap_cpos = nullptr, *snap_cmat = nullptr;
  // depth_kernel_mesh: per-frame lists of (triangle, pixel box) records, sized for rast_frames frames
  unsigned long long* rast_list = nullptr;
  int rast_frames = 0;
  int max_lds = 0;  // hipDeviceAttributeMaxSharedMemoryPerBlock of the batch's device
  // ray queries (batch_ray): the uploaded geom lists of the filter triples seen so far, oldest first
  struct RayList { unsigned group_mask; bool no_static; int bodyexclude; RayGeom* d; int count; bool mesh; };
  std::deque<RayList> ray_lists;
  // the model needs the extended step kernels (step.hip MRS_EXT): general convex (MPR) collision
  // pairs, or rangefinders with more than 32 ray geoms
  bool ext = false;
};

namespace {

void* dalloc(BatchImpl& b, size_t bytes) {
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
  HIP_CHECK(hipMemsetAsync(p, 0, bytes ? bytes : 16, b.stream));
  b.allocs.push_back(p);
  return p;
}

static_assert(kRlitHead == kLitHead && kRlitLight == kLitLight && kRlitMat == kLitMat && kRlitTex == kLitTex &&
                  kRlitMaxLights == kLitMaxLights && kRastMaxGeoms == kDepthGeoms,
              "devtables.h restates lit.h's block layout and the frame kernels' geom limit");

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
void check_env_range(const BatchImpl& b, int env0, int n) {
  if (env0 < 0 || n < 0 || env0 + n > b.n) throw std::invalid_argument("env range out of bounds");
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
  b.dm.rf_static = b.dm.rf_mode ? static_cast<float*>(dalloc(b, std::max(1, b.dm.nrf) * sizeof(float))) : nullptr;
  b.group = p.group; b.g16_one_wg = p.g16_one_wg; b.wpb16 = p.wpb16; b.helpers = p.helpers; b.ext = p.ext;
  b.pair_g1 = T.pair_g1; b.pair_g2 = T.pair_g2; b.pair_dim = T.pair_dim; b.pair_mu = T.pair_mu;
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
      HIP_CHECK(launch_step(d_prod, b->L.total, b->dm.shr_total, b->st, 1, 1, true, b->group, false, b->ext, false, false, b->stream));
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
#ifdef MRS_DEPTH_STATS
  {
    unsigned long long h[4] = {};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_depth_stats), sizeof h) == hipSuccess && h[0])
      fprintf(stderr, "depth stats: tiles %llu, candidate visits %llu (%.2f per tile), winning visits %llu (%.1f %%)\n",
              h[0], h[1], static_cast<double>(h[1]) / h[0], h[2], 100.0 * h[2] / std::max(1ull, h[1]));
  }
#endif
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->rstream) (void)hipStreamSynchronize(b->rstream);
  for (void* p : b->allocs) (void)hipFree(p);
  if (b->pool_qpos) (void)hipFree(b->pool_qpos);
  if (b->pool_qvel) (void)hipFree(b->pool_qvel);
  if (b->rast_list) (void)hipFree(b->rast_list);
  for (const BatchImpl::RayList& l : b->ray_lists) (void)hipFree(l.d);
  if (b->snap_ev) (void)hipEventDestroy(b->snap_ev);
  if (b->rend_ev) (void)hipEventDestroy(b->rend_ev);
  if (b->rstream) (void)hipStreamDestroy(b->rstream);
  for (int k = 0; k < 2; ++k) {
    if (b->ev0[k]) (void)hipEventDestroy(b->ev0[k]);
    if (b->ev1[k]) (void)hipEventDestroy(b->ev1[k]);
  }
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
}

int batch_num_envs(const BatchImpl* b) { return b->n; }

int batch_layout(const BatchImpl* b, int* out, int n) {
  int v[19];
  plan_layout_values(b->dm, b->group, b->g16_one_wg, b->wpb16, b->helpers, v);  // (the first 16: plan.h)
  v[16] = b->dm.cfrc_contact ? 1 : 0;
  v[17] = b->dm.dyn_mask;
  v[18] = b->dm.solve_fuse;
  int k = 0;
  for (; k < n && k < 19; ++k) out[k] = v[k];
  return k;
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
  HIP_CHECK(launch_step(b->d_dm, b->L.total, b->dm.shr_total, st, b->n, n_steps, forward_only, b->group,
                        b->model->solver != MRS_SOL_PGS, b->ext, b->dm.prm_mask != 0, b->dm.dyn_mask != 0, b->stream));
  if (timed) HIP_CHECK(hipEventRecord(b->ev1[0], b->stream));
  b->ev_valid[0] = timed;
}

namespace {
struct Poses { const float *gpos, *gmat, *cpos, *cmat; };

void check_render_args(const BatchImpl* b, int cam, int env0, int n) {
  const Model& m = *b->model;
  if (cam < 0 || cam >= m.ncam) throw std::invalid_argument("camera index out of range");
  if (env0 < 0 || n < 1 || env0 + n > b->n) throw std::invalid_argument("env range out of bounds");
  if (m.ngeom > kMaxRenderGeoms) throw UnsupportedError("too many geoms for the depth kernel");
}

// depth (+ colour) kernel launch on `stream` from the given geom / camera poses, bracketed by the
// batch's render timing events
void render_launch(BatchImpl* b, int cam, int env0, int n, float* dout, unsigned char* drgb, const Poses& ps,
                   hipStream_t stream) {
  const Model& m = *b->model;
  const int W = m.cam_resolution[2 * cam], H = m.cam_resolution[2 * cam + 1];
  const float f = static_cast<float>(0.5 * H / std::tan(m.cam_fovy[cam] * M_PI / 360.0));
  const float znear = static_cast<float>(m.vis_znear * m.stat_extent), zfar = static_cast<float>(m.vis_zfar * m.stat_extent);
  const DevModel& d = b->dm;
  const MeshRef mesh{d.mesh_vert.p, d.mesh_face.p, d.geom_dataid.p, d.mesh_vertadr.p, d.mesh_faceadr.p,
                     d.mesh_facenum.p, d.mesh_bvh.p, d.mesh_bvhadr.p, d.mesh_bvhnum.p, d.mesh_tri.p};
  const LitRef lr{d.rlit.p, d.geom_matid.p, d.lit_nlight, d.lit_mat0, d.lit_tex0, d.lit_sky};
  // the binned kernel needs its band of W x kBandH 64-bit keys in LDS (within the device's per-block
  // limit) and a per-frame triangle list in global memory: frames go in chunks whose lists fit a
  // budget (MRS_RAST_BUDGET_MB, default 2048 MB), so a large mesh over many envs renders in several
  // launches instead of failing the allocation
  const size_t band_lds = static_cast<size_t>(W) * kBandH * sizeof(unsigned long long);
  if (b->max_lds == 0) {
    int v = 0;
    HIP_CHECK(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, b->device));
    b->max_lds = v > 0 ? v : 65536;
  }
  const bool raster = d.nrast > 0 && W <= 2048 && H <= kBandH * kMaxBands && band_lds <= static_cast<size_t>(b->max_lds) &&
                     !std::getenv("MRS_DEPTH_V2") && !std::getenv("MRS_DEPTH_V1");
  const size_t per_frame = static_cast<size_t>(std::max(d.nrast_pair, 1)) * sizeof(unsigned long long);
  const char* bud = std::getenv("MRS_RAST_BUDGET_MB");
  const size_t budget = (bud ? static_cast<size_t>(std::max(1L, std::atol(bud))) : 2048) << 20;
  const int chunk = static_cast<int>(std::max<size_t>(1, std::min<size_t>(n, budget / per_frame)));
  if (raster && b->rast_frames < chunk) {
    // (one render at a time per batch: the lists are reused by every later frame batch)
    if (b->rast_list) {
      HIP_CHECK(hipStreamSynchronize(b->stream));
      if (b->rstream) HIP_CHECK(hipStreamSynchronize(b->rstream));
      HIP_CHECK(hipFree(b->rast_list));
    }
    HIP_CHECK(hipMalloc(&b->rast_list, static_cast<size_t>(chunk) * per_frame));
    b->rast_frames = chunk;
  }
  const bool timed = (b->timing & 2) != 0;
  if (timed) HIP_CHECK(hipEventRecord(b->ev0[1], stream));
  if (raster) {
    for (int c0 = 0; c0 < n; c0 += chunk) {
      const int nc = std::min(chunk, n - c0);
      const size_t px = static_cast<size_t>(c0) * W * H;
      hipLaunchKernelGGL(drgb ? depth_kernel_mesh<true> : depth_kernel_mesh<false>, dim3(nc), dim3(256), band_lds,
                         stream, d.geom_type.p, d.geom_group.p,
                         d.geom_size.p, d.geom_rgba.p, m.ngeom, ps.gpos, ps.gmat, ps.cpos, ps.cmat, m.ncam, cam,
                         env0 + c0, W, H, f, znear, zfar, dout + px, drgb ? drgb + 3 * px : nullptr, mesh,
                         d.rast_geom.p, d.rast_base.p, d.nrast, d.nrast_pair, b->rast_list, lr);
    }
  } else if (m.ngeom <= kDepthGeoms && !std::getenv("MRS_DEPTH_V1")) {
    const bool has_mesh = d.nrast > 0 || std::any_of(m.geom_type.begin(), m.geom_type.end(),
                                                      [](int t) { return t == MRS_GEOM_MESH; });
    auto kern = has_mesh ? (drgb ? depth_kernel_v2<true, true> : depth_kernel_v2<false, true>)
                         : (drgb ? depth_kernel_v2<true, false> : depth_kernel_v2<false, false>);
    hipLaunchKernelGGL(kern, dim3(n), dim3(256), 0, stream,
                       d.geom_type.p, d.geom_group.p, d.geom_size.p,
                       d.geom_rgba.p, m.ngeom, ps.gpos, ps.gmat, ps.cpos, ps.cmat, m.ncam,
                       cam, env0, W, H, f, znear, zfar, dout, drgb, mesh, lr);
  } else {
    dim3 grid(((W + 15) / 16) * ((H + 15) / 16), n);
    hipLaunchKernelGGL(drgb ? depth_kernel<true> : depth_kernel<false>, grid, dim3(256), 0, stream, d.geom_type.p,
                       d.geom_group.p, d.geom_size.p, d.geom_rbound.p,
                       d.geom_rgba.p, m.ngeom, ps.gpos, ps.gmat, ps.cpos, ps.cmat, m.ncam,
                       cam, env0, W, H, f, znear, zfar, dout, drgb, mesh, lr);
  }
  HIP_CHECK(hipGetLastError());
  if (timed) HIP_CHECK(hipEventRecord(b->ev1[1], stream));
  b->ev_valid[1] = timed;
}
}  // namespace

void batch_render_depth(BatchImpl* b, int cam, int env0, int n, float* out, bool device_out, unsigned char* rgb_out) {
  check_render_args(b, cam, env0, n);
  const Model& m = *b->model;
  HIP_CHECK(hipSetDevice(b->device));
  const int W = m.cam_resolution[2 * cam], H = m.cam_resolution[2 * cam + 1];
  const size_t bytes = static_cast<size_t>(n) * W * H * sizeof(float);
  const size_t rgb_bytes = rgb_out ? static_cast<size_t>(n) * W * H * 3 : 0;
  float* dout = out;
  unsigned char* drgb = rgb_out;
  void* tmp = nullptr;
  if (!device_out) {
    HIP_CHECK(hipMallocAsync(&tmp, bytes + rgb_bytes, b->stream));
    dout = static_cast<float*>(tmp);
    if (rgb_out) drgb = static_cast<unsigned char*>(tmp) + bytes;
  }
  if (b->rend_pending) HIP_CHECK(hipStreamWaitEvent(b->stream, b->rend_ev, 0));  // one render at a time
  render_launch(b, cam, env0, n, dout, drgb, Poses{b->st.geom_xpos, b->st.geom_xmat, b->st.cam_xpos, b->st.cam_xmat},
                b->stream);
  if (!device_out) {
    HIP_CHECK(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, b->stream));
    if (rgb_out) HIP_CHECK(hipMemcpyAsync(rgb_out, drgb, rgb_bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_CHECK(hipFreeAsync(tmp, b->stream));
    HIP_CHECK(hipStreamSynchronize(b->stream));
  }
}

// Camera pipeline: the poses of the last step are copied into a snapshot on the batch stream (so the
// copy is ordered after that step and before the next), then the frame is rendered from the snapshot
// on the batch's render stream while later steps run on the batch stream.  A new snapshot waits for
// the previous asynchronous render to finish reading the old one.  batch_render_wait orders the
// batch stream after the last render (frames complete for anything queued later).
void batch_render_async(BatchImpl* b, int cam, int env0, int n, float* d_out, unsigned char* d_rgb) {
  check_render_args(b, cam, env0, n);
  const Model& m = *b->model;
  HIP_CHECK(hipSetDevice(b->device));
  const size_t ng = static_cast<size_t>(b->n) * std::max(1, m.ngeom), nc = static_cast<size_t>(b->n) * std::max(1, m.ncam);
  if (!b->rstream) {
    HIP_CHECK(hipStreamCreateWithFlags(&b->rstream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&b->snap_ev, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&b->rend_ev, hipEventDisableTiming));
    b->snap_gpos = static_cast<float*>(dalloc(*b, ng * 3 * sizeof(float)));
    b->snap_gmat = static_cast<float*>(dalloc(*b, ng * 9 * sizeof(float)));
    b->snap_cpos = static_cast<float*>(dalloc(*b, nc * 3 * sizeof(float)));
    b->snap_cmat = static_cast<float*>(dalloc(*b, nc * 9 * sizeof(float)));
  }
  if (b->rend_pending) HIP_CHECK(hipStreamWaitEvent(b->stream, b->rend_ev, 0));
  HIP_CHECK(hipMemcpyAsync(b->snap_gpos, b->st.geom_xpos, ng * 3 * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
  HIP_CHECK(hipMemcpyAsync(b->snap_gmat, b->st.geom_xmat, ng * 9 * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
  HIP_CHECK(hipMemcpyAsync(b->snap_cpos, b->st.cam_xpos, nc * 3 * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
  HIP_CHECK(hipMemcpyAsync(b->snap_cmat, b->st.cam_xmat, nc * 9 * sizeof(float), hipMemcpyDeviceToDevice, b->stream));
  HIP_CHECK(hipEventRecord(b->snap_ev, b->stream));
  HIP_CHECK(hipStreamWaitEvent(b->rstream, b->snap_ev, 0));
  render_launch(b, cam, env0, n, d_out, d_rgb, Poses{b->snap_gpos, b->snap_gmat, b->snap_cpos, b->snap_cmat}, b->rstream);
  HIP_CHECK(hipEventRecord(b->rend_ev, b->rstream));
  b->rend_pending = true;
}

void batch_render_wait(BatchImpl* b) {
  HIP_CHECK(hipSetDevice(b->device));
  if (b->rend_pending) HIP_CHECK(hipStreamWaitEvent(b->stream, b->rend_ev, 0));
}

// ---- ray queries (mrs_batch_ray / mrs_batch_ray_device; kernel: rayquery.h, geom lists: rayfilter.h)
namespace {
constexpr size_t kRayListCache = 8;

// the device list of a filter triple: uploaded on first use and kept, the oldest of kRayListCache dropped
// for a new one (after the queued queries that may read it have run)
const BatchImpl::RayList& ray_list(BatchImpl* b, unsigned group_mask, bool no_static, int bodyexclude) {
  for (const BatchImpl::RayList& l : b->ray_lists)
    if (l.group_mask == group_mask && l.no_static == no_static && l.bodyexclude == bodyexclude) return l;
  const std::vector<RayGeom> host = build_ray_filter(*b->model, group_mask, no_static, bodyexclude);
  if (b->ray_lists.size() >= kRayListCache) {
    HIP_CHECK(hipStreamSynchronize(b->stream));
    HIP_CHECK(hipFree(b->ray_lists.front().d));
    b->ray_lists.pop_front();
  }
  BatchImpl::RayList l{group_mask, no_static, bodyexclude, nullptr, static_cast<int>(host.size()),
                       std::any_of(host.begin(), host.end(), [](const RayGeom& g) { return g.type == MRS_GEOM_MESH; })};
  HIP_CHECK(hipMalloc(&l.d, std::max<size_t>(1, host.size()) * sizeof(RayGeom)));
  try {
    if (!host.empty()) {
      HIP_CHECK(hipMemcpyAsync(l.d, host.data(), host.size() * sizeof(RayGeom), hipMemcpyHostToDevice, b->stream));
      HIP_CHECK(hipStreamSynchronize(b->stream));  // (the host list is read by then)
    }
  } catch (...) {  // (a list that was never filled is not kept)
    (void)hipFree(l.d);
    throw;
  }
  b->ray_lists.push_back(l);
  return b->ray_lists.back();
}

// every argument of a query that the host can check, before any launch
void check_ray_args(const BatchImpl* b, int n_rays, int flags, int frame_type, int frame_id, int bodyexclude,
                    int env0, int n) {
  const Model& m = *b->model;
  if (n_rays < 0) throw std::invalid_argument("negative number of rays");
  check_ray_filter(m, flags, bodyexclude);
  if (frame_type != MRS_RAY_FRAME_WORLD && frame_type != MRS_RAY_FRAME_GEOM && frame_type != MRS_RAY_FRAME_CAMERA)
    throw std::invalid_argument("unknown ray frame type");
  if (frame_type == MRS_RAY_FRAME_GEOM && (frame_id < 0 || frame_id >= m.ngeom))
    throw std::invalid_argument("ray frame geom out of range");
  if (frame_type == MRS_RAY_FRAME_CAMERA && (frame_id < 0 || frame_id >= m.ncam))
    throw std::invalid_argument("ray frame camera out of range");
  check_env_range(*b, env0, n);
}

// the launch for envs [env0, env0 + n): device rays and outputs, rows of env0 first; arguments checked
void ray_launch(BatchImpl* b, const float* d_pnt, const float* d_vec, int n_rays, int flags, int frame_type,
                int frame_id, unsigned group_mask, int bodyexclude, float* d_dist, int* d_geomid, int env0, int n) {
  const Model& m = *b->model;
  const BatchImpl::RayList& l = ray_list(b, group_mask, (flags & MRS_RAY_NO_STATIC) != 0, bodyexclude);
  RayQueryArgs a{};
  a.list = l.d; a.nkeep = l.count; a.ngeom = m.ngeom;
  a.geom_xpos = b->st.geom_xpos; a.geom_xmat = b->st.geom_xmat;
  if (frame_type == MRS_RAY_FRAME_GEOM) {
    a.frame_pos = b->st.geom_xpos + 3 * static_cast<size_t>(frame_id);
    a.frame_mat = b->st.geom_xmat + 9 * static_cast<size_t>(frame_id);
    a.frame_stride = m.ngeom;
  } else if (frame_type == MRS_RAY_FRAME_CAMERA) {
    a.frame_pos = b->st.cam_xpos + 3 * static_cast<size_t>(frame_id);
    a.frame_mat = b->st.cam_xmat + 9 * static_cast<size_t>(frame_id);
    a.frame_stride = m.ncam;
  }
  a.n_rays = n_rays; a.shared = (flags & MRS_RAY_SHARED) != 0;
  const DevModel& d = b->dm;
  const MeshRef mesh{d.mesh_vert.p, d.mesh_face.p, d.geom_dataid.p, d.mesh_vertadr.p, d.mesh_faceadr.p,
                     d.mesh_facenum.p, d.mesh_bvh.p, d.mesh_bvhadr.p, d.mesh_bvhnum.p, d.mesh_tri.p};
  const unsigned tiles = static_cast<unsigned>((n_rays + 255) / 256);
  constexpr int kMaxGridY = 65535;
  for (int r0 = 0; r0 < n; r0 += kMaxGridY) {  // (the grid's y extent is 16 bits)
    const int nr = std::min(kMaxGridY, n - r0);
    const size_t rows = static_cast<size_t>(r0) * n_rays;
    a.env0 = env0 + r0;
    a.pnt = d_pnt + (a.shared ? 0 : rows * 3);
    a.vec = d_vec + (a.shared ? 0 : rows * 3);
    a.dist = d_dist + rows;
    a.geomid = d_geomid ? d_geomid + rows : nullptr;
    hipLaunchKernelGGL(l.mesh ? ray_query_kernel<true> : ray_query_kernel<false>, dim3(tiles, nr), dim3(256), 0,
                       b->stream, a, mesh);
  }
  HIP_CHECK(hipGetLastError());
}
}  // namespace

void batch_ray_device(BatchImpl* b, const float* d_pnt, const float* d_vec, int n_rays, int flags, int frame_type,
                      int frame_id, unsigned group_mask, int bodyexclude, float* d_dist, int* d_geomid) {
  check_ray_args(b, n_rays, flags, frame_type, frame_id, bodyexclude, 0, b->n);
  if (n_rays == 0) return;
  if (!d_pnt || !d_vec || !d_dist) throw std::invalid_argument("null ray or distance buffer");
  HIP_CHECK(hipSetDevice(b->device));
  ray_launch(b, d_pnt, d_vec, n_rays, flags, frame_type, frame_id, group_mask, bodyexclude, d_dist, d_geomid, 0, b->n);
}

void batch_ray(BatchImpl* b, const double* pnt, const double* vec, int n_rays, int flags, int frame_type, int frame_id,
               unsigned group_mask, int bodyexclude, double* dist, int* geomid, int env0, int n) {
  check_ray_args(b, n_rays, flags, frame_type, frame_id, bodyexclude, env0, n);
  if (n_rays == 0 || n == 0) return;
  if (!pnt || !vec || !dist) throw std::invalid_argument("null ray or distance buffer");
  HIP_CHECK(hipSetDevice(b->device));
  // rays through fp32 as rows_to_device converts, distances back as rows_to_host does
  const size_t nin = static_cast<size_t>((flags & MRS_RAY_SHARED) ? 1 : n) * n_rays * 3;
  const size_t nout = static_cast<size_t>(n) * n_rays;
  std::vector<float> in(2 * nin), out(nout);
  for (size_t k = 0; k < nin; ++k) { in[k] = static_cast<float>(pnt[k]); in[nin + k] = static_cast<float>(vec[k]); }
  void* tmp = nullptr;
  HIP_CHECK(hipMallocAsync(&tmp, (2 * nin + 2 * nout) * sizeof(float), b->stream));
  float* d_in = static_cast<float*>(tmp);
  float* d_dist = d_in + 2 * nin;
  int* d_geomid = geomid ? reinterpret_cast<int*>(d_dist + nout) : nullptr;
  try {
    HIP_CHECK(hipMemcpyAsync(d_in, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
    ray_launch(b, d_in, d_in + nin, n_rays, flags, frame_type, frame_id, group_mask, bodyexclude, d_dist, d_geomid, env0, n);
    HIP_CHECK(hipMemcpyAsync(out.data(), d_dist, nout * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    if (geomid) HIP_CHECK(hipMemcpyAsync(geomid, d_geomid, nout * sizeof(int), hipMemcpyDeviceToHost, b->stream));
  } catch (...) {
    (void)hipFreeAsync(tmp, b->stream);
    throw;
  }
  HIP_CHECK(hipFreeAsync(tmp, b->stream));
  HIP_CHECK(hipStreamSynchronize(b->stream));
  for (size_t k = 0; k < nout; ++k) dist[k] = out[k];
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
