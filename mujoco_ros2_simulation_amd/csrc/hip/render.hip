// Frames and ray queries of a batch: the three depth (+ colour) kernels, the ray-query kernel
// (rayquery.h) and their host side -- the frame launch by the plan of renderplan.h, the camera pipeline on
// the batch's render stream, and the ray queries' geom lists and launches.  Host side of the C ABI in
// include/mrs.h, next to batch.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/mrs.h"
#include "../mjcf/model.h"
#include "batch.h"
#include "batch_impl.h"
#include "devmodel.h"
#include "devtables.h"
#include "renderplan.h"
#include "raymesh.h"
#include "rayfilter.h"
#include "lit.h"

namespace mrs {

namespace {

// the model's meshes for the render kernels (mrs_model.h mesh arrays, device copies)
struct MeshRef {
  const float* vert;
  const int *face, *dataid, *vertadr, *faceadr, *facenum;
  const float* bvh;           // bounding volume hierarchies (8 floats per node, build_mesh_bvh)
  const int *bvhadr, *bvhnum;  // per mesh: first node, node count (0: no hierarchy, every triangle)
  const float* tri;            // pre-gathered triangle records (DevModel::mesh_tri)
  // raymesh.h ray_mesh against mesh `dataid` (a geom's dataid[g]) with the geom's half extents `size`
  __device__ __forceinline__ float ray(int dataid, const float* size, const float lp[3], const float lv[3],
                                       int* tri = nullptr) const {
    return ray_mesh(this->tri + 9 * faceadr[dataid], facenum[dataid], size, lp, lv, bvh + 8 * bvhadr[dataid],
                    bvhnum[dataid], tri);
  }
};
inline MeshRef mesh_ref(const DevModel& d) {
  return {d.mesh_vert.p, d.mesh_face.p, d.geom_dataid.p, d.mesh_vertadr.p, d.mesh_faceadr.p,
          d.mesh_facenum.p, d.mesh_bvh.p, d.mesh_bvhadr.p, d.mesh_bvhnum.p, d.mesh_tri.p};
}

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

// ------------------------------------------------------------------ depth camera kernel
// One thread per pixel, one env per blockIdx.y; the env's geom poses are staged in LDS.
// Eye-space depth: ray through the pixel centre with camera-frame direction (x, y, -1), so the ray
// parameter of the nearest hit is the eye-space z that OpenGL + the plugin's linearisation
// (src/mujoco_cameras.cpp:222-235) produce; rows in ROS order (flip of :229-240 applied).
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
      tt = mesh.ray(id, geom_size + 3 * g, lp, lv, &tri);
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
      mesh.ray(id, geom_size + 3 * bestg, lp, lv, &tri);
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
          // (MeshRef::ray spelled out: through this lambda the call compiles to the same instructions in
          // another order, and the kernels' code is kept as it was)
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
constexpr int kDepthTileW = 64, kDepthTileH = MRS_DEPTH_TILE_H, kDepthChunk = MRS_DEPTH_CHUNK;
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
      t = mesh.ray(h.dataid, h.size, lp, lv, &tri);
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
          t = mesh.ray(o.dataid, sz, lp, lv, &tri);
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
            mesh.ray(o.dataid, o.size, o.lp, lv, &tri);
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
constexpr int kMaxSpan = 4;  // (kBandH, kMaxBands: renderplan.h)
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

// ------------------------------------------------------------------ frames: host side
struct Poses { const float *gpos, *gmat, *cpos, *cmat; };

void check_render_args(const BatchImpl* b, int cam, int env0, int n) {
  const Model& m = *b->model;
  if (cam < 0 || cam >= m.ncam) throw std::invalid_argument("camera index out of range");
  if (env0 < 0 || n < 1 || env0 + n > b->n) throw std::invalid_argument("env range out of bounds");
  check_render_geoms(m.ngeom);
}

// the plan of n frames of camera `cam` (renderplan.h) from the model, the counts of its tables and the
// render switches as they are set now
RenderPlan plan_frames(const Model& m, const DevModel& d, int cam, int n, int max_lds) {
  // (a model with raster lists has mesh geoms: only one without them is scanned)
  const bool has_mesh_geom = d.nrast > 0 || std::any_of(m.geom_type.begin(), m.geom_type.end(),
                                                        [](int t) { return t == MRS_GEOM_MESH; });
  return choose_render(m.ngeom, has_mesh_geom, d.nrast, d.nrast_pair, m.cam_resolution[2 * cam],
                       m.cam_resolution[2 * cam + 1], n, max_lds, read_render_overrides());
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
  const MeshRef mesh = mesh_ref(d);
  const LitRef lr{d.rlit.p, d.geom_matid.p, d.lit_nlight, d.lit_mat0, d.lit_tex0, d.lit_sky};
  if (b->max_lds == 0) {
    int v = 0;
    HIP_CHECK(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, b->device));
    b->max_lds = v > 0 ? v : 65536;
  }
  const RenderPlan plan = plan_frames(m, d, cam, n, b->max_lds);
  if (plan.kind == RenderPlan::BINNED && b->rast_frames < plan.chunk) {
    // (one render at a time per batch: the lists are reused by every later frame batch)
    if (b->rast_list) {
      HIP_CHECK(hipStreamSynchronize(b->stream));
      if (b->rstream) HIP_CHECK(hipStreamSynchronize(b->rstream));
      HIP_CHECK(hipFree(b->rast_list));
    }
    HIP_CHECK(hipMalloc(&b->rast_list, static_cast<size_t>(plan.chunk) * plan.per_frame));
    b->rast_frames = plan.chunk;
  }
  const bool timed = (b->timing & 2) != 0;
  if (timed) HIP_CHECK(hipEventRecord(b->ev0[1], stream));
  switch (plan.kind) {
    case RenderPlan::BINNED:
      for (int c0 = 0; c0 < n; c0 += plan.chunk) {
        const int nc = std::min(plan.chunk, n - c0);
        const size_t px = static_cast<size_t>(c0) * W * H;
        hipLaunchKernelGGL(drgb ? depth_kernel_mesh<true> : depth_kernel_mesh<false>, dim3(nc), dim3(256), plan.band_lds,
                           stream, d.geom_type.p, d.geom_group.p,
                           d.geom_size.p, d.geom_rgba.p, m.ngeom, ps.gpos, ps.gmat, ps.cpos, ps.cmat, m.ncam, cam,
                           env0 + c0, W, H, f, znear, zfar, dout + px, drgb ? drgb + 3 * px : nullptr, mesh,
                           d.rast_geom.p, d.rast_base.p, d.nrast, d.nrast_pair, b->rast_list, lr);
      }
      break;
    case RenderPlan::FRAME: {
      auto kern = plan.mesh ? (drgb ? depth_kernel_v2<true, true> : depth_kernel_v2<false, true>)
                            : (drgb ? depth_kernel_v2<true, false> : depth_kernel_v2<false, false>);
      hipLaunchKernelGGL(kern, dim3(plan.grid_x), dim3(256), 0, stream,
                         d.geom_type.p, d.geom_group.p, d.geom_size.p,
                         d.geom_rgba.p, m.ngeom, ps.gpos, ps.gmat, ps.cpos, ps.cmat, m.ncam,
                         cam, env0, W, H, f, znear, zfar, dout, drgb, mesh, lr);
      break;
    }
    case RenderPlan::TILE:
      hipLaunchKernelGGL(drgb ? depth_kernel<true> : depth_kernel<false>, dim3(plan.grid_x, plan.grid_y), dim3(256), 0,
                         stream, d.geom_type.p,
                         d.geom_group.p, d.geom_size.p, d.geom_rbound.p,
                         d.geom_rgba.p, m.ngeom, ps.gpos, ps.gmat, ps.cpos, ps.cmat, m.ncam,
                         cam, env0, W, H, f, znear, zfar, dout, drgb, mesh, lr);
      break;
  }
  HIP_CHECK(hipGetLastError());
  if (timed) HIP_CHECK(hipEventRecord(b->ev1[1], stream));
  b->ev_valid[1] = timed;
}
}  // namespace

// mrs_debug_render_plan: the render switches, the model's raster counts and the plan; touches no device
int render_plan(const Model& m, int cam, int n_frames, int max_lds, long long* out, int n) {
  if (cam < 0 || cam >= m.ncam) throw std::invalid_argument("camera index out of range");
  DevModel d{};
  std::vector<int> rast_geom, rast_base;
  raster_lists(m, d, rast_geom, rast_base);
  const RenderPlan p = plan_frames(m, d, cam, n_frames, max_lds);
  const long long v[7] = {p.kind, p.mesh, static_cast<long long>(p.band_lds), p.chunk,
                          static_cast<long long>(p.per_frame), p.grid_x, p.grid_y};
  int k = 0;
  for (; k < n && k < 7; ++k) out[k] = v[k];
  return k;
}

// the render side of batch_free: the streams have drained
void render_free(BatchImpl& b) {
#ifdef MRS_DEPTH_STATS
  {
    unsigned long long h[4] = {};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_depth_stats), sizeof h) == hipSuccess && h[0])
      fprintf(stderr, "depth stats: tiles %llu, candidate visits %llu (%.2f per tile), winning visits %llu (%.1f %%)\n",
              h[0], h[1], static_cast<double>(h[1]) / h[0], h[2], 100.0 * h[2] / std::max(1ull, h[1]));
  }
#endif
  if (b.rast_list) (void)hipFree(b.rast_list);
  for (const BatchImpl::RayList& l : b.ray_lists) (void)hipFree(l.d);
  if (b.snap_ev) (void)hipEventDestroy(b.snap_ev);
  if (b.rend_ev) (void)hipEventDestroy(b.rend_ev);
  if (b.rstream) (void)hipStreamDestroy(b.rstream);
}

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
  const MeshRef mesh = mesh_ref(b->dm);
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

}  // namespace mrs
