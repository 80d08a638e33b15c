// Analytic ray primitives in the geom frame, of the step kernel's rangefinders and touch sensors
// (step.hip): mju_rayGeom of engine_ray restated -- plane, sphere, capsule, ellipsoid, cylinder, and the
// box in slab form.  Returns the nearest t >= 0, or -1.  (render.hip's ray_prim repeats the first five
// cases: taking them from here changed its kernels' registers)
#pragma once
#include <hip/hip_runtime.h>

#include "devmodel.h"
#include "step/base.h"
#include "step/math.h"

namespace mrs {
namespace {

__device__ __forceinline__ float ray_quad(float a, float b, float c, float x[2]) {
  float det = b * b - a * c;
  if (det < kMinVal) { x[0] = x[1] = -1; return -1; }
  det = sqrtf(det);
  float ia = 1.0f / a;
  x[0] = (-b - det) * ia;
  x[1] = (-b + det) * ia;
  if (x[0] >= 0) return x[0];
  if (x[1] >= 0) return x[1];
  return -1;
}
template <class PS>
__device__ float ray_geom_local(int type, const PS s, const float lp[3], const float lv[3]) {
  float x[2];
  switch (type) {
    case MRS_GEOM_PLANE: {
      // parallel (within 1e-6 rad) or facing away: miss (fp32-safe form of MuJoCo's lv[2] > -mjMINVAL)
      if (lv[2] >= 0 || lv[2] * lv[2] <= 1e-12f * dot3(lv, lv)) return -1;
      float t = -lp[2] / lv[2];
      if (t < 0) return -1;
      float p0 = lp[0] + t * lv[0], p1 = lp[1] + t * lv[1];
      if ((s[0] <= 0 || fabsf(p0) <= s[0]) && (s[1] <= 0 || fabsf(p1) <= s[1])) return t;
      return -1;
    }
    case MRS_GEOM_SPHERE:
      return ray_quad(dot3(lv, lv), dot3(lv, lp), dot3(lp, lp) - s[0] * s[0], x);
    case MRS_GEOM_CAPSULE: {
      float best = -1;
      float a = lv[0] * lv[0] + lv[1] * lv[1];
      if (a > kMinVal) {
        float b = lv[0] * lp[0] + lv[1] * lp[1], c = lp[0] * lp[0] + lp[1] * lp[1] - s[0] * s[0];
        ray_quad(a, b, c, x);
        for (int i = 0; i < 2; ++i)
          if (x[i] >= 0 && fabsf(lp[2] + x[i] * lv[2]) <= s[1] && (best < 0 || x[i] < best)) best = x[i];
      }
      float vv = dot3(lv, lv);
      for (int e = -1; e <= 1; e += 2) {
        float q[3] = {lp[0], lp[1], lp[2] - e * s[1]};
        ray_quad(vv, dot3(lv, q), dot3(q, q) - s[0] * s[0], x);
        for (int i = 0; i < 2; ++i)
          if (x[i] >= 0 && e * (lp[2] + x[i] * lv[2] - e * s[1]) >= 0 && (best < 0 || x[i] < best)) best = x[i];
      }
      return best;
    }
    case MRS_GEOM_ELLIPSOID: {
      float q[3] = {lp[0] / s[0], lp[1] / s[1], lp[2] / s[2]}, v[3] = {lv[0] / s[0], lv[1] / s[1], lv[2] / s[2]};
      return ray_quad(dot3(v, v), dot3(v, q), dot3(q, q) - 1, x);
    }
    case MRS_GEOM_CYLINDER: {
      float best = -1;
      float a = lv[0] * lv[0] + lv[1] * lv[1];
      if (a > kMinVal) {
        float b = lv[0] * lp[0] + lv[1] * lp[1], c = lp[0] * lp[0] + lp[1] * lp[1] - s[0] * s[0];
        ray_quad(a, b, c, x);
        for (int i = 0; i < 2; ++i)
          if (x[i] >= 0 && fabsf(lp[2] + x[i] * lv[2]) <= s[1] && (best < 0 || x[i] < best)) best = x[i];
      }
      if (fabsf(lv[2]) > kMinVal)
        for (int e = -1; e <= 1; e += 2) {
          float t = (e * s[1] - lp[2]) / lv[2];
          if (t < 0) continue;
          float p0 = lp[0] + t * lv[0], p1 = lp[1] + t * lv[1];
          if (p0 * p0 + p1 * p1 <= s[0] * s[0] && (best < 0 || t < best)) best = t;
        }
      return best;
    }
    case MRS_GEOM_BOX: {
      // slab form of mj_rayBox's face test: the same face parameters (+-s - lp) / lv, nearest
      // non-negative crossing (entry from outside, exit from inside); measured C3 +5.7% over the
      // face-by-face loop (a ray grazing an edge may take the adjacent face's equal-t crossing)
      float tmin = -3.0e38f, tmax = 3.0e38f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float inv = __builtin_amdgcn_rcpf(lv[i]);
        const bool par = fabsf(lv[i]) <= kMinVal;
        const float t1 = (-s[i] - lp[i]) * inv, t2 = (s[i] - lp[i]) * inv;
        const bool inside = fabsf(lp[i]) <= s[i];
        tmin = fmaxf(tmin, par ? (inside ? -3.0e38f : 3.0e38f) : fminf(t1, t2));
        tmax = fminf(tmax, par ? (inside ? 3.0e38f : -3.0e38f) : fmaxf(t1, t2));
      }
      if (tmax < tmin || tmax < 0) return -1;
      return tmin >= 0 ? tmin : tmax;
    }
  }
  return -1;
}

}  // namespace
}  // namespace mrs
