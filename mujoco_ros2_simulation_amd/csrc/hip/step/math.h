// Step kernel: small fp32 vector, quaternion and spatial-algebra helpers (the mju_* functions the
// phases use: mju_mulQuat, mju_quat2Mat, mju_rotVecQuat, mju_crossMotion, mju_crossForce, ...), is_bad and clampf.
#pragma once
#include <hip/hip_runtime.h>

#include "base.h"

namespace mrs {
namespace {

__device__ __forceinline__ void quat_mul(float r[4], const float a[4], const float b[4]) {
  float t0 = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  float t1 = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  float t2 = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  float t3 = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = t0; r[1] = t1; r[2] = t2; r[3] = t3;
}
__device__ __forceinline__ void quat_normalize(float q[4]) {
  float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < kMinVal) { q[0] = 1; q[1] = q[2] = q[3] = 0; return; }
  float in = 1.0f / n;
  q[0] *= in; q[1] *= in; q[2] *= in; q[3] *= in;
}
__device__ __forceinline__ void quat2mat(float m[9], const float q[4]) {
  float w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
__device__ __forceinline__ void mat_vec(float r[3], const float m[9], const float v[3]) {
  float a = m[0] * v[0] + m[1] * v[1] + m[2] * v[2];
  float b = m[3] * v[0] + m[4] * v[1] + m[5] * v[2];
  float c = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
  r[0] = a; r[1] = b; r[2] = c;
}
template <class PM>
__device__ __forceinline__ void matT_vec(float r[3], const PM* m, const float v[3]) {
  float a = m[0] * v[0] + m[3] * v[1] + m[6] * v[2];
  float b = m[1] * v[0] + m[4] * v[1] + m[7] * v[2];
  float c = m[2] * v[0] + m[5] * v[1] + m[8] * v[2];
  r[0] = a; r[1] = b; r[2] = c;
}
__device__ __forceinline__ void rot_quat(float r[3], const float v[3], const float q[4]) {
  float m[9];
  quat2mat(m, q);
  mat_vec(r, m, v);
}
__device__ __forceinline__ void cross3(float r[3], const float a[3], const float b[3]) {
  float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
__device__ __forceinline__ float dot3(const float a[3], const float b[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
__device__ __forceinline__ float normalize3(float a[3]) {
  float n = sqrtf(dot3(a, a));
  if (n < kMinVal) { a[0] = 1; a[1] = a[2] = 0; return n; }
  float in = 1.0f / n;
  a[0] *= in; a[1] *= in; a[2] *= in;
  return n;
}
__device__ __forceinline__ void axis_angle_quat(float q[4], const float ax[3], float ang) {
  float s, c;
  sincosf(0.5f * ang, &s, &c);
  q[0] = c; q[1] = ax[0] * s; q[2] = ax[1] * s; q[3] = ax[2] * s;
}
template <class PI>
__device__ __forceinline__ void mul_inert_vec(float r[6], const PI* i, const float v[6]) {
  r[0] = i[0] * v[0] + i[3] * v[1] + i[4] * v[2] - i[8] * v[4] + i[7] * v[5];
  r[1] = i[3] * v[0] + i[1] * v[1] + i[5] * v[2] + i[8] * v[3] - i[6] * v[5];
  r[2] = i[4] * v[0] + i[5] * v[1] + i[2] * v[2] - i[7] * v[3] + i[6] * v[4];
  r[3] = i[8] * v[1] - i[7] * v[2] + i[9] * v[3];
  r[4] = i[6] * v[2] - i[8] * v[0] + i[9] * v[4];
  r[5] = i[7] * v[0] - i[6] * v[1] + i[9] * v[5];
}
template <class PR, class PV, class PU>
__device__ __forceinline__ void cross_motion(PR* r, const PV* v, const PU* u) {
  float t0 = -v[2] * u[1] + v[1] * u[2];
  float t1 = v[2] * u[0] - v[0] * u[2];
  float t2 = -v[1] * u[0] + v[0] * u[1];
  float t3 = -v[2] * u[4] + v[1] * u[5] - v[5] * u[1] + v[4] * u[2];
  float t4 = v[2] * u[3] - v[0] * u[5] + v[5] * u[0] - v[3] * u[2];
  float t5 = -v[1] * u[3] + v[0] * u[4] - v[4] * u[0] + v[3] * u[1];
  r[0] = t0; r[1] = t1; r[2] = t2; r[3] = t3; r[4] = t4; r[5] = t5;
}
template <class PR, class PV, class PF>
__device__ __forceinline__ void cross_force(PR* r, const PV* v, const PF* f) {
  float t0 = -v[2] * f[1] + v[1] * f[2] - v[5] * f[4] + v[4] * f[5];
  float t1 = v[2] * f[0] - v[0] * f[2] + v[5] * f[3] - v[3] * f[5];
  float t2 = -v[1] * f[0] + v[0] * f[1] - v[4] * f[3] + v[3] * f[4];
  float t3 = -v[2] * f[4] + v[1] * f[5];
  float t4 = v[2] * f[3] - v[0] * f[5];
  float t5 = -v[1] * f[3] + v[0] * f[4];
  r[0] = t0; r[1] = t1; r[2] = t2; r[3] = t3; r[4] = t4; r[5] = t5;
}
__device__ __forceinline__ bool is_bad(float x) { return !(x == x) || x > kMaxVal || x < -kMaxVal; }
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

}  // namespace
}  // namespace mrs
