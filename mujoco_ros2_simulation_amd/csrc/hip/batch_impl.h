// The batch as its two translation units see it: batch.hip (creation, env arrays, resets, exports, step
// launches) and render.hip (frames and ray queries).  Private to those two: capi.cc goes through batch.h
// and never sees BatchImpl's members.
#pragma once

#include <hip/hip_runtime.h>

#include <deque>
#include <stdexcept>
#include <string>
#include <vector>

#include "../mjcf/model.h"
#include "batch.h"
#include "devmodel.h"
#include "rayfilter.h"
#include "start_rows.h"

namespace mrs {

#define HIP_CHECK(x)                                                                         \
  do {                                                                                       \
    hipError_t err_ = (x);                                                                   \
    if (err_ != hipSuccess)                                                                  \
      throw DeviceError(std::string(#x) + " failed: " + hipGetErrorString(err_));            \
  } while (0)

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
  std::vector<int> pair_g1, pair_g2;  // host copy of the collision pairs the device walks (contact export)
  int pairs_pruned = 0;               // admissible pairs left out of them (devtables.h prune_pairs)
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
  // the model needs the extended step kernels (step/base.h MRS_EXT): general convex (MPR) collision
  // pairs, or rangefinders with more than 32 ray geoms
  bool ext = false;
};

// a zero-filled device allocation that lives as long as the batch
inline void* dalloc(BatchImpl& b, size_t bytes) {
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
  HIP_CHECK(hipMemsetAsync(p, 0, bytes ? bytes : 16, b.stream));
  b.allocs.push_back(p);
  return p;
}

inline void check_env_range(const BatchImpl& b, int env0, int n) {
  if (env0 < 0 || n < 0 || env0 + n > b.n) throw std::invalid_argument("env range out of bounds");
}

// render.hip: the render stream and its events, the triangle lists and the ray lists, released once the
// batch's streams have drained (batch_free)
void render_free(BatchImpl& b);

}  // namespace mrs
