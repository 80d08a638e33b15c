// The plan of a frame launch: which of the three depth kernels (render.hip) renders n frames of a
// camera, with which template argument, LDS bytes, grid and frame chunk, chosen from the model's counts,
// the frame size, the device's LDS limit and the render switches.  Host only, no HIP, a pure function:
// the same inputs give the same plan with or without a device (mrs_debug_render_plan).  The limits the
// decision shares with the kernels are defined here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>

#include "batch.h"

namespace mrs {

// geoms the tile kernel (depth_kernel) and a chunk of the ray query stage in LDS
constexpr int kMaxRenderGeoms = 256;
// geoms of the frame kernels (depth_kernel_v2, depth_kernel_mesh): one lane of a wave each
constexpr int kDepthGeoms = 64;
// the binned kernel's band of rows and the bands its LDS counters hold
constexpr int kBandH = 8, kMaxBands = 128;

// The render switches (tests and A/B runs).  read_render_overrides() is the one place that reads them,
// once per render call: tests set them after the batch exists
struct RenderOverrides {
  bool v1, v2;     // MRS_DEPTH_V1 / MRS_DEPTH_V2 present: the tile kernel / the frame kernel for every frame
  long budget_mb;  // MRS_RAST_BUDGET_MB: the binned kernel's triangle lists per launch (at least 1; unset: 2048)
};

inline RenderOverrides read_render_overrides() {
  const char* bud = std::getenv("MRS_RAST_BUDGET_MB");
  return {std::getenv("MRS_DEPTH_V1") != nullptr, std::getenv("MRS_DEPTH_V2") != nullptr,
          bud ? std::max(1L, std::atol(bud)) : 2048};
}

struct RenderPlan {
  // BINNED: depth_kernel_mesh, one workgroup per frame, `chunk` frames per launch; FRAME: depth_kernel_v2,
  // one workgroup per frame; TILE: depth_kernel, one workgroup per 16 x 16 pixels
  enum Kind { BINNED, FRAME, TILE } kind;
  bool mesh;              // depth_kernel_v2's kMesh: the model has mesh geoms
  std::size_t band_lds;   // dynamic LDS bytes of the binned kernel: its band of W x kBandH 64-bit keys
  int chunk;              // frames per launch of the binned kernel (1 <= chunk <= n_frames)
  std::size_t per_frame;  // bytes of one frame's triangle list
  unsigned grid_x, grid_y;  // the grid (of the first launch: a last chunk may be shorter)
};

// no kernel renders more geoms than the tile kernel stages (a render call checks this before it allocates)
inline void check_render_geoms(int ngeom) {
  if (ngeom > kMaxRenderGeoms) throw UnsupportedError("too many geoms for the depth kernel");
}

// The binned kernel needs its band in LDS (within the device's per-block limit max_lds) and a per-frame
// triangle list in global memory: frames go in chunks whose lists fit the budget, so a large mesh over
// many envs renders in several launches instead of failing the allocation.  has_mesh_geom: some geom is
// a mesh; nrast, nrast_pair: DevModel's (devtables.h raster_lists)
inline RenderPlan choose_render(int ngeom, bool has_mesh_geom, int nrast, int nrast_pair, int W, int H, int n_frames,
                                int max_lds, const RenderOverrides& o) {
  check_render_geoms(ngeom);
  RenderPlan p{};
  p.band_lds = static_cast<std::size_t>(W) * kBandH * sizeof(unsigned long long);
  const bool raster = nrast > 0 && W <= 2048 && H <= kBandH * kMaxBands && p.band_lds <= static_cast<std::size_t>(max_lds) &&
                      !o.v2 && !o.v1;
  p.per_frame = static_cast<std::size_t>(std::max(nrast_pair, 1)) * sizeof(unsigned long long);
  const std::size_t budget = static_cast<std::size_t>(o.budget_mb) << 20;
  p.chunk = static_cast<int>(std::max<std::size_t>(1, std::min<std::size_t>(n_frames, budget / p.per_frame)));
  p.mesh = nrast > 0 || has_mesh_geom;
  if (raster) {
    p.kind = RenderPlan::BINNED;
    p.grid_x = p.chunk;
    p.grid_y = 1;
  } else if (ngeom <= kDepthGeoms && !o.v1) {
    p.kind = RenderPlan::FRAME;
    p.grid_x = n_frames;
    p.grid_y = 1;
  } else {
    p.kind = RenderPlan::TILE;
    p.grid_x = ((W + 15) / 16) * ((H + 15) / 16);
    p.grid_y = n_frames;
  }
  return p;
}

}  // namespace mrs
