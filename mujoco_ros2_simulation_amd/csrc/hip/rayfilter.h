// Host only: the geoms a batched ray query may hit (mrs_batch_ray / mrs_debug_ray_filter, include/mrs.h).
// A filter triple (group mask, static flag, excluded body) keeps a subset of the model's geoms with
// mj_ray's meaning; the query kernel (rayquery.h) walks the compact list of the kept geoms, in geom
// order, so a filtered geom costs nothing per ray.  No device code and no HIP type: capi.cc includes
// this for the debug entry, render.hip for the lists it uploads.
#pragma once

#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../../include/mrs.h"
#include "../mjcf/model.h"

namespace mrs {

// One kept geom as the kernel stages it: 8 words, uploaded as they are (rayquery.h reads the same
// struct).  rbound is the model's bounding radius about the geom's frame origin (0 for a plane, which
// has no bounding sphere); dataid the mesh id of a mesh geom, else -1.
struct RayGeom {
  int id, type, dataid;
  float rbound, size[3];
  int pad;
};
static_assert(sizeof(RayGeom) == 32, "RayGeom is eight 32-bit words");

inline void check_ray_filter(const Model& m, int flags, int bodyexclude) {
  if (flags & ~(MRS_RAY_SHARED | MRS_RAY_NO_STATIC)) throw std::invalid_argument("unknown ray flag");
  if (bodyexclude < -1 || bodyexclude >= m.nbody) throw std::invalid_argument("bodyexclude out of range");
}

// mj_ray's geom elimination (engine_ray ray_eliminate, oracle.c ray_scene): the excluded body's geoms,
// the geoms with rgba alpha exactly 0 (the rule the rangefinder tables use, devtables.h), with a group
// mask the geoms whose group is outside 0..5 or not in the mask (0: every group, geomgroup == NULL),
// and with no_static the geoms of bodies welded to the world (body_weldid == 0: flg_static = 0)
inline bool ray_filter_keeps(const Model& m, int g, unsigned group_mask, bool no_static, int bodyexclude) {
  const int body = m.geom_bodyid[g];
  if (body == bodyexclude) return false;
  if (m.geom_rgba[4 * static_cast<size_t>(g) + 3] == 0) return false;
  if (group_mask) {
    const int grp = m.geom_group[g];
    if (grp < 0 || grp > 5 || !((group_mask >> grp) & 1u)) return false;
  }
  if (no_static && m.body_weldid[body] == 0) return false;
  return true;
}

// the kept geoms of a filter triple, in geom order
inline std::vector<RayGeom> build_ray_filter(const Model& m, unsigned group_mask, bool no_static, int bodyexclude) {
  std::vector<RayGeom> out;
  for (int g = 0; g < m.ngeom; ++g) {
    if (!ray_filter_keeps(m, g, group_mask, no_static, bodyexclude)) continue;
    RayGeom r;
    std::memset(&r, 0, sizeof r);
    r.id = g;
    r.type = m.geom_type[g];
    r.dataid = r.type == MRS_GEOM_MESH ? m.geom_dataid[g] : -1;
    r.rbound = static_cast<float>(m.geom_rbound[g]);
    for (int i = 0; i < 3; ++i) r.size[i] = static_cast<float>(m.geom_size[3 * static_cast<size_t>(g) + i]);
    out.push_back(r);
  }
  return out;
}

}  // namespace mrs
