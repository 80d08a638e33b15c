// mjModel / mjData lifecycle (include/mujoco_ros2_control/mj_types.hpp).
#include "mujoco_ros2_control/mj_types.hpp"

#include <cstring>
#include <new>

namespace {

void fill_view(mjModel* m) {
  mrs_model_view v{};
  mrs_model_view_get(m->handle, &v);
  static_cast<mrs_model_view&>(*m) = v;
  mjOption& o = m->opt;
  o.timestep = v.timestep;
  for (int k = 0; k < 3; ++k) o.gravity[k] = v.gravity[k];
  o.tolerance = v.tolerance;
  o.impratio = v.impratio;
  o.ls_tolerance = v.ls_tolerance;
  o.integrator = v.integrator;
  o.solver = v.solver;
  o.iterations = v.iterations;
  o.ls_iterations = v.ls_iterations;
  o.cone = v.cone;
  o.disableflags = v.disableflags;
}

}  // namespace

mjModel* mj_wrapModel(mrs_model* handle) {
  if (!handle) return nullptr;
  mjModel* m = new mjModel();
  m->handle = handle;
  fill_view(m);
  return m;
}

mjModel* mj_copyModel(mjModel* dest, const mjModel* src) {
  if (!src || !src->handle) return nullptr;
  mrs_model* copy = mrs_model_copy(src->handle);
  if (!copy) return nullptr;
  if (!dest) return mj_wrapModel(copy);
  mrs_model_free(dest->handle);
  dest->handle = copy;
  fill_view(dest);
  return dest;
}

void mj_deleteModel(mjModel* m) {
  if (!m) return;
  mrs_model_free(m->handle);
  delete m;
}

mjData* mj_makeData(const mjModel* m) {
  if (!m) return nullptr;
  mjData* d = new mjData();
  d->nq = m->nq;
  d->nv = m->nv;
  d->nu = m->nu;
  d->nsensordata = m->nsensordata;
  d->nbody = m->nbody;
  d->na = m->na;
  d->nmocap = m->nmocap;
  const size_t n = size_t(d->nq) + 5 * size_t(d->nv) + size_t(d->nu) + size_t(d->nsensordata) + 6 * size_t(d->nbody) +
                   size_t(d->na) + 7 * size_t(d->nmocap);
  d->buffer = new double[n > 0 ? n : 1]();
  double* p = d->buffer;
  auto take = [&p](int k) { double* r = p; p += k; return r; };
  d->qpos = take(d->nq);
  d->qvel = take(d->nv);
  d->qacc = take(d->nv);
  d->qacc_warmstart = take(d->nv);
  d->ctrl = take(d->nu);
  d->qfrc_applied = take(d->nv);
  d->qfrc_actuator = take(d->nv);
  d->sensordata = take(d->nsensordata);
  d->xfrc_applied = take(6 * d->nbody);
  d->act = take(d->na);
  d->mocap_pos = take(3 * d->nmocap);
  d->mocap_quat = take(4 * d->nmocap);
  for (int b = 0; b < m->nbody && d->nmocap > 0; ++b) {
    const int id = m->body_mocapid[b];
    if (id < 0) continue;
    std::memcpy(d->mocap_pos + 3 * id, m->body_pos + 3 * b, 3 * sizeof(double));
    std::memcpy(d->mocap_quat + 4 * id, m->body_quat + 4 * b, 4 * sizeof(double));
  }
  return d;
}

mjData* mj_copyData(mjData* dest, const mjModel* m, const mjData* src) {
  if (!m || !src) return nullptr;
  if (src->nq != m->nq || src->nv != m->nv || src->nu != m->nu || src->nsensordata != m->nsensordata ||
      src->nbody != m->nbody || src->na != m->na || src->nmocap != m->nmocap)
    return nullptr;
  if (!dest) dest = mj_makeData(m);
  else if (dest->nq != m->nq || dest->nv != m->nv || dest->nu != m->nu || dest->nsensordata != m->nsensordata ||
           dest->nbody != m->nbody || dest->na != m->na || dest->nmocap != m->nmocap)
    return nullptr;
  const size_t n = size_t(m->nq) + 5 * size_t(m->nv) + size_t(m->nu) + size_t(m->nsensordata) + 6 * size_t(m->nbody) +
                   size_t(m->na) + 7 * size_t(m->nmocap);
  if (dest != src) std::memcpy(dest->buffer, src->buffer, n * sizeof(double));
  dest->time = src->time;
  return dest;
}

void mj_deleteData(mjData* d) {
  if (!d) return;
  delete[] d->buffer;
  delete d;
}
