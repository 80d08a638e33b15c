// Batched ray queries against the posed scene (mrs_batch_ray_device, include/mrs.h): mj_ray /
// mj_multiRay for arbitrary rays of every env.  Included by render.hip after ray_prim and MeshRef.
//
// One workgroup of 256 threads handles one env and a tile of 256 consecutive rays; the grid is
// (ray tiles, envs).  The workgroup stages the env's kept geoms (rayfilter.h: the compact list of the
// call's filter) in LDS -- world position, rotation, size, bounding radius, type -- in chunks of at most
// kMaxRenderGeoms, so a longer list takes several passes over the same rays.  Each lane owns one ray,
// loaded once (consecutive lanes read consecutive rays) and turned into the world by the env's frame
// pose in registers.  The geom loop is wave-uniform: every lane tests the same staged geom, so the
// primitive switch does not diverge and the geom record is an LDS broadcast read.  Per ray a
// bounding-sphere reject comes first: the sphere is beside or behind the ray, or the ray enters it past
// the nearest hit so far; the primitive test of a sphere ahead starts where the ray enters it, which
// keeps fp32's quadratics well conditioned at range.  Planes have no bounding sphere.  Mesh geoms wait for a second loop over the
// chunk (the per-lane hierarchy walk of ray_mesh diverges, so it stays out of the uniform primitive
// loop), compiled only into the instantiation that lists with a mesh launch.  The nearest hit wins and
// equal distances go to the lower geom id, the oracle's strict `<` in geom order.
#pragma once

struct RayStaged {  // one kept geom of the env in LDS: 20 words
  float p[3], R[9], size[3], r2, rb;
  int type, id, dataid;
};

struct RayQueryArgs {
  const RayGeom* list;  // the filter's kept geoms, geom order
  int nkeep, ngeom;
  const float *geom_xpos, *geom_xmat;  // [n_envs][ngeom][3] / [9]
  // the frame's pose per env (null: world rays): env e's is frame_pos + e * frame_stride * 3 and
  // frame_mat + e * frame_stride * 9
  const float *frame_pos, *frame_mat;
  int frame_stride;
  const float *pnt, *vec;  // rows of the first env of the launch ([n][n_rays][3], or [n_rays][3] shared)
  int n_rays, shared, env0;
  float* dist;  // [n][n_rays], row 0 = env0
  int* geomid;  // likewise, or null
};

template <bool kMesh>
__global__ __launch_bounds__(256) void ray_query_kernel(const RayQueryArgs a, const MeshRef mesh) {
  __shared__ RayStaged G[kMaxRenderGeoms];
  __shared__ float F[12];
  const int row = blockIdx.y;
  const size_t e = static_cast<size_t>(a.env0) + row;
  const int r = blockIdx.x * 256 + threadIdx.x;
  const bool live = r < a.n_rays;
  const bool framed = a.frame_pos != nullptr;
  if (framed && threadIdx.x < 12)
    F[threadIdx.x] = threadIdx.x < 3 ? a.frame_pos[e * a.frame_stride * 3 + threadIdx.x]
                                     : a.frame_mat[e * a.frame_stride * 9 + threadIdx.x - 3];
  float o[3] = {0, 0, 0}, v[3] = {0, 0, 0};
  if (live) {
    const size_t at = ((a.shared ? 0 : static_cast<size_t>(row) * a.n_rays) + r) * 3;
    for (int i = 0; i < 3; ++i) { o[i] = a.pnt[at + i]; v[i] = a.vec[at + i]; }
  }
  if (framed) {
    __syncthreads();
    const float lo[3] = {o[0], o[1], o[2]}, lv[3] = {v[0], v[1], v[2]};
    for (int i = 0; i < 3; ++i) {
      o[i] = F[i] + F[3 + 3 * i] * lo[0] + F[4 + 3 * i] * lo[1] + F[5 + 3 * i] * lo[2];
      v[i] = F[3 + 3 * i] * lv[0] + F[4 + 3 * i] * lv[1] + F[5 + 3 * i] * lv[2];
    }
  }
  const float vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  // a zero (or non-finite) direction hits nothing: the lane sits the loops out, it is never divided by
  const bool cast = live && vv > 0 && vv < 3.0e38f;
  const float ivv = cast ? 1.0f / vv : 0.0f, ivn = cast ? rsqrtf(vv) : 0.0f;
  float best = -1;
  int bestg = -1;

  for (int c0 = 0; c0 < a.nkeep; c0 += kMaxRenderGeoms) {
    const int nc = min(kMaxRenderGeoms, a.nkeep - c0);
    __syncthreads();  // (the chunk before has been read by every lane)
    if (threadIdx.x < nc) {
      const RayGeom s = a.list[c0 + threadIdx.x];
      RayStaged& t = G[threadIdx.x];
      const float* p = a.geom_xpos + (e * a.ngeom + s.id) * 3;
      const float* R = a.geom_xmat + (e * a.ngeom + s.id) * 9;
      for (int i = 0; i < 3; ++i) { t.p[i] = p[i]; t.size[i] = s.size[i]; }
      for (int i = 0; i < 9; ++i) t.R[i] = R[i];
      t.rb = s.rbound * 1.001f + 1e-4f;
      t.r2 = t.rb * t.rb;
      t.type = s.type; t.id = s.id; t.dataid = s.dataid;
    }
    __syncthreads();
    if (!cast) continue;
    for (int pass = 0; pass < (kMesh ? 2 : 1); ++pass) {
      for (int k = 0; k < nc; ++k) {
        const RayStaged& t = G[k];
        if ((t.type == MRS_GEOM_MESH) != (pass == 1)) continue;  // (wave-uniform)
        float d[3] = {t.p[0] - o[0], t.p[1] - o[1], t.p[2] - o[2]};
        float t0 = 0;  // the ray parameter the primitive test starts from
        if (t.type != MRS_GEOM_PLANE) {
          // the ray's nearest point to the centre, s along the ray: the sphere is missed when that point
          // is outside it, behind when s < 0 with the origin outside, and cannot beat the nearest hit
          // when even its near side, s - rb / |v|, lies past it
          const float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
          const float s = (d[0] * v[0] + d[1] * v[1] + d[2] * v[2]) * ivv;
          const float q[3] = {d[0] - s * v[0], d[1] - s * v[1], d[2] - s * v[2]};
          const float qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
          const float near = s - t.rb * ivn;
          const bool skip = (qq > t.r2) | ((s < 0) & (dd > t.r2)) | ((best >= 0) & (near > best));
          if (skip) continue;
          // a sphere ahead of the origin: the test starts where the ray enters it.  Every hit lies inside
          // the sphere, so none is lost, and the quadratics of ray_prim see an origin one radius from the
          // geom instead of the whole range away (b^2 - a c cancels to rb^2, not to range^2: a 2 cm sphere
          // at 1 m otherwise loses 2e-6 of its distance)
          t0 = fmaxf(near, 0.0f);
          for (int i = 0; i < 3; ++i) d[i] -= t0 * v[i];
        }
        float lp[3], lv[3];
        for (int i = 0; i < 3; ++i) {
          lp[i] = -(t.R[i] * d[0] + t.R[3 + i] * d[1] + t.R[6 + i] * d[2]);
          lv[i] = t.R[i] * v[0] + t.R[3 + i] * v[1] + t.R[6 + i] * v[2];
        }
        float th;
        if (kMesh && pass == 1)
          th = mesh.ray(t.dataid, t.size, lp, lv);
        else
          th = ray_prim(t.type, t.size, lp, lv);
        if (th >= 0) th += t0;
        if (th >= 0 && (best < 0 || th < best || (th == best && t.id < bestg))) { best = th; bestg = t.id; }
      }
    }
  }
  if (live) {
    const size_t at = static_cast<size_t>(row) * a.n_rays + r;
    a.dist[at] = best;
    if (a.geomid) a.geomid[at] = bestg;
  }
}
