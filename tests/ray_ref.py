"""Reference side of the ray-query tests: the fp64 oracle's mj_ray (binding.OracleData.ray) over arrays
of rays, and the acceptance rule -- the project's rangefinder rule (tests/test_gpu_parity.py
_compare_rollout), restated self-contained:

1. hit / miss disagreement on at most 0.2 % of rays;
2. among common hits, relative error |d - d_ref| / max(1, d_ref) above 2e-5 on at most 0.5 %, and a
   median below 1e-6;
3. on every ray that is not an outlier of rule 1 or 2, geomid equals the oracle's;
4. every outlier grazes: the oracle's own answer changes (hit / miss, geom id, or distance by more than
   1e-4 relative) when the ray direction is turned by 1e-4 rad about either axis perpendicular to it, in
   either sense;
5. a failing non-grazing ray is printed with its env, index and both answers.

The caps are conditions, not tolerances: the scenes and seeds of the tests keep the oracle compared with
itself at inputs perturbed by one fp32 rounding inside them (tests/test_ray_scenes.py, no GPU needed)."""
import numpy as np

FLIP_CAP, ERR_TOL, ERR_CAP, MEDIAN_CAP = 0.002, 2e-5, 0.005, 1e-6
GRAZE_ANGLE, GRAZE_REL = 1e-4, 1e-4


def f32(a) -> np.ndarray:
    """fp32-rounded values as fp64: what both sides are given"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def quat_mat(q) -> np.ndarray:
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def oracle_rays(od, pnt, vec, bodyexclude=-1):
    """od.ray over rays [R, 3]: (dist [R], geomid [R])"""
    pnt, vec = np.asarray(pnt, dtype=np.float64).reshape(-1, 3), np.asarray(vec, dtype=np.float64).reshape(-1, 3)
    d, g = np.empty(len(pnt)), np.empty(len(pnt), dtype=np.int32)
    for k in range(len(pnt)):
        d[k], g[k] = od.ray(pnt[k], vec[k], bodyexclude)
    return d, g


def to_world(pos, mat, pnt, vec):
    """rays [R, 3] of a frame with world position pos [3] and rotation mat [3, 3] (or row-major [9])"""
    R = np.asarray(mat, dtype=np.float64).reshape(3, 3)
    return np.asarray(pos) + np.asarray(pnt) @ R.T, np.asarray(vec) @ R.T


def grazes(od, p, v, bodyexclude=-1) -> bool:
    """rule 4 for one world ray"""
    d0, g0 = od.ray(p, v, bodyexclude)
    n = np.linalg.norm(v)
    if n == 0:
        return False
    a = np.cross(v, [1.0, 0, 0] if abs(v[0]) < 0.9 * n else [0, 1.0, 0])
    a /= np.linalg.norm(a)
    b = np.cross(v, a) / n
    for axis in (a, b):
        for s in (GRAZE_ANGLE, -GRAZE_ANGLE):
            # Rodrigues, axis perpendicular to v
            v1 = v * np.cos(s) + np.cross(axis, v) * np.sin(s)
            d1, g1 = od.ray(p, v1, bodyexclude)
            if (d1 < 0) != (d0 < 0) or g1 != g0 or (d0 >= 0 and abs(d1 - d0) > GRAZE_REL * max(1.0, d0)):
                return True
    return False


def check(name, ods, pnt, vec, dist, geomid=None, ref=None, bodyexclude=-1, idmap=None):
    """rules 1-5 for one query.  ods: one forwarded OracleData per env; pnt / vec: the world rays
    [n, R, 3] given to the oracle; dist [n, R] and geomid [n, R] (or None) the answers under test; ref: the
    oracle's answers (dist, geomid) when already computed; idmap: oracle geom id -> id of the scene under
    test (a filter's reference scene is compiled without the removed geoms).  Returns the outlier count"""
    pnt, vec = np.asarray(pnt, dtype=np.float64), np.asarray(vec, dtype=np.float64)
    n, R = pnt.shape[:2]
    dist = np.asarray(dist, dtype=np.float64).reshape(n, R)
    if ref is None:
        both = [oracle_rays(ods[e], pnt[e], vec[e], bodyexclude) for e in range(n)]
        ref = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    d_ref, g_ref = np.asarray(ref[0]).reshape(n, R), np.asarray(ref[1]).reshape(n, R)
    if idmap is not None:
        g_ref = np.where(g_ref >= 0, np.asarray(idmap)[np.maximum(g_ref, 0)], -1)
    flip = (dist < 0) != (d_ref < 0)
    hit = (dist >= 0) & (d_ref >= 0)
    err = np.zeros_like(dist)
    err[hit] = np.abs(dist[hit] - d_ref[hit]) / np.maximum(1.0, d_ref[hit])
    out = flip | (err > ERR_TOL)
    med = float(np.median(err[hit])) if hit.any() else 0.0
    print(f"{name}: {n} x {R} rays, {int(hit.sum())} common hits, {int(flip.sum())} flips, "
          f"{int((err > ERR_TOL).sum())} above {ERR_TOL:g}, max rel err {err.max() if err.size else 0:.2e}, median {med:.2e}")
    assert np.isfinite(dist).all(), f"{name}: non-finite distance"
    assert np.all((dist >= 0) | (dist == -1)), f"{name}: a miss must be exactly -1"
    assert flip.mean() <= FLIP_CAP, f"{name}: hit / miss disagreement on {flip.mean():.4f} of rays"
    if hit.any():
        assert np.mean(err[hit] > ERR_TOL) <= ERR_CAP, f"{name}: {np.mean(err[hit] > ERR_TOL):.4f} of hits above {ERR_TOL:g}"
        assert med < MEDIAN_CAP, f"{name}: median rel err {med:.2e}"
    if geomid is not None:
        geomid = np.asarray(geomid).reshape(n, R)
        assert np.all(geomid[dist < 0] == -1), f"{name}: a miss must give geomid -1"
        for e, k in np.argwhere((geomid != g_ref) & ~out):
            print(f"{name}: env {e} ray {k}: geomid {geomid[e, k]} dist {dist[e, k]!r}, oracle {g_ref[e, k]} {d_ref[e, k]!r}")
        assert np.array_equal(geomid[~out], g_ref[~out]), f"{name}: geomid differs on a ray that is no outlier"
    for e, k in np.argwhere(out):
        if not grazes(ods[e], pnt[e, k], vec[e, k], bodyexclude):
            print(f"{name}: env {e} ray {k}: dist {dist[e, k]!r}, oracle {d_ref[e, k]!r} (geom {g_ref[e, k]})")
            raise AssertionError(f"{name}: outlier that does not graze (env {e}, ray {k})")
    return int(out.sum())
