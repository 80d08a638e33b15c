#!/usr/bin/env python3
"""Timing of the batched ray query (Batch.ray_device) on one GPU: one JSON line.

1. C3's scene (arm7_lidar), 8192 envs, a shared 32 x 32 grid of rays in the last link's geom frame:
   microseconds per launch and rays per second.
2. C4's scene (mobile_base), 2048 envs, the camera's 640 x 480 pixel rays as a shared pattern through
   FRAME_CAMERA, next to render_depth_device on the same batch in the same run, the two alternating: the
   depth kernel casts the same number of rays through the same primitives with a tile cull the query
   lacks, so it is the yardstick (ratio = query time / depth time).

Each figure is the median over --reps launches timed one by one with HIP events on the batch stream,
after --warmup launches of the same shape; the spread (min, max) is reported beside it.  Separate from
bench.py: nothing here gates anything.

    python scripts/bench_ray_query.py [--reps 30] [--warmup 5] [--envs3 8192] [--envs4 2048]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timed(torch, stream, launches, warmup, reps):
    """per-launch milliseconds [len(launches), reps] of the launches alternating, HIP events on `stream`"""
    for _ in range(warmup):
        for f in launches:
            f()
    stream.synchronize()
    evs = []
    for _ in range(reps):
        for f in launches:
            e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            e[0].record(stream)
            f()
            e[1].record(stream)
            evs.append(e)
    stream.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in evs]).reshape(reps, len(launches)).T
    return ms


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--envs3", type=int, default=8192)
    ap.add_argument("--envs4", type=int, default=2048)
    args = ap.parse_args()

    import torch
    from mujoco_ros2_simulation_amd import sim, synth

    if not torch.cuda.is_available():
        sys.exit("bench_ray_query.py: no GPU (there is no CPU path to time)")
    stream = torch.cuda.Stream()
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup}

    def posed(scene, n):
        model = sim.Model.load(ROOT / "scenes" / scene)
        b = sim.Batch(model, n)
        b.set_stream(stream.cuda_stream)
        b.set(sim.FIELD_QPOS, synth.initial_qpos(model, np.arange(n)))
        b.step(10)
        b.sync()
        return model, b

    def dev(a, dtype=None):
        with torch.cuda.stream(stream):
            return torch.tensor(a, dtype=dtype or torch.float32, device="cuda").contiguous()

    # 1. C3: a shared 32 x 32 height-scanner grid under the last link
    n = args.envs3
    model, b = posed("arm7_lidar.xml", n)
    gx, gy = np.meshgrid(np.linspace(-0.5, 0.5, 32), np.linspace(-0.5, 0.5, 32), indexing="ij")
    pnt = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.2)], axis=1)
    vec = np.tile([0.0, 0.0, -1.0], (gx.size, 1))
    dp, dv = dev(pnt), dev(vec)
    with torch.cuda.stream(stream):
        dist = torch.empty((n, gx.size), dtype=torch.float32, device="cuda")
        gid = torch.empty((n, gx.size), dtype=torch.int32, device="cuda")
    frame = ("geom", model.name2id(sim.OBJ_GEOM, "g7"))
    ms = timed(torch, stream, [lambda: b.ray_device(dp.data_ptr(), dv.data_ptr(), gx.size, dist.data_ptr(), gid.data_ptr(),
                                                    shared=True, frame=frame)], args.warmup, args.reps)[0]
    with torch.cuda.stream(stream):
        hit = float((dist >= 0).float().mean().cpu())
    result["c3_grid"] = {"scene": "arm7_lidar", "envs": n, "rays_per_env": int(gx.size), "ngeom": model.ngeom,
                         "hit_share": hit, **stats(ms), "us_per_launch": float(np.median(ms) * 1e3),
                         "rays_per_s": float(n * gx.size / (np.median(ms) * 1e-3))}
    del dist, gid
    b.close()

    # 2. C4: the camera's pixel rays as a query, next to the depth kernel
    n = args.envs4
    model, b = posed("mobile_base.xml", n)
    W, H = (int(x) for x in model.cam_resolution[0])
    f = 0.5 * H / np.tan(np.deg2rad(model.cam_fovy[0]) / 2)
    px, py = np.meshgrid((np.arange(W) + 0.5 - W / 2) / f, (H / 2 - np.arange(H) - 0.5) / f, indexing="xy")
    vec = np.stack([px.ravel(), py.ravel(), np.full(px.size, -1.0)], axis=1)
    dp, dv = dev(np.zeros_like(vec)), dev(vec)
    with torch.cuda.stream(stream):
        dist = torch.empty((n, H * W), dtype=torch.float32, device="cuda")
        frames = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    b.set_timing(0)
    ms = timed(torch, stream, [lambda: b.ray_device(dp.data_ptr(), dv.data_ptr(), H * W, dist.data_ptr(), 0, shared=True,
                                                    frame=("camera", 0)),
                               lambda: b.render_depth_device(0, 0, n, frames.data_ptr())], args.warmup, args.reps)
    with torch.cuda.stream(stream):
        # the same rays: where both hit inside the view range the two depths agree (ray parameter = eye depth)
        d, z = dist.view(n, H, W)[:4], frames[:4]
        both = (d > 0.05) & (z > 0.05) & (z < 100)
        agree = float(((d - z).abs()[both] < 1e-3 * z[both]).float().mean().cpu()) if bool(both.any()) else None
    rays = n * H * W
    result["c4_camera"] = {"scene": "mobile_base", "envs": n, "rays_per_env": H * W, "ngeom": model.ngeom,
                           "query": {**stats(ms[0]), "ns_per_ray": float(np.median(ms[0]) * 1e6 / rays)},
                           "depth_kernel": {**stats(ms[1]), "ns_per_ray": float(np.median(ms[1]) * 1e6 / rays)},
                           "query_over_depth": float(np.median(ms[0]) / np.median(ms[1])),
                           "depth_agreement_share": agree}
    b.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
