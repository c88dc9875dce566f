"""Time the depth-map fusion (pointmvsnet_amd/fusion.py) on a DTU-sized scan: 49 views of 640 x 480.

    python tools/microbench_fusion.py [--views 49] [--height 480] [--width 640] [--numpy-views 2]

The cameras sit on a 7 x 7 grid facing a tilted plane ~600 units away, so that -- as on DTU -- every view overlaps most of
the others and the partner gathers really happen; depth maps by ray-plane intersection plus noise.  Prints one JSON line:
the whole fusion (Stage A, V mark launches, prefix sum, compaction; median of the runs, wall clock around a device
synchronisation), Stage A alone (HIP events, with its algorithmic bytes -> GB/s) and the float64 NumPy statement of
tests/test_fusion.py on the same machine, timed on ``--numpy-views`` reference views and scaled to all of them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def make_scan(V, h, w, seed=0):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(V)))
    target = np.array([0.0, 0.0, 600.0])
    n = np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    K = np.array([[361.5 * w / 160.0, 0.0, w / 2.0], [0.0, 361.5 * w / 160.0, h / 2.0], [0.0, 0.0, 1.0]])
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
    depths, Ks, Es = [], [], []
    for v in range(V):
        centre = np.array([(v % side - (side - 1) / 2.0) * 60.0, (v // side - (side - 1) / 2.0) * 60.0, 0.0])
        fwd = (target - centre) / np.linalg.norm(target - centre)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])                      # world -> camera
        t = -R @ centre
        d = (n @ target - n @ centre) / (rays @ (R @ n))                        # n . (R^T ray d + centre) = n . target
        depths.append((d + rng.normal(0.0, 0.3, d.shape)).astype(np.float32))
        Ks.append(K)
        Es.append(np.concatenate([R, t[:, None]], 1))
    return np.stack(depths), np.stack(Ks), np.stack(Es), rng.integers(0, 256, (V, h, w, 3), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--numpy-views", type=int, default=2)
    args = ap.parse_args()
    from pointmvsnet_amd import _lib, fusion
    depths, K, E, images = make_scan(args.views, args.height, args.width)
    dev = torch.device("cuda:0")
    d_dev, i_dev = torch.from_numpy(depths).to(dev), torch.from_numpy(images).to(dev)
    pts, _ = fusion.fuse_depth_maps(d_dev, K, E, images=i_dev)                 # warm-up
    torch.cuda.synchronize()
    walls = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        pts, _ = fusion.fuse_depth_maps(d_dev, K, E, images=i_dev)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    timer = _lib.KernelTimer(only="pf_fuse_stage_a_f32")
    _lib.set_timer(timer)
    for _ in range(args.runs):
        fusion.fuse_depth_maps(d_dev, K, E, images=i_dev)
    _lib.set_timer(None)
    a = timer.summary()["pf_fuse_stage_a_f32"]
    out = {"views": args.views, "height": args.height, "width": args.width, "points": int(pts.shape[0]),
           "fusion_ms_median": sorted(walls)[len(walls) // 2], "fusion_ms_all": walls,
           "stage_a_ms": a["ms"] / a["launches"], "stage_a_algo_gbytes": a["bytes"] / a["launches"] / 1e9,
           "stage_a_gbytes_per_s": a["bytes"] / a["ms"] / 1e6, "event_floor_ms": a["event_floor_ms"]}
    if args.numpy_views > 0:
        import test_fusion as TF
        # the statement walks all V reference views; time it on the first few (every view costs the same V - 1 partners)
        nv = min(args.numpy_views, args.views)
        t0 = time.perf_counter()
        TF.statement_stage_a(depths, K, E, images, views=range(nv))
        per_view = (time.perf_counter() - t0) / nv
        out["numpy_stage_a_s_per_view"] = per_view
        out["numpy_stage_a_s_extrapolated"] = per_view * args.views
    print(json.dumps(out))


if __name__ == "__main__":
    main()
