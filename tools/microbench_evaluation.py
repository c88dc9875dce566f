"""Time the point-cloud evaluation (pointmvsnet_amd/evaluation.py) on a DTU-sized scan.

    python tools/microbench_evaluation.py [--views 49] [--height 480] [--width 640] [--outliers 0.02] [--runs 5] [--no-scipy]

Fuses the 49-view 640 x 480 plane scan of tools/microbench_fusion.py, adds far outliers (``--outliers`` of the fused points,
uniformly in the cloud's bounding box stretched to a cube) and scores the result against the plane sampled at 0.2 pitch.
Prints one JSON line: points in, points after thinning, thinning rounds, the time of the thinning and of each of the two
searches (HIP events around the call, so the sort and the other plumbing of the call are inside; the kernel entries alone
are listed next to them), of the whole ``evaluate_point_cloud`` (wall clock around a device synchronisation), medians of
``--runs``, and ``cKDTree.query(..., workers=16, distance_upper_bound=max_dist)`` on the same clouds on the same machine
(one run each, tree construction reported apart).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(fn, runs):
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return median(out), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--outliers", type=float, default=0.02)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import _lib, evaluation as EV, fusion
    depths, K, E, _ = make_scan(args.views, args.height, args.width)
    dev = torch.device("cuda:0")
    pts, _ = fusion.fuse_depth_maps(torch.from_numpy(depths).to(dev), K, E)
    fused = pts.cpu().numpy()
    rng = np.random.default_rng(0)
    lo, hi = fused.min(axis=0), fused.max(axis=0)
    mid, half = (lo + hi) / 2.0, float((hi - lo).max()) / 2.0
    n_out = int(round(args.outliers * len(fused)))
    outliers = rng.uniform(mid - half, mid + half, (n_out, 3)).astype(np.float32)
    data_np = np.concatenate([fused, outliers])
    # ground truth: the scan's plane n . X = n . target sampled at 0.2 pitch over the fused cloud's footprint
    n = np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    target = np.array([0.0, 0.0, 600.0])
    u = np.cross(n, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    rel = fused.astype(np.float64) - target
    cu, cv = rel @ u, rel @ v
    gu, gv = np.meshgrid(np.arange(cu.min(), cu.max(), 0.2), np.arange(cv.min(), cv.max(), 0.2), indexing="ij")
    gt_np = (target + gu[..., None] * u + gv[..., None] * v).reshape(-1, 3).astype(np.float32)
    data, gt = torch.from_numpy(data_np).to(dev), torch.from_numpy(gt_np).to(dev)

    scores = EV.evaluate_point_cloud(data, gt)                                 # warm-up of every shape
    torch.cuda.synchronize()
    walls = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        scores = EV.evaluate_point_cloud(data, gt)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    thin_ms, thinned = event_ms(lambda: EV.thin_points(data), args.runs)
    rounds = EV.last_thinning_rounds()
    acc_ms, _ = event_ms(lambda: EV.nearest_distances(thinned, gt), args.runs)
    acc_unfinished = EV.last_unfinished_queries()
    comp_ms, _ = event_ms(lambda: EV.nearest_distances(gt, thinned), args.runs)
    comp_unfinished = EV.last_unfinished_queries()
    timer = _lib.KernelTimer()
    _lib.set_timer(timer)
    EV.thin_points(data)
    mark = len(timer.records)
    EV.nearest_distances(thinned, gt)
    mark2 = len(timer.records)
    EV.nearest_distances(gt, thinned)
    _lib.set_timer(None)
    torch.cuda.synchronize()

    def kernels(records):
        out = {}
        for name, e0, e1, _, _, _ in records:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out

    out = {"views": args.views, "height": args.height, "width": args.width, "outlier_share": args.outliers,
           "points_in": int(data.shape[0]), "points_thinned": int(thinned.shape[0]), "gt_points": int(gt.shape[0]),
           "thinning_rounds": rounds, "thin_ms": thin_ms, "accuracy_search_ms": acc_ms, "completeness_search_ms": comp_ms,
           "accuracy_unfinished_after_cells": acc_unfinished, "completeness_unfinished_after_cells": comp_unfinished,
           "evaluate_ms_median": median(walls), "evaluate_ms_all": walls, "runs": args.runs,
           "thin_kernels_ms_one_run": kernels(timer.records[:mark]),
           "accuracy_kernels_ms_one_run": kernels(timer.records[mark:mark2]),
           "completeness_kernels_ms_one_run": kernels(timer.records[mark2:]), "scores": scores}
    if not args.no_scipy:
        from scipy.spatial import cKDTree
        th = thinned.cpu().numpy().astype(np.float64)
        g64 = gt_np.astype(np.float64)
        t0 = time.perf_counter()
        tree_gt = cKDTree(g64)
        t1 = time.perf_counter()
        tree_gt.query(th, workers=16, distance_upper_bound=20.0)
        t2 = time.perf_counter()
        tree_th = cKDTree(th)
        t3 = time.perf_counter()
        tree_th.query(g64, workers=16, distance_upper_bound=20.0)
        t4 = time.perf_counter()
        out.update(scipy_accuracy_build_ms=(t1 - t0) * 1e3, scipy_accuracy_query_ms=(t2 - t1) * 1e3,
                   scipy_completeness_build_ms=(t3 - t2) * 1e3, scipy_completeness_query_ms=(t4 - t3) * 1e3,
                   scipy_runs=1, scipy_workers=16)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
