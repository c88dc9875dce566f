"""Time the cloud cleaning (pointmvsnet_amd/cloud_filter.py) on a DTU-sized scan.

    python tools/microbench_cloud_filter.py [--views 49] [--height 480] [--width 640] [--outliers 0.02] [--runs 5]
        [--radius 2.0] [--voxel 0.2] [--cells 1 2 3 4] [--scipy-k 16] [--no-scipy] [--out profiles/cloud_filter_microbench.jsonl]

The scan is that of tools/microbench_evaluation.py: the fused 49-view 640 x 480 plane scan of tools/microbench_fusion.py plus
far outliers (``--outliers`` of the fused points, uniformly in the cloud's bounding box stretched to a cube), with random
colours and unit normals.  One JSON line per case, printed and appended to ``--out``; times are HIP events around warm,
back-to-back calls, medians of ``--runs``:

* ``knn``: the search at ``k`` = 8, 16, 32 and ``--radius`` for every grid pitch of ``--cells`` (cells to the radius; 1 is the
  plain form, whose 27 cells hold the radius): the grid build alone (keys, sort, pack), the search alone on the built grid,
  the candidates in the 27 cells of the first ring (mean and largest, counted from the grid's keys) and whether the result
  equals the first pitch's bit for bit; at the module's default pitch also the whole ``knn_mean_distances`` call and
  ``cKDTree.query(k + 1, distance_upper_bound=R, workers=16)`` for the ``--scipy-k`` on the same machine (one run, the tree's
  construction apart);
* ``radius``: ``radius_outlier_mask`` at ``min_neighbors`` 4;
* ``voxel``: ``voxel_downsample`` at ``--voxel`` with and without colours and normals, the reduction kernel alone, and a
  torch-only route (``torch.unique(return_inverse=True)`` on the same keys plus ``index_add_``: float32 atomics, no fixed order);
* ``clean``: ``clean_cloud`` whole (voxel, radius test, statistical test), wall clock around a device synchronisation.
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
    fn()                                                                       # warm
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return median(out), res


def candidates_per_point(grid):
    """int64 (N,), sorted order: the records a point's thread walks in the 27 cells around it (itself included)."""
    keys = grid.keys
    nx, ny, nz = grid.cells
    mask = (1 << 21) - 1
    cx, cy, cz = keys >> 42, (keys >> 21) & mask, keys & mask
    z0, z1 = (cz - 1).clamp(min=0), (cz + 1).clamp(max=nz - 1)
    total = torch.zeros_like(keys)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            x, y = cx + dx, cy + dy
            ok = (x >= 0) & (x < nx) & (y >= 0) & (y < ny)
            base = (x.clamp(0, nx - 1) << 42) | (y.clamp(0, ny - 1) << 21)
            lo = torch.searchsorted(keys, base | z0)
            hi = torch.searchsorted(keys, (base | z1) + 1)
            total += torch.where(ok, hi - lo, torch.zeros_like(lo))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--outliers", type=float, default=0.02)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--scipy-k", type=int, nargs="*", default=[16])
    ap.add_argument("--cells", type=int, nargs="+", default=[1, 2, 3, 4], help="grid pitches to compare: cells per radius")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_filter_microbench.jsonl"))
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import _lib, cloud_filter as CF, fusion
    depths, K, E, _ = make_scan(args.views, args.height, args.width)
    dev = torch.device("cuda:0")
    pts, _ = fusion.fuse_depth_maps(torch.from_numpy(depths).to(dev), K, E)
    fused = pts.cpu().numpy()
    rng = np.random.default_rng(0)
    lo, hi = fused.min(axis=0), fused.max(axis=0)
    mid, half = (lo + hi) / 2.0, float((hi - lo).max()) / 2.0
    n_out = int(round(args.outliers * len(fused)))
    data_np = np.concatenate([fused, rng.uniform(mid - half, mid + half, (n_out, 3)).astype(np.float32)])
    n = len(data_np)
    data = torch.from_numpy(data_np).to(dev)
    colors = torch.from_numpy(rng.integers(0, 256, (n, 3), dtype=np.uint8)).to(dev)
    normals = torch.nn.functional.normalize(torch.randn((n, 3), device=dev, generator=torch.Generator(dev).manual_seed(0)), dim=1)
    R, runs = args.radius, args.runs
    scan = {"views": args.views, "height": args.height, "width": args.width, "outlier_share": args.outliers, "points": n,
            "runs": runs}
    lines = []

    def emit(case, **values):
        line = dict(case=case, **scan)
        line.update(values)
        lines.append(line)
        print(json.dumps(line), flush=True)

    # ---- the searches, per grid pitch: what a thread walks, the grid build and the search apart
    tree = None
    if not args.no_scipy and args.scipy_k:
        from scipy.spatial import cKDTree
        p64 = data_np.astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(p64)
        tree_ms = (time.perf_counter() - t0) * 1e3
    R32 = np.float32(R)
    reference = {}
    for cells in args.cells:
        default = cells == CF.CELLS_PER_RADIUS
        grid_ms, grid = event_ms(lambda: CF._search_grid(data, R32, cells=cells), runs)
        cand = candidates_per_point(grid)
        info = {"cells_per_radius": cells, "default": default, "grid_build_ms": grid_ms, "grid_edge": grid.edge,
                "grid_cells": grid.cells, "candidates_27_cells_mean": float(cand.double().mean()),
                "candidates_27_cells_max": int(cand.max())}
        for k in (8, 16, 32):
            mean = torch.empty((n,), dtype=torch.float32, device=dev)
            count = torch.empty((n,), dtype=torch.int32, device=dev)
            search_ms, _ = event_ms(lambda: CF._knn_stats(grid, R32, k, mean, count), runs)
            if k not in reference:
                reference[k] = (mean, count)
            extra = {"equals_first_pitch_bit_for_bit": bool(torch.equal(mean, reference[k][0]) and
                                                            torch.equal(count, reference[k][1])),
                     "points_with_k_neighbours": int((count == k).sum()), "mean_of_m": float(mean.double().mean())}
            if default:
                extra["call_ms"], m = event_ms(lambda: CF.knn_mean_distances(data, R, k), runs)
                extra["call_equals_search"] = bool(torch.equal(m, mean))
                if tree is not None and k in args.scipy_k:
                    t0 = time.perf_counter()
                    tree.query(p64, k=k + 1, distance_upper_bound=float(R32), workers=16)
                    extra.update(scipy_build_ms=tree_ms, scipy_query_ms=(time.perf_counter() - t0) * 1e3, scipy_runs=1,
                                 scipy_workers=16)
            emit("knn", k=k, radius=R, search_ms=search_ms, **dict(info, **extra))
    radius_ms, keep = event_ms(lambda: CF.radius_outlier_mask(data, R, 4), runs)
    emit("radius", min_neighbors=4, radius=R, call_ms=radius_ms, cells_per_radius=CF.CELLS_PER_RADIUS, kept=int(keep.sum()))

    # ---- the voxel merge
    bare_ms, bare = event_ms(lambda: CF.voxel_downsample(data, args.voxel), runs)
    full_ms, full = event_ms(lambda: CF.voxel_downsample(data, args.voxel, colors, normals, return_inverse=True), runs)
    timer = _lib.KernelTimer()
    _lib.set_timer(timer)
    CF.voxel_downsample(data, args.voxel, colors, normals, return_inverse=True)
    _lib.set_timer(None)
    torch.cuda.synchronize()
    kernels = {name: e0.elapsed_time(e1) for name, e0, e1, _, _, _ in timer.records}

    inv = float(np.float32(1.0) / np.float32(args.voxel))
    origin = data.amin(dim=0)

    def torch_route():
        c = torch.floor((data - origin) * inv).long()
        key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
        uniq, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
        m = uniq.numel()
        pos = torch.zeros((m, 3), dtype=torch.float32, device=dev).index_add_(0, inverse, data) / counts[:, None]
        col = torch.zeros((m, 3), dtype=torch.float32, device=dev).index_add_(0, inverse, colors.float()) / counts[:, None]
        nrm = torch.nn.functional.normalize(torch.zeros((m, 3), dtype=torch.float32, device=dev).index_add_(0, inverse, normals),
                                            dim=1)
        return pos, col.round().to(torch.uint8), nrm, inverse

    torch_ms, via_torch = event_ms(torch_route, runs)
    same_rows = via_torch[0].shape == full[0].shape and bool(torch.equal(via_torch[3], full[3]))
    emit("voxel", voxel=args.voxel, rows=int(full[0].shape[0]), call_ms_points_only=bare_ms,
         call_ms_colours_normals_inverse=full_ms, kernels_ms_one_run=kernels, torch_only_ms=torch_ms,
         points_only_equals_full=bool(torch.equal(bare[0], full[0])), torch_only_same_rows=same_rows,
         torch_only_max_position_difference=float((via_torch[0] - full[0]).abs().max()) if same_rows else None)

    # ---- the whole cleaning
    clean = dict(voxel=args.voxel, max_radius=R, k=16, std_ratio=2.0, min_neighbors=4)
    CF.clean_cloud(data, colors, normals, **clean)
    torch.cuda.synchronize()
    walls = []
    for _ in range(runs):
        t0 = time.perf_counter()
        report = CF.clean_cloud(data, colors, normals, **clean)[3]
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    emit("clean", clean_ms_median=median(walls), clean_ms_all=walls, report=report, **clean)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
