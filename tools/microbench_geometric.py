"""Time the round-trip geometric consistency filter (pointmvsnet_amd/geometric.py) on a DTU-sized scan: 49 views of
640 x 480, once against all other views and once against ``--num-src`` sources per view.

    python tools/microbench_geometric.py [--views 49] [--height 480] [--width 640] [--num-src 10] [--runs 20]

The scan is that of tools/microbench_fusion.py (a 7 x 7 grid of cameras facing a tilted plane, so every view overlaps most
of the others and the gathers really happen).  The ``num_src`` sources of a view are its nearest camera centres, nearest
first, as ``Cameras/pair.txt`` would list them.  Per configuration one JSON line, printed and appended to
``profiles/geometric_microbench.jsonl``: the whole call (matrix composition on the host, uploads, the kernel, prefix sum,
compaction; median of the runs, wall clock around a device synchronisation), the kernel alone (HIP events, with its
algorithmic bytes -> GB/s) and, for orientation only, ``fuse_depth_maps`` on the same maps in the same process (a
different algorithm with a different output: no ratio between the two is a claim).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def nearest_sources(E, num_src):
    """(V, num_src) int32: every view's nearest camera centres, nearest first (-1 pads when there are fewer views)."""
    C = np.stack([-np.linalg.inv(e[:3, :3]) @ e[:3, 3] for e in E])
    V = C.shape[0]
    table = np.full((V, num_src), -1, np.int32)
    for i in range(V):
        order = [j for j in np.argsort(np.linalg.norm(C - C[i], axis=1), kind="stable") if j != i][:num_src]
        table[i, :len(order)] = order
    return table


def _commit():
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def _wall(fn, runs):
    fn()                                                                       # warm-up
    torch.cuda.synchronize()
    walls = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return walls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--num-src", type=int, default=10)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometric_microbench.jsonl"))
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import _lib, fusion, geometric
    depths, K, E, images = make_scan(args.views, args.height, args.width)
    dev = torch.device("cuda:0")
    d_dev, i_dev = torch.from_numpy(depths).to(dev), torch.from_numpy(images).to(dev)
    fuse_walls = _wall(lambda: fusion.fuse_depth_maps(d_dev, K, E, images=i_dev), args.runs)
    fuse_points = int(fusion.fuse_depth_maps(d_dev, K, E, images=i_dev)[0].shape[0])
    lines = []
    for label, table in (("all", None), ("num_src", nearest_sources(E, args.num_src))):
        def call():
            return geometric.geometric_filter(d_dev, K, E, images=i_dev, sources=table)
        walls = _wall(call, args.runs)
        timer = _lib.KernelTimer(only="pf_geo_filter_f32")
        _lib.set_timer(timer)
        for _ in range(args.runs):
            out = call()
        _lib.set_timer(None)
        k = timer.summary()["pf_geo_filter_f32"]
        lines.append({
            "bench": "geometric_filter", "sources": label, "sources_per_view": args.views - 1 if table is None else args.num_src,
            "views": args.views, "height": args.height, "width": args.width, "runs": args.runs, "commit": _commit(),
            "points": int(out[3].shape[0]), "kept_share": float(out[1].float().mean()),
            "call_ms_median": sorted(walls)[len(walls) // 2], "call_ms_min": min(walls), "call_ms_max": max(walls),
            "kernel_ms": k["ms"] / k["launches"], "kernel_algo_gbytes": k["bytes"] / k["launches"] / 1e9,
            "kernel_gbytes_per_s": k["bytes"] / k["ms"] / 1e6, "event_floor_ms": k["event_floor_ms"],
            "fuse_depth_maps_ms_median": sorted(fuse_walls)[len(fuse_walls) // 2], "fuse_depth_maps_points": fuse_points})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
