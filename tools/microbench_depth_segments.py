"""Time the depth-map segments, the speckle removal and the gap filling (pointmvsnet_amd/depth_segments.py,
csrc/depth_segments.hip) on the synthetic scan of 49 views at 640 x 480 and at 1600 x 1152.  Meant to be run on the MI355X.

    python tools/microbench_depth_segments.py [--views 49] [--runs 5] [--sizes 480x640 1152x1600] [--cases scan plane percolation]
                                              [--host-max-pixels 20000000]

Three inputs per size.  ``scan``: the depth maps of tools/microbench_fusion.py (a 7 x 7 grid of cameras facing a tilted plane,
depth noise 0.3) with planted speckles -- 0.5 % of the pixels in islands of 5 to 80 pixels at 0.8 times their depth -- and
planted pin-holes, 1 % of the pixels in horizontal runs of 1 to 3.  ``plane``: every view one smooth plane, one segment per
view: the size-counting hub.  ``percolation``: a constant depth on a site-percolation mask at p = 0.59: tortuous segments,
the most merge work.  One JSON line per size and input: every kernel under HIP events (per call, the merge and compress
launches summed over the rounds; median of the runs after a warm-up), the whole calls under HIP events and on the wall
clock, the number of rounds, the border edges per view and how many of them united two pieces, the tile size of the library
that ran (``PF_LIB_PATH`` selects another build of it), and GB/s of the algorithmic bytes of the tile kernel (depth in, label
and piece count out: 12 bytes per pixel).  For orientation only, a host route on the same link graph:
``scipy.sparse.csgraph.connected_components`` (inputs of at most ``--host-max-pixels`` pixels; the graph's construction is
timed apart).  The lines are printed and appended to ``profiles/depth_segments_microbench.jsonl``.  No ratio is a claim.
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

ENTRIES = {"pf_depth_tile_segments_f32": "tile_ms", "pf_depth_border_merge_f32": "merge_ms", "pf_depth_label_compress": "compress_ms",
           "pf_depth_segment_sizes": "sizes_ms", "pf_depth_speckle_mask_f32": "mask_ms", "pf_depth_gap_fill_f32": "gap_fill_ms"}


def _commit():
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def _median(values):
    return sorted(values)[len(values) // 2]


def _timed(fn, runs):
    """``fn`` under a HIP event pair and on the wall clock: (event ms per run, wall ms per run), after a warm-up."""
    fn()
    torch.cuda.synchronize()
    events, walls = [], []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        events.append(e0.elapsed_time(e1))
    return events, walls


def _kernels(fn, runs):
    """HIP-event time of every C-ABI entry inside ``fn``, summed per call: ({entry: [ms per run]}, event floor)."""
    from pointmvsnet_amd import _lib
    fn()
    torch.cuda.synchronize()
    sums, floor = {}, None
    for _ in range(runs):
        timer = _lib.KernelTimer()
        _lib.set_timer(timer)
        try:
            fn()
        finally:
            _lib.set_timer(None)
        floor = next(iter(timer.summary().values()))["event_floor_ms"]        # synchronises
        run = {}
        for name, e0, e1, _, _, _ in timer.records:
            run[name] = run.get(name, 0.0) + e0.elapsed_time(e1)
        for name, ms in run.items():
            sums.setdefault(name, []).append(ms)
    return sums, floor


def plant(depths, seed=0, speckle_share=0.005, hole_share=0.01):
    """Speckles and pin-holes planted into (V, h, w) depths, in place: (speckle pixels, hole pixels)."""
    rng = np.random.default_rng(seed)
    V, h, w = depths.shape
    speckles = holes = 0
    for v in range(V):
        target, done = int(speckle_share * h * w), 0
        while done < target:
            k = int(rng.integers(5, 81))
            side = int(np.ceil(np.sqrt(k)))
            y0, x0 = int(rng.integers(0, h - side)), int(rng.integers(0, w - side))
            yy, xx = np.divmod(np.arange(k), side)
            depths[v, y0 + yy, x0 + xx] *= np.float32(0.8)
            done += k
        speckles += done
        runs = int(hole_share * h * w / 2)
        ys, xs, ls = rng.integers(0, h, runs), rng.integers(0, w - 3, runs), rng.integers(1, 4, runs)
        for length in (1, 2, 3):
            sel = ls >= length
            depths[v, ys[sel], xs[sel] + length - 1] = 0.0
        holes += int((depths[v] == 0).sum())
    return speckles, holes


def make_case(case, V, h, w):
    if case == "scan":
        from microbench_fusion import make_scan
        depths = make_scan(V, h, w)[0]
        speckles, holes = plant(depths)
        return depths, {"planted_speckle_pixels": speckles, "planted_hole_pixels": holes}
    if case == "plane":
        ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
        plane = (600.0 + 0.05 * xs + 0.03 * ys).astype(np.float32)
        return np.broadcast_to(plane, (V, h, w)).copy(), {}
    if case == "percolation":
        rng = np.random.default_rng(1)
        return np.where(rng.random((V, h, w)) < 0.59, np.float32(600.0), np.float32(0.0)).astype(np.float32), {"p": 0.59}
    raise ValueError(case)


def host_route(depths, rel_jump=0.01, depth_min=1e-3, depth_max=1e5):
    """scipy.sparse.csgraph.connected_components on the link graph: (graph ms, components ms, number of segments)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    ok = (depths > np.float32(depth_min)) & (depths < np.float32(depth_max))
    n = depths.size
    index = np.arange(n, dtype=np.int32).reshape(depths.shape)
    rel = np.float32(rel_jump)
    a, b = depths[:, :, :-1], depths[:, :, 1:]
    right = ok[:, :, :-1] & ok[:, :, 1:] & (np.abs(a - b) <= rel * np.minimum(a, b))
    a, b = depths[:, :-1, :], depths[:, 1:, :]
    down = ok[:, :-1, :] & ok[:, 1:, :] & (np.abs(a - b) <= rel * np.minimum(a, b))
    rows = np.concatenate([index[:, :, :-1][right], index[:, :-1, :][down]])
    cols = np.concatenate([index[:, :, 1:][right], index[:, 1:, :][down]])
    graph = coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(n, n)).tocsr()
    t1 = time.perf_counter()
    count, comp = connected_components(graph, directed=False)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(count - (~ok).sum()), comp, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--sizes", nargs="+", default=["480x640", "1152x1600"], help="HEIGHTxWIDTH of the depth maps")
    ap.add_argument("--cases", nargs="+", default=["scan", "plane", "percolation"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-size", type=int, default=100)
    ap.add_argument("--max-gap", type=int, default=7)
    ap.add_argument("--host-max-pixels", type=int, default=20000000, help="the host route runs on inputs up to this size (0: never)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_segments_microbench.jsonl"))
    args = ap.parse_args()
    from pointmvsnet_amd import _lib, build
    from pointmvsnet_amd import depth_segments as DS
    dev = torch.device("cuda:0")
    V = args.views
    usage = None
    try:
        with open(build.USAGE_FILE) as f:
            usage = {name.split("_kernel")[0].split("depth_")[-1]: {k: u[k] for k in ("vgprs", "sgprs", "scratch_bytes_per_lane")}
                     for name, u in json.load(f)["depth_segments.hip"].items() if "depth_" in name}
    except (OSError, ValueError, KeyError):
        pass
    tw, th = DS.tile_size()
    lines = []
    for size in args.sizes:
        h, w = (int(v) for v in size.split("x"))
        for case in args.cases:
            depths, extra = make_case(case, V, h, w)
            d_dev = torch.from_numpy(depths).to(dev)
            n = V * h * w
            line = dict(extra, bench="depth_segments", case=case, views=V, height=h, width=w, tile_w=tw, tile_h=th, runs=args.runs,
                        min_size=args.min_size, max_gap=args.max_gap, commit=_commit(), device=torch.cuda.get_device_name(0),
                        library=os.path.basename(_lib.LIB_PATH), resource_usage=usage)
            calls = {"segments_with_sizes": lambda: DS.depth_segments(d_dev, return_sizes=True),
                     "remove_speckles": lambda: DS.remove_speckles(d_dev, args.min_size),
                     "fill_gaps": lambda: DS.fill_gaps(d_dev, args.max_gap),
                     "clean_depth_maps": lambda: DS.clean_depth_maps(d_dev, min_size=args.min_size, max_gap=args.max_gap)}
            sums, floor = _kernels(calls["clean_depth_maps"], args.runs)
            for entry, key in ENTRIES.items():
                if entry in sums:
                    line[key] = _median(sums[entry])
            line["event_floor_ms"] = floor
            line["tile_gbytes_per_s"] = 12.0 * n / line["tile_ms"] / 1e6
            for name, fn in calls.items():
                events, walls = _timed(fn, args.runs)
                line[name + "_event_ms"], line[name + "_wall_ms"] = _median(events), _median(walls)
            out, report = calls["clean_depth_maps"]()
            line["report"] = report
            labels = DS.depth_segments(d_dev)
            line.update({k: v for k, v in DS.last_segment_stats().items()})
            line["two_calls_equal"] = bool(torch.equal(labels, DS.depth_segments(d_dev)))
            if args.host_max_pixels and n <= args.host_max_pixels:
                try:
                    graph_ms, comp_ms, segments, comp, ok = host_route(depths)
                except ImportError:
                    pass
                else:
                    lab = labels.cpu().numpy().reshape(-1)
                    first = np.full(comp.max() + 1, n, dtype=np.int64)
                    np.minimum.at(first, comp, np.arange(n))
                    line.update(host_graph_ms=graph_ms, host_components_ms=comp_ms, host_segments=segments,
                                host_labels_equal=bool(np.array_equal(np.where(ok.reshape(-1), first[comp], -1), lab)))
                    del comp, ok, lab, first
            lines.append(line)
            print(json.dumps(line), flush=True)
            del d_dev, labels, out
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
