"""Time the batched confidence filter (pointmvsnet_amd/scan.py) on a DTU scan's worth of predictions: 49 views, the four
interpolation modes, at the flow / coarse map sizes of BASELINE cfg 2 and cfg 5 (taken from ``synthetic.make_config``).

    python tools/microbench_scan_filter.py [--views 49] [--configs cfg2 cfg5] [--runs 20] [--file-runs 3]

Per size and mode: the kernel (HIP events around the launch, median after warm-up, with its algorithmic bytes -> GB/s) and
the whole ``filter_depth_maps`` call (wall clock around a device synchronisation: tables, uploads, launch).  Baseline per
size: the file route for the same data -- ``probability_filter(..., "NEAREST")`` over the PFM files (three ``load_pfm``
and one ``write_pfm`` per view) plus the ``load_pfm`` / stack / upload with which ``fuse_scene_folder`` reads them back.
Prints one JSON line and appends it to profiles/scan_filter_microbench.jsonl.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(vals):
    return sorted(vals)[len(vals) // 2]


def sizes_of(cfg):
    """(flow map size, coarse map size) of a configuration: the last image scale and the 1/8 coarse grid."""
    from pointmvsnet_amd import synthetic
    H, W = synthetic.CONFIGS[cfg][:2]
    _, img_scales, _ = synthetic.make_config(cfg)
    return (int(H * img_scales[-1]), int(W * img_scales[-1])), (H // 8, W // 8)


def file_route(folder, V, dev, runs):
    from pointmvsnet_amd.utils import eval_file_logger as EL
    from pointmvsnet_amd.utils.io import load_pfm
    filt, load = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        EL.probability_filter(folder, 0.2, 0.1, "flow", V, "NEAREST")
        t1 = time.perf_counter()
        maps = [np.ascontiguousarray(load_pfm(os.path.join(folder, "%08d_flow_prob_filtered.pfm" % v))[0], dtype=np.float32)
                for v in range(V)]
        torch.from_numpy(np.stack(maps)).to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        filt.append((t1 - t0) * 1e3)
        load.append((t2 - t1) * 1e3)
    return median(filt), median(load)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--configs", nargs="+", default=["cfg2", "cfg5"])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--file-runs", type=int, default=3)
    args = ap.parse_args()
    from pointmvsnet_amd import _lib, scan
    from pointmvsnet_amd.utils import eval_file_logger as EL
    from pointmvsnet_amd.utils.io import write_pfm
    dev = torch.device("cuda:0")
    V = args.views
    out = {"views": V, "runs": args.runs, "device": torch.cuda.get_device_name(0), "cases": []}
    for cfg in args.configs:
        (h, w), (ih, iw) = sizes_of(cfg)
        g = torch.Generator().manual_seed(0)
        depths = 400.0 + 300.0 * torch.rand(V, h, w, generator=g)
        flow = torch.rand(V, 5, h, w, generator=g) ** 2
        flow = flow / flow.sum(dim=1, keepdim=True)
        init = torch.rand(V, ih, iw, generator=g)
        case = {"config": cfg, "flow_size": [h, w], "coarse_size": [ih, iw], "modes": {}}
        d, f, i = depths.to(dev), flow.to(dev), init.to(dev)
        for mode in ("NEAREST", "BILINEAR", "CUBIC", "LANCZOS4"):
            for _ in range(args.warmup):
                scan.filter_depth_maps(d, f, i, mode=mode)
            torch.cuda.synchronize()
            walls = []
            timer = _lib.KernelTimer(only="pf_scan_filter_f32")
            _lib.set_timer(timer)
            for _ in range(args.runs):
                t0 = time.perf_counter()
                scan.filter_depth_maps(d, f, i, mode=mode)
                torch.cuda.synchronize()
                walls.append((time.perf_counter() - t0) * 1e3)
            _lib.set_timer(None)
            floor = timer.summary()["pf_scan_filter_f32"]["event_floor_ms"]
            ms = median([e0.elapsed_time(e1) for _, e0, e1, _, _, _ in timer.records])
            nbytes = timer.records[0][3]
            case["modes"][mode] = {"kernel_ms_median": ms, "algo_mbytes": nbytes / 1e6, "gbytes_per_s": nbytes / ms / 1e6,
                                   "call_ms_median": median(walls), "event_floor_ms": floor}
        with tempfile.TemporaryDirectory() as folder:
            for v in range(V):
                write_pfm(os.path.join(folder, "%08d_flow.pfm" % v), depths[v].numpy())
                write_pfm(os.path.join(folder, "%08d_flow_prob.pfm" % v),
                          EL.flow_confidence_np(flow[v].permute(1, 2, 0).numpy()))
                write_pfm(os.path.join(folder, "%08d_init_prob.pfm" % v), init[v].numpy())
            filt, load = file_route(folder, V, dev, args.file_runs)
        case["file_route"] = {"probability_filter_ms_median": filt, "load_stack_upload_ms_median": load, "runs": args.file_runs}
        out["cases"].append(case)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "scan_filter_microbench.jsonl"), "a") as fjson:
        fjson.write(line + "\n")


if __name__ == "__main__":
    main()
