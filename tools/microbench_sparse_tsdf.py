"""Time the sparse TSDF volume (pointmvsnet_amd/sparse_tsdf.py, csrc/sparse_tsdf.hip) on the scan of tools/microbench_tsdf.py.

    python tools/microbench_sparse_tsdf.py [--views 49] [--height 480] [--width 640] [--voxels 1.0 0.5 0.25 0.125] [--runs 5]
                                           [--dense-max-samples 100000000]

The 49-view 640 x 480 synthetic scan (a tilted plane at depth 600, noise 0.3, random colours), the volume ``volume_bounds`` of
it grown by ``trunc = 4 voxel``, with colour, ``min_weight`` 2: what ``microbench_tsdf.py`` meshes through the dense volume.
Per voxel size every C-ABI entry is timed on its own (HIP events around the call on its stream, ``_lib.KernelTimer``; one
warm-up run, then the median of ``--runs``): touch, neighbours, integrate, count, emit, vertices; next to them the whole
``allocate + integrate + extract`` call (events around the Python calls, ended by a synchronisation; it includes torch's
nonzero, cumsum and sorted unique, the accessors and the host synchronisations).  ``allocated_bricks`` of
``virtual_bricks`` and ``state_bytes`` against the dense ``24 nx ny nz`` come from ``report()``.  Where the grid has at most
``--dense-max-samples`` samples the dense route runs next to it, ``TSDFVolume.integrate + extract`` timed the same way, and
``mesh_equal`` says whether vertices, colours and keys are the dense ones byte for byte and the faces the same rows.
Prints one JSON line per voxel size and appends it to profiles/sparse_tsdf_microbench.jsonl.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

KERNELS = {"touch": "pf_sparse_tsdf_touch", "neighbours": "pf_sparse_tsdf_neighbours", "integrate": "pf_sparse_tsdf_integrate_f32",
           "count": "pf_sparse_tsdf_count_triangles", "emit": "pf_sparse_tsdf_emit_triangles",
           "vertices": "pf_sparse_tsdf_vertices_f32"}


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), res


def sorted_rows(faces):
    rows = faces.to(torch.int64)
    first = rows.argmin(dim=1, keepdim=True)                                        # the rotation of a face is free
    rows = torch.gather(rows, 1, (first + torch.arange(3, device=rows.device)) % 3)
    for column in (2, 1, 0):                                                        # three stable sorts: lexicographic
        rows = rows[torch.argsort(rows[:, column], stable=True)]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--voxels", type=float, nargs="+", default=[1.0, 0.5, 0.25, 0.125])
    ap.add_argument("--min-weight", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dense-max-samples", type=int, default=100000000)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import _lib, sparse_tsdf, tsdf
    V, h, w = args.views, args.height, args.width
    depths_np, K, E, images_np = make_scan(V, h, w)
    dev = torch.device(args.device)
    depths, images = torch.from_numpy(depths_np).to(dev), torch.from_numpy(images_np).to(dev)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for voxel in args.voxels:
        trunc = 4.0 * voxel
        origin, dims = tsdf.dims_for(tsdf.volume_bounds(depths, K, E, pad=trunc), voxel,
                                     max_samples=sparse_tsdf.MAX_VIRTUAL_SAMPLES)
        samples = dims[0] * dims[1] * dims[2]

        def sparse_route():
            vol = sparse_tsdf.SparseTSDFVolume(origin, voxel, dims, trunc, with_colour=True, device=dev)
            vol.allocate(depths, K, E)
            vol.integrate(depths, K, E, images=images)
            return vol, vol.extract(args.min_weight)

        timer = _lib.KernelTimer()
        _lib.set_timer(timer)
        whole_ms = []
        for run in range(args.runs + 1):                                            # the first is the warm-up
            vol = mesh = None                                                       # free the run before
            ms, (vol, mesh) = event_ms(sparse_route)
            whole_ms.append(ms)
        _lib.set_timer(None)
        torch.cuda.synchronize()
        kernels = {}
        for name, e0, e1, _, _, _ in timer.records:
            kernels.setdefault(name, []).append(e0.elapsed_time(e1))
        out = {"views": V, "height": h, "width": w, "voxel": voxel, "trunc": trunc, "dims": list(dims), "samples": samples,
               "runs": args.runs, "min_weight": args.min_weight, "with_colour": True}
        out.update(vol.report())
        out["state_share"] = out["state_bytes"] / float(out["dense_state_bytes"])
        for short, name in KERNELS.items():
            out[short + "_kernel_ms"] = median(kernels[name][1:]) if len(kernels.get(name, [])) > 1 else None
        out.update(sparse_call_ms=median(whole_ms[1:]), vertices=int(mesh[0].shape[0]), faces=int(mesh[1].shape[0]),
                   peak_memory_bytes=int(torch.cuda.max_memory_allocated(dev)))
        if samples <= args.dense_max_samples:
            def dense_route():
                d = tsdf.TSDFVolume(origin, voxel, dims, trunc, with_colour=True, device=dev)
                d.integrate(depths, K, E, images=images)
                return d.extract(args.min_weight)

            dense_ms = []
            for run in range(args.runs + 1):
                dense_mesh = None
                ms, dense_mesh = event_ms(dense_route)
                dense_ms.append(ms)
            equal = all(torch.equal(mesh[c], dense_mesh[c]) for c in (0, 2, 3)) and \
                torch.equal(sorted_rows(mesh[1]), sorted_rows(dense_mesh[1]))
            out.update(dense_call_ms=median(dense_ms[1:]), mesh_equal=bool(equal))
            dense_mesh = None
        vol = mesh = None
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        line = json.dumps(out)
        print(line, flush=True)
        with open(os.path.join(ROOT, "profiles", "sparse_tsdf_microbench.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
