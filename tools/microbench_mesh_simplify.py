"""Time mesh simplification (pointmvsnet_amd/mesh_simplify.py, csrc/mesh_simplify.hip) on DTU-sized TSDF meshes.

    python tools/microbench_mesh_simplify.py [--views 49] [--height 480] [--width 640] [--voxels 1.0 0.5] [--sparse-voxels 0.25]
                                             [--cells 2 4 8] [--thresholds 0 4 8 16 32 64 128 256 1024 -1] [--runs 5]
                                             [--no-orientation] [--no-quality]

The meshes are ``TSDFVolume.extract`` of the 49-view 640 x 480 synthetic scan of tools/microbench_tsdf.py (a tilted plane at
depth 600, noise 0.3) at every ``--voxels`` pitch and ``SparseTSDFVolume.extract`` at every ``--sparse-voxels`` pitch (skipped
with a note when the device runs out of memory).  Per mesh and per cell of ``--cells`` voxels, after one warm-up, the median
of ``--runs`` of HIP-event times (events on the stream around the step, ended by a synchronisation):

* the whole ``simplify_mesh`` call for ``"quadric"`` and for ``"mean"``;
* every step apart: ``clusters`` (the key kernel, torch's stable sort, the reduce kernel), ``faces`` (the remap and
  classification kernel), ``duplicates`` (torch's two stable sorts and the keep-first kernel), ``corner_table`` (torch's
  stable sort and searchsorted), ``quadric`` (both kernels and the ``nonzero`` that lists the long clusters) and ``compaction``
  (torch's nonzero, cumsum and gathers);
* the quadric kernels alone (event pairs around each launch, ``_lib.KernelTimer``) at every threshold of ``--thresholds``
  between the thread-per-cluster and the wave-per-cluster path (0: every cluster gets a wave; -1: every cluster gets a
  thread), with the number of clusters and corners on each side: ``mesh_simplify.WAVE_MIN_CORNERS`` is chosen from this.

For orientation, unless ``--no-orientation``: a torch-only mean-placement route on the same GPU (``torch.unique`` of the
cell keys, three ``index_add_`` calls in float32 whose atomics sum in no fixed order, ``torch.unique`` of the sorted cluster
triples) -- a yardstick for time and not for bits.  Quality, unless ``--no-quality``, through existing code:
``point_mesh_distances`` from the input vertices to the simplified surface, mean and largest in cells, for both
placements, and ``mesh_edge_counts`` before and after.
Prints one JSON line per mesh and cell and appends it to profiles/mesh_simplify_microbench.jsonl.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), res


def torch_mean_route(vertices, faces, cell):
    """Vertex clustering with library operators: float32 means by index_add_, unique triples; (vertices, faces)."""
    lo = vertices.amin(dim=0)
    c = torch.floor((vertices - lo) * (1.0 / cell)).long()
    keys = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    uniq, cluster, counts = torch.unique(keys, return_inverse=True, return_counts=True)
    total = torch.zeros((uniq.numel(), 3), dtype=torch.float32, device=vertices.device)
    total.index_add_(0, cluster, vertices)
    means = total / counts[:, None].float()
    triple = cluster[faces.long()]
    alive = (triple[:, 0] != triple[:, 1]) & (triple[:, 1] != triple[:, 2]) & (triple[:, 0] != triple[:, 2])
    triple = triple[alive]
    asc = torch.sort(triple, dim=1)[0]
    _, first = torch.unique(asc, dim=0, return_inverse=True)
    keep = torch.zeros((triple.shape[0],), dtype=torch.bool, device=vertices.device)
    order = torch.sort(first, stable=True)[1]
    run_start = torch.ones_like(keep)
    run_start[1:] = first[order][1:] != first[order][:-1]
    keep[order[run_start]] = True
    kept = triple[keep]
    used = torch.zeros((uniq.numel(),), dtype=torch.bool, device=vertices.device)
    used[kept.reshape(-1)] = True
    remap = torch.cumsum(used, dim=0) - 1
    return means[used], remap[kept]


def steps_apart(ms, cf, vertices, faces32, cell, reg):
    """One pass of ``simplify_mesh`` taken apart, every step between events: {step: ms} and the pieces."""
    dev, Nv = vertices.device, int(vertices.shape[0])
    inv = cf._voxel_inverse(cell, "microbench", "cell")
    lo, cells = cf._voxel_cells(vertices, inv, "microbench")
    t = {}
    t["clusters"], (means, _, _, _, cluster, _) = event_ms(lambda: cf._voxel_reduce(vertices, lo, inv, cells, None, None, True))
    M = int(means.shape[0])
    t["faces"], (triple, ascending, collapsed) = event_ms(lambda: ms._classify_faces(faces32, Nv, cluster, M))

    def duplicates():
        survivors = torch.nonzero(collapsed == 0).view(-1)
        return ms._keep_first(ascending, ms._sort_by_triple(ascending, survivors, M))

    t["duplicates"], keep = event_ms(duplicates)
    t["corner_table"], (offsets, corners) = event_ms(lambda: ms._cluster_corner_table(triple, M))
    t["quadric"], (positions, fallback) = event_ms(
        lambda: ms._quadric_positions(vertices, faces32, offsets, corners, means, np.float32(cell), reg))

    def compaction():
        source = torch.nonzero(keep).view(-1)
        kept = triple[source].long()
        used = torch.zeros((M,), dtype=torch.bool, device=dev)
        used[kept.reshape(-1)] = True
        remap = torch.where(used, torch.cumsum(used, dim=0, dtype=torch.int64) - 1, torch.full((M,), -1, dtype=torch.int64, device=dev))
        return positions[used], remap[kept].to(torch.int32), remap[cluster]

    t["compaction"], _ = event_ms(compaction)
    return t, (means, offsets, corners)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--voxels", type=float, nargs="*", default=[1.0, 0.5])
    ap.add_argument("--sparse-voxels", type=float, nargs="*", default=[0.25])
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0, 8.0], help="cell edges in voxels")
    ap.add_argument("--thresholds", type=int, nargs="+", default=[0, 4, 8, 16, 32, 64, 128, 256, 1024, -1])
    ap.add_argument("--min-weight", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-orientation", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import _lib, cloud_filter, mesh_simplify, sparse_tsdf, tsdf
    from pointmvsnet_amd.mesh_distance import point_mesh_distances
    V, h, w = args.views, args.height, args.width
    depths_np, K, E, images_np = make_scan(V, h, w)
    dev = torch.device(args.device)
    depths, images = torch.from_numpy(depths_np).to(dev), torch.from_numpy(images_np).to(dev)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    reg = 1e-3
    for voxel, sparse in [(v, False) for v in args.voxels] + [(v, True) for v in args.sparse_voxels]:
        trunc = 4.0 * voxel
        try:
            origin, dims = tsdf.dims_for(tsdf.volume_bounds(depths, K, E, pad=trunc), voxel,
                                         max_samples=sparse_tsdf.MAX_VIRTUAL_SAMPLES if sparse else None)
            vol = (sparse_tsdf.SparseTSDFVolume if sparse else tsdf.TSDFVolume)(origin, voxel, dims, trunc, with_colour=True,
                                                                                device=dev)
            vol.integrate(depths, K, E, images=images)
            vertices, faces, colours = vol.extract(args.min_weight)[:3]
            del vol
        except torch.cuda.OutOfMemoryError as exc:
            print(json.dumps({"voxel": voxel, "sparse": sparse, "skipped": "out of memory: %s" % str(exc)[:80]}), flush=True)
            continue
        torch.cuda.empty_cache()
        nv, nf = int(vertices.shape[0]), int(faces.shape[0])
        faces32 = faces.to(torch.int32).contiguous()
        edges_before = None if args.no_quality else mesh_simplify.mesh_edge_counts(faces)
        for cell_voxels in args.cells:
            cell = float(np.float32(cell_voxels * voxel))
            calls = {"quadric": [], "mean": []}
            steps = {}
            for run in range(args.runs + 1):                        # the first is the warm-up
                for placement in ("quadric", "mean"):
                    ms, res = event_ms(lambda: mesh_simplify.simplify_mesh(vertices, faces, cell, colours=colours,
                                                                           placement=placement, return_maps=True))
                    calls[placement].append(ms)
                    if placement == "quadric":
                        simplified = res
                t, (means, offsets, corners) = steps_apart(mesh_simplify, cloud_filter, vertices, faces32, cell, reg)
                for k, v in t.items():
                    steps.setdefault(k, []).append(v)
            rep = simplified[3]
            lengths = offsets[1:] - offsets[:-1]
            out = {"views": V, "height": h, "width": w, "voxel": voxel, "sparse": sparse, "dims": list(dims), "vertices": nv,
                   "faces": nf, "cell_voxels": cell_voxels, "cell": cell, "runs": args.runs, "report": rep,
                   "wave_min_corners": mesh_simplify.WAVE_MIN_CORNERS,
                   "corners_per_cluster_mean": float(lengths.float().mean()), "corners_per_cluster_max": int(lengths.max()),
                   "quadric_call_ms": median(calls["quadric"][1:]), "mean_call_ms": median(calls["mean"][1:])}
            out.update({k + "_ms": median(v[1:]) for k, v in steps.items()})
            sweep = []
            for threshold in args.thresholds:
                limit = int(lengths.max()) + 1 if threshold < 0 else threshold
                timer = _lib.KernelTimer()
                _lib.set_timer(timer)
                for run in range(args.runs + 1):
                    mesh_simplify._quadric_positions(vertices, faces32, offsets, corners, means, np.float32(cell), reg, threshold=limit)
                _lib.set_timer(None)
                torch.cuda.synchronize()
                per = {}
                for name, e0, e1, _, _, _ in timer.records:
                    per.setdefault(name, []).append(e0.elapsed_time(e1))
                long_ = lengths >= limit
                sweep.append({"threshold": threshold, "wave_clusters": int(long_.sum()), "wave_corners": int(lengths[long_].sum()),
                              "thread_kernel_ms": median(per["pf_mesh_quadric_thread_f64"][1:]) if "pf_mesh_quadric_thread_f64" in per else 0.0,
                              "wave_kernel_ms": median(per["pf_mesh_quadric_wave_f64"][1:]) if "pf_mesh_quadric_wave_f64" in per else 0.0})
                sweep[-1]["kernels_ms"] = sweep[-1]["thread_kernel_ms"] + sweep[-1]["wave_kernel_ms"]
            out["threshold_sweep"] = sweep
            if not args.no_orientation:
                torch_mean_route(vertices, faces, cell)
                times = []
                for _ in range(args.runs):
                    ms, ref = event_ms(lambda: torch_mean_route(vertices, faces, cell))
                    times.append(ms)
                out.update(torch_mean_route_ms=median(times), torch_mean_route_vertices=int(ref[0].shape[0]),
                           torch_mean_route_faces=int(ref[1].shape[0]))
            if not args.no_quality:
                out["edges_before"], out["edges_after"] = edges_before, mesh_simplify.mesh_edge_counts(simplified[1])
                for placement in ("quadric", "mean"):
                    res = simplified if placement == "quadric" else mesh_simplify.simplify_mesh(
                        vertices, faces, cell, placement="mean", return_maps=True)
                    if res[1].shape[0]:
                        mapped = vertices[res[4] >= 0]
                        dist = point_mesh_distances(mapped, res[0], res[1], max_dist=8.0 * cell)
                        out["distance_%s_mean_cells" % placement] = float(dist.double().mean()) / cell
                        out["distance_%s_max_cells" % placement] = float(dist.max()) / cell
            line = json.dumps(out)
            print(line, flush=True)
            with open(os.path.join(ROOT, "profiles", "mesh_simplify_microbench.jsonl"), "a") as f:
                f.write(line + "\n")
        del vertices, faces, colours, faces32


if __name__ == "__main__":
    main()
