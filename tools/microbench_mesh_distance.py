"""Time the exact point-to-mesh distances (pointmvsnet_amd/mesh_distance.py, csrc/mesh_distance.hip) on a DTU-sized TSDF mesh.

    python tools/microbench_mesh_distance.py [--views 49] [--height 480] [--width 640] [--voxels 1.0 0.5] [--pitch 0.2]
                                             [--outliers 0.02] [--max-dist 20] [--runs 5]

The mesh is ``TSDFVolume.extract`` of the 49-view 640 x 480 synthetic scan of tools/microbench_tsdf.py (a tilted plane at
depth 600, noise 0.3) at every ``--voxels`` pitch.  The queries are the scan's plane sampled at ``--pitch`` over the mesh's
footprint plus ``--outliers`` of that number placed uniformly in the mesh's bounding box stretched to a cube (the far
outliers of tools/microbench_evaluation.py).  Per mesh, after one warm-up, the median of ``--runs`` HIP-event times (events
on the stream around the step, ended by a synchronisation), the steps of ``point_mesh_distances`` timed apart:

* the fine grid's build (count kernel, cumsum, the host's read of the total, emit kernel, torch's stable sort, pack kernel),
  with the count, emit and pack kernels on their own (event pairs around each launch, ``_lib.KernelTimer``);
* the first pass (one thread per query) and the collection of the unfinished queries;
* the coarse grid's build and the second pass (one wave per query);
* the whole call.

It reports the pairs per face of both grids, the number of second-pass queries and the candidates tested per query: the
face records a query's thread (or wave) evaluates, recomputed on the host for a sample of 4096 queries from the sorted
keys exactly as the kernels walk them (the cube of radius 1, again the cube of radius 3 for a query farther than 0.95
cell edges, the 27 coarse cells in the second pass).  For orientation the sampled route on the same input:
``sample_surface`` at ``--pitch`` and ``nearest_distances`` from the queries to the samples, and the difference between
the two completeness means over the queries below the cap on both routes.  Prints one JSON line per voxel size and
appends it to profiles/mesh_distance_microbench.jsonl.
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


def cube_candidates(points, grid, radius, clamp):
    """Per point the number of face records in the cube of ``radius`` cells around its cell, from the sorted keys as the
    kernels find them; the cell arithmetic is float32 as in pf_cloud_grid.h.  ``clamp`` is the kernel's clamp beyond the grid."""
    keys = grid.keys.cpu().numpy()
    o = np.asarray(grid.origin, np.float32)
    edge = np.float32(grid.edge)
    n = np.asarray(grid.cells, np.int64)
    cell = np.floor((points.astype(np.float32) - o) / edge)
    cell = np.clip(cell, -float(clamp + 1), (n + clamp).astype(np.float32)).astype(np.int64)
    total = np.zeros(len(points), np.int64)
    z0, z1 = np.maximum(cell[:, 2] - radius, 0), np.minimum(cell[:, 2] + radius, n[2] - 1)
    for dx in range(-radius, radius + 1):
        for dy in range(-radius, radius + 1):
            x, y = cell[:, 0] + dx, cell[:, 1] + dy
            ok = (x >= 0) & (x < n[0]) & (y >= 0) & (y < n[1]) & (z0 <= z1)
            base = (np.where(ok, x, 0) << 42) | (np.where(ok, y, 0) << 21)
            lo = np.searchsorted(keys, base | np.where(ok, z0, 0), side="left")
            hi = np.searchsorted(keys, base | np.where(ok, z1, 0), side="right")
            total += np.where(ok, hi - lo, 0)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--voxels", type=float, nargs="+", default=[1.0, 0.5])
    ap.add_argument("--min-weight", type=int, default=2)
    ap.add_argument("--pitch", type=float, default=0.2)
    ap.add_argument("--outliers", type=float, default=0.02)
    ap.add_argument("--max-dist", type=float, default=20.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import _lib, evaluation, mesh_distance as D, mesh_ops, tsdf
    V, h, w = args.views, args.height, args.width
    depths_np, K, E, _ = make_scan(V, h, w)
    dev = torch.device(args.device)
    depths = torch.from_numpy(depths_np).to(dev)
    cap = float(np.float32(args.max_dist))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for voxel in args.voxels:
        trunc = 4.0 * voxel
        origin, dims = tsdf.dims_for(tsdf.volume_bounds(depths, K, E, pad=trunc), voxel)
        vol = tsdf.TSDFVolume(origin, voxel, dims, trunc, with_colour=False, device=dev)
        vol.integrate(depths, K, E)
        vertices, faces = vol.extract(args.min_weight)[:2]
        del vol
        vertices = vertices.contiguous()
        nv, nf = int(vertices.shape[0]), int(faces.shape[0])
        # the queries: the scan's plane n . X = n . target at the pitch over the mesh's footprint, and far outliers
        mesh_np = vertices.cpu().numpy().astype(np.float64)
        n = np.array([0.15, -0.1, 1.0])
        n /= np.linalg.norm(n)
        target = np.array([0.0, 0.0, 600.0])
        u = np.cross(n, [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        cu, cv = (mesh_np - target) @ u, (mesh_np - target) @ v
        gu, gv = np.meshgrid(np.arange(cu.min(), cu.max(), args.pitch), np.arange(cv.min(), cv.max(), args.pitch), indexing="ij")
        plane_np = (target + gu[..., None] * u + gv[..., None] * v).reshape(-1, 3).astype(np.float32)
        rng = np.random.default_rng(0)
        lo, hi = mesh_np.min(axis=0), mesh_np.max(axis=0)
        mid, half = (lo + hi) / 2.0, float((hi - lo).max()) / 2.0
        n_out = int(round(args.outliers * len(plane_np)))
        outliers = rng.uniform(mid - half, mid + half, (n_out, 3)).astype(np.float32)
        query_np = np.concatenate([plane_np, outliers])
        query = torch.from_numpy(query_np).to(dev)
        nq = int(query.shape[0])
        faces32 = mesh_ops._faces32("microbench", faces, nv, vertices)
        box = D._mesh_box(vertices)

        steps = {k: [] for k in ("fine_build", "first_pass", "collect", "coarse_build", "second_pass", "call", "sample_surface",
                                 "nearest_distances")}
        timer = _lib.KernelTimer()
        for run in range(args.runs + 1):                        # the first is the warm-up
            torch.cuda.synchronize()
            ms, (dist, face) = event_ms(lambda: D.point_mesh_distances(query, vertices, faces, cap, return_face=True))
            steps["call"].append(ms)
            report = D.last_grid_report()
            _lib.set_timer(timer)                               # the steps on their own
            ms, fine = event_ms(lambda: D._FaceGrid(vertices, faces32, box[0], box[1], cap / D.FINE_CELLS_PER_MAX_DIST))
            steps["fine_build"].append(ms)
            d1 = torch.full((nq,), cap, dtype=torch.float32, device=dev)
            f1 = torch.full((nq,), -1, dtype=torch.int32, device=dev)
            done = torch.empty((nq,), dtype=torch.uint8, device=dev)
            ms, _ = event_ms(lambda: D._first_pass(query, fine, cap, d1, f1, done))
            steps["first_pass"].append(ms)
            ms, todo = event_ms(lambda: torch.nonzero(done == 0).view(-1))
            steps["collect"].append(ms)
            ms, coarse = event_ms(lambda: D._FaceGrid(vertices, faces32, box[0], box[1], cap * D.MARGIN))
            steps["coarse_build"].append(ms)
            ms, _ = event_ms(lambda: D._second_pass(query, todo, coarse, cap, d1, f1))
            steps["second_pass"].append(ms)
            _lib.set_timer(None)
            assert torch.equal(d1, dist) and torch.equal(f1.long(), face)        # the steps are the call
            ms, samples = event_ms(lambda: mesh_ops.sample_surface(vertices, faces, args.pitch)[0])
            steps["sample_surface"].append(ms)
            ms, d_sampled = event_ms(lambda: evaluation.nearest_distances(query, samples, cap))
            steps["nearest_distances"].append(ms)
        torch.cuda.synchronize()
        per_run = {}
        for name, e0, e1, _, _, _ in timer.records:
            per_run.setdefault(name, []).append(e0.elapsed_time(e1))
        runs = args.runs + 1

        def kernel_ms(name):                                    # per run the sum over its launches; the median over the runs
            ms = per_run.get(name, [])
            if not ms:
                return None
            each = len(ms) // runs
            return median([sum(ms[r * each:(r + 1) * each]) for r in range(1, runs)])

        # candidates per query on a sample, as the kernels walk the keys
        pick = rng.choice(nq, min(4096, nq), replace=False)
        d_pick = dist[torch.from_numpy(pick).to(dev)].cpu().numpy()
        finished = done[torch.from_numpy(pick).to(dev)].cpu().numpy() != 0
        ring1 = cube_candidates(query_np[pick], fine, 1, D.FINE_RINGS)
        ring3 = cube_candidates(query_np[pick], fine, 3, D.FINE_RINGS)
        reach1 = float(np.float32(0.95) * np.float32(fine.edge))
        stopped_at_1 = finished & (d_pick <= reach1)
        first = ring1 + np.where(stopped_at_1, 0, ring3)
        second = np.where(finished, 0, cube_candidates(query_np[pick], coarse, 1, 1))
        both = (dist < cap) & (d_sampled < cap)
        exact_mean = float(dist[both].double().mean()) if int(both.sum()) else float("nan")
        sampled_mean = float(d_sampled[both].double().mean()) if int(both.sum()) else float("nan")
        out = {"views": V, "height": h, "width": w, "voxel": voxel, "dims": list(dims), "vertices": nv, "faces": nf,
               "queries": nq, "outliers": n_out, "pitch": args.pitch, "max_dist": cap, "runs": args.runs,
               "fine_edge": fine.edge, "fine_widenings": fine.widenings, "fine_pairs": fine.pairs,
               "fine_pairs_per_face": fine.pairs / float(max(nf, 1)), "coarse_edge": coarse.edge,
               "coarse_widenings": coarse.widenings, "coarse_pairs": coarse.pairs,
               "coarse_pairs_per_face": coarse.pairs / float(max(nf, 1)), "budget": D.pair_budget(nf),
               "second_pass_queries": report["second_pass_queries"], "capped_queries": int((face < 0).sum()),
               "call_ms": median(steps["call"][1:]), "fine_build_ms": median(steps["fine_build"][1:]),
               "first_pass_ms": median(steps["first_pass"][1:]), "collect_ms": median(steps["collect"][1:]),
               "coarse_build_ms": median(steps["coarse_build"][1:]), "second_pass_ms": median(steps["second_pass"][1:]),
               "count_kernels_ms": kernel_ms("pf_mesh_dist_count_f32"), "emit_kernels_ms": kernel_ms("pf_mesh_dist_emit_f32"),
               "pack_kernels_ms": kernel_ms("pf_mesh_dist_pack_f32"),
               "candidates_sample": int(len(pick)), "first_pass_candidates_per_query": float(first.mean()),
               "first_pass_candidates_max": int(first.max()), "stopped_at_ring_1_share": float(stopped_at_1.mean()),
               "second_pass_candidates_per_query": float(second[~finished].mean()) if (~finished).any() else 0.0,
               "first_pass_ns_per_candidate": 1e6 * median(steps["first_pass"][1:]) / max(float(first.mean()) * nq, 1.0),
               "samples": int(samples.shape[0]), "sample_surface_ms": median(steps["sample_surface"][1:]),
               "nearest_distances_ms": median(steps["nearest_distances"][1:]),
               "sampled_route_ms": median(steps["sample_surface"][1:]) + median(steps["nearest_distances"][1:]),
               "compared_queries": int(both.sum()), "completeness_mean_exact": exact_mean,
               "completeness_mean_sampled": sampled_mean, "sampled_minus_exact": sampled_mean - exact_mean}
        line = json.dumps(out)
        print(line, flush=True)
        with open(os.path.join(ROOT, "profiles", "mesh_distance_microbench.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
