"""Time the mesh rasteriser (pointmvsnet_amd/render.py "Mesh rasterisation", csrc/mesh_render.hip) on a DTU-sized job.

    python tools/microbench_mesh_render.py [--views 49] [--height 480] [--width 640] [--voxels 1.0 0.5] [--runs 5]
        [--lane-pixels 16 32 64 128]

The scan is the synthetic one of tools/microbench_fusion.py (49 views of 640 x 480 of a tilted plane at depth 600, noise 0.3).

(a) Its TSDF mesh (``TSDFVolume`` over ``volume_bounds`` grown by ``trunc = 4 voxel``, ``min_weight`` 2) at every ``--voxels``
    pitch is rasterised into the scan's own views: the raster kernel, the decode and the barycentric pass apart (HIP events
    around each C-ABI entry, the zbuf fill apart; a warm-up call, then the median of ``--runs``), next to the whole
    ``render_mesh_depth_maps`` call with both extra maps.  The raster kernel is timed once per ``--lane-pixels`` value S
    (``pf_mesh_raster_tuned_f32``): faces whose clamped bounding box holds more than S pixels are walked by a wave instead
    of a lane.  ``face_views_per_s`` is faces x views over the raster time at the library's own S.
(b) A two-triangle plane that covers every view: the wave-shared walk alone.
(c) For orientation only, ``render_depth_maps`` of the same mesh's vertices at ``splat=1``.

Prints one JSON line per case and appends it to profiles/mesh_render_microbench.jsonl.
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


def event_ms(fn, runs):
    """The median of ``runs`` event-timed calls after one warm-up call, and the last result."""
    out, res = [], fn()
    for _ in range(runs):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return median(out), res


def time_mesh(vertices, faces, K, E, h, w, runs, lane_pixels):
    """The three kernels apart and the whole call, on ``vertices`` (Nv, 3) float32 and ``faces`` (Nf, 3) int32 on the GPU."""
    from pointmvsnet_amd import _lib, render
    dev = vertices.device
    proj = torch.from_numpy(render.world_maps(K, E)).to(dev)
    V, Nv, Nf = int(proj.shape[0]), int(vertices.shape[0]), int(faces.shape[0])
    zbuf = torch.empty((V, h, w), dtype=torch.int64, device=dev)
    depth = torch.empty((V, h, w), dtype=torch.float32, device=dev)
    index = torch.empty((V, h, w), dtype=torch.int32, device=dev)
    bary = torch.empty((V, h, w, 3), dtype=torch.float32, device=dev)
    head = (_lib.ptr(vertices), Nv, _lib.ptr(faces), Nf, _lib.ptr(proj), V, h, w, 1e-3, 1e5)

    def raster(S):
        def once():
            zbuf.fill_(-1)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.call("pf_mesh_raster_tuned_f32", *(head + (0, S, _lib.ptr(zbuf), _lib.stream())))
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        once()                                                                    # warm-up
        return median([once() for _ in range(runs)])

    raster_ms = {str(S): raster(S) for S in lane_pixels}
    own = raster(render.MESH_LANE_PIXELS)                                         # leaves the library's own zbuf behind
    decode_ms, _ = event_ms(lambda: _lib.call("pf_cloud_zbuf_decode", _lib.ptr(zbuf), V, h, w, _lib.ptr(depth), _lib.ptr(index),
                                              _lib.stream()), runs)
    bary_ms, _ = event_ms(lambda: _lib.call("pf_mesh_bary_f32", *(head + (_lib.ptr(index), _lib.ptr(bary), _lib.stream()))), runs)
    fill_ms, _ = event_ms(lambda: zbuf.fill_(-1), runs)
    call_ms, got = event_ms(lambda: render.render_mesh_depth_maps(vertices, faces, K, E, h, w, return_index=True,
                                                                  return_barycentric=True), runs)
    again = render.render_mesh_depth_maps(vertices, faces, K, E, h, w, return_index=True, return_barycentric=True)
    return {"vertices": Nv, "faces": Nf, "raster_ms_by_lane_pixels": raster_ms, "lane_pixels": render.MESH_LANE_PIXELS,
            "raster_ms": own, "decode_ms": decode_ms, "bary_ms": bary_ms, "zbuf_fill_ms": fill_ms,
            "render_mesh_depth_maps_ms": call_ms, "face_views_per_s": Nf * V / (own * 1e-3),
            "filled_share": float((got[0] > 0).float().mean()),
            "two_calls_equal": bool(all(torch.equal(a, b) for a, b in zip(got, again)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--voxels", type=float, nargs="+", default=[1.0, 0.5])
    ap.add_argument("--min-weight", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--lane-pixels", type=int, nargs="+", default=[16, 32, 64, 128])
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import render, tsdf
    V, h, w = args.views, args.height, args.width
    depths_np, K, E, _ = make_scan(V, h, w)
    dev = torch.device("cuda:0")
    depths = torch.from_numpy(depths_np).to(dev)
    common = {"views": V, "height": h, "width": w, "runs": args.runs, "zbuf_bytes": 8 * V * h * w}
    lines = []
    for voxel in args.voxels:                                                     # (a) and (c)
        trunc = 4.0 * voxel
        origin, dims = tsdf.dims_for(tsdf.volume_bounds(depths, K, E, pad=trunc), voxel)
        vol = tsdf.TSDFVolume(origin, voxel, dims, trunc, with_colour=False, device=dev)
        vol.integrate(depths, K, E)
        vertices, faces = vol.extract(args.min_weight)[:2]
        del vol
        row = dict(common, case="tsdf_mesh", voxel=voxel, dims=list(dims))
        row.update(time_mesh(vertices, faces, K, E, h, w, args.runs, args.lane_pixels))
        splat_ms, cloud_depth = event_ms(lambda: render.render_depth_maps(vertices, K, E, h, w, splat=1), args.runs)
        row.update(splat1_of_the_vertices_ms=splat_ms, splat1_filled_share=float((cloud_depth > 0).float().mean()))
        lines.append(row)
        del vertices, faces
    # (b) two triangles through the scan's plane n . X = n . target, far larger than any view's footprint
    n = np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    a = np.cross(n, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    corners = np.array([0.0, 0.0, 600.0]) + 600.0 * np.array([-a - b, a - b, a + b, -a + b])
    vertices = torch.from_numpy(corners.astype(np.float32)).to(dev)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev)
    row = dict(common, case="two_triangle_plane")
    row.update(time_mesh(vertices, faces, K, E, h, w, args.runs, args.lane_pixels))
    lines.append(row)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_render_microbench.jsonl"), "a") as f:
        for row in lines:
            line = json.dumps(row)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
