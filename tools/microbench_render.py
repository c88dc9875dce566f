"""Time the point-cloud renderer (pointmvsnet_amd/render.py, csrc/cloud_render.hip) on a DTU-sized job.

    python tools/microbench_render.py [--views 49] [--height 480] [--width 640] [--runs 5] [--no-torch]

The cloud is the ground-truth plane of tools/microbench_evaluation.py sampled at 0.2 pitch plus the fused 49-view 640 x 480
scan of tools/microbench_fusion.py; it is rendered into the scan's 49 views at ``splat`` 0 and 1.  Per ``splat`` the splat
and the decode are timed separately (HIP events around each C-ABI entry, the zbuf fill apart; medians of ``--runs``) next to
the whole ``render_depth_maps`` call with the index map, and next to a torch-only route on the same GPU for the depth
alone: per view a matmul projection, then ``scatter_reduce_(..., "amin")`` per footprint offset.  That route has no index
map, and its float arithmetic is the library's, so ``torch_depth_equal_share`` reports how many pixels agree bit for bit
and ``torch_filled_equal`` whether the same pixels are filled.  Prints one JSON line and appends it to
profiles/render_microbench.jsonl.
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
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return median(out), res


def torch_route(points, proj, h, w, splat, depth_min=1e-3, depth_max=1e5):
    """The depth maps alone with library operators: the nearest z per pixel through scatter_reduce_ (amin)."""
    V = proj.shape[0]
    P = proj.view(V, 3, 4)
    out = torch.full((V, h * w), float("inf"), device=points.device)
    for v in range(V):
        q = points @ P[v, :, :3].t() + P[v, :, 3]
        z = q[:, 2]
        u, t = q[:, 0] / z, q[:, 1] / z
        ok = (z > depth_min) & (z < depth_max) & (u >= -splat) & (u < w + splat) & (t >= -splat) & (t < h + splat)
        xc, yc, z = torch.floor(u[ok]).long(), torch.floor(t[ok]).long(), z[ok]
        for dy in range(-splat, splat + 1):
            for dx in range(-splat, splat + 1):
                x, y = xc + dx, yc + dy
                inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
                out[v].scatter_reduce_(0, (y * w + x)[inside], z[inside], "amin")
    return torch.where(torch.isinf(out), torch.zeros_like(out), out).view(V, h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import _lib, fusion, render
    V, h, w = args.views, args.height, args.width
    depths, K, E, _ = make_scan(V, h, w)
    dev = torch.device("cuda:0")
    fused, _ = fusion.fuse_depth_maps(torch.from_numpy(depths).to(dev), K, E)
    fused_np = fused.cpu().numpy()
    # the scan's plane n . X = n . target sampled at 0.2 pitch over the fused cloud's footprint (microbench_evaluation.py)
    n = np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    target = np.array([0.0, 0.0, 600.0])
    a = np.cross(n, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    rel = fused_np.astype(np.float64) - target
    ca, cb = rel @ a, rel @ b
    ga, gb = np.meshgrid(np.arange(ca.min(), ca.max(), 0.2), np.arange(cb.min(), cb.max(), 0.2), indexing="ij")
    plane = (target + ga[..., None] * a + gb[..., None] * b).reshape(-1, 3).astype(np.float32)
    points = torch.cat([torch.from_numpy(plane).to(dev), fused]).contiguous()
    N = int(points.shape[0])
    proj = torch.from_numpy(render.world_maps(K, E)).to(dev)
    out = {"views": V, "height": h, "width": w, "points": N, "plane_points": int(plane.shape[0]),
           "fused_points": int(fused.shape[0]), "runs": args.runs, "cloud_bytes": 12 * N, "zbuf_bytes": 8 * V * h * w}
    for splat in (0, 1):
        zbuf = torch.empty((V, h, w), dtype=torch.int64, device=dev)
        depth = torch.empty((V, h, w), dtype=torch.float32, device=dev)
        index = torch.empty((V, h, w), dtype=torch.int32, device=dev)

        def splat_once():
            zbuf.fill_(-1)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.call("pf_cloud_splat_f32", _lib.ptr(points), N, _lib.ptr(proj), V, h, w, splat, 1e-3, 1e5, _lib.ptr(zbuf),
                      _lib.stream())
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        splat_once()                                                              # warm-up
        splat_ms = median([splat_once() for _ in range(args.runs)])
        decode_ms, _ = event_ms(lambda: _lib.call("pf_cloud_zbuf_decode", _lib.ptr(zbuf), V, h, w, _lib.ptr(depth),
                                                  _lib.ptr(index), _lib.stream()), args.runs)
        fill_ms, _ = event_ms(lambda: zbuf.fill_(-1), args.runs)
        call_ms, (got, got_index) = event_ms(lambda: render.render_depth_maps(points, K, E, h, w, splat=splat,
                                                                              return_index=True), args.runs)
        again = render.render_depth_maps(points, K, E, h, w, splat=splat, return_index=True)
        row = {"splat_ms": splat_ms, "decode_ms": decode_ms, "zbuf_fill_ms": fill_ms, "render_depth_maps_ms": call_ms,
               "projections_per_us": N * V / (splat_ms * 1e3), "filled_share": float((got > 0).float().mean()),
               "two_calls_equal": bool(torch.equal(got, again[0]) and torch.equal(got_index, again[1]))}
        if not args.no_torch:
            torch_route(points, proj, h, w, splat)                                # warm-up
            torch_ms, ref = event_ms(lambda: torch_route(points, proj, h, w, splat), max(1, args.runs // 2))
            row.update(torch_route_ms=torch_ms, torch_filled_equal=bool(torch.equal(ref > 0, got > 0)),
                       torch_depth_equal_share=float((ref == got).float().mean()),
                       torch_depth_max_abs_diff=float((ref - got).abs().max()))
        out["splat%d" % splat] = row
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "render_microbench.jsonl"), "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
