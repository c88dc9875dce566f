"""Time the normal maps (pointmvsnet_amd/normals.py, csrc/depth_normals.hip) on a DTU-sized scan: 49 views of 640 x 480.

    python tools/microbench_normals.py [--views 49] [--height 480] [--width 640] [--runs 20] [--no-torch]

The scan is that of tools/microbench_fusion.py (a 7 x 7 grid of cameras facing a tilted plane, depth noise 0.3).  One JSON
line per ``step`` in (1, 3): ``depth_normals`` as a whole call (matrix composition on the host, upload, the kernel; median of
the runs, wall clock around a device synchronisation) and the kernel alone (HIP events) with its algorithmic bytes -- 16 per
pixel: the pixel's own depth in, three floats out -- as GB/s, next to a torch-only route of the same specification on the
same GPU (shifted slices, ``where`` and ``cross``; its float arithmetic is the library's, so ``torch_defined_equal`` and
``torch_angle_max_deg`` say how far the two agree) and, for orientation only, next to the bytes per second that the
preprocessing kernels reached (profiles/preprocess_microbench.jsonl, cfg 5).  One more line for the disparity fuser:
``fuse_depth_maps`` with and without ``with_normals`` and the fused-normal kernel alone.  The lines are printed and appended
to ``profiles/normals_microbench.jsonl``.  No ratio between the routes is a claim: the torch route exists to place the number.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


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


def _kernel(name, fn, runs):
    """HIP-event time of the C-ABI entry ``name`` inside ``fn``: (ms per launch, bytes per launch, event floor, fn's result)."""
    from pointmvsnet_amd import _lib
    timer = _lib.KernelTimer(only=name)
    _lib.set_timer(timer)
    try:
        for _ in range(runs):
            out = fn()
    finally:
        _lib.set_timer(None)
    k = timer.summary()[name]
    return k["ms"] / k["launches"], k["bytes"] / k["launches"], k["event_floor_ms"], out


def _shifted(t, dy, dx):
    """``out[:, y, x] = t[:, y + dy, x + dx]`` where inside, else 0; and the (h, w) inside mask."""
    h, w = t.shape[1:3]
    out = torch.zeros_like(t)
    inside = torch.zeros((h, w), dtype=torch.bool, device=t.device)
    if abs(dy) >= h or abs(dx) >= w:
        return out, inside
    dst = (slice(max(-dy, 0), min(h - dy, h)), slice(max(-dx, 0), min(w - dx, w)))
    src = (slice(max(dy, 0), min(h + dy, h)), slice(max(dx, 0), min(w + dx, w)))
    out[(slice(None),) + dst] = t[(slice(None),) + src]
    inside[dst] = True
    return out, inside


def torch_route(depths, A, step, rel_jump=0.01, depth_min=1e-3, depth_max=1e5):
    """The specification of pointmvsnet_amd/normals.py with library operators: depths (V, h, w), A (V, 3, 3) on the GPU."""
    V, h, w = depths.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=depths.device) + 0.5, torch.arange(w, device=depths.device) + 0.5, indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1)
    P = torch.einsum("vab,hwb->vhwa", A, pix) * depths[..., None]
    valid = (depths > depth_min) & (depths < depth_max)

    def linked(dy, dx):
        dq, inside = _shifted(depths, dy, dx)
        return valid & inside & (dq > depth_min) & (dq < depth_max) & ((dq - depths).abs() <= rel_jump * depths)

    def tangent(dy, dx):
        f, b = linked(dy, dx), linked(-dy, -dx)
        head = torch.where(f[..., None], _shifted(P, dy, dx)[0], P)
        tail = torch.where(b[..., None], _shifted(P, -dy, -dx)[0], P)
        return head - tail, f | b

    tx, okx = tangent(0, step)
    ty, oky = tangent(step, 0)
    c = torch.cross(tx, ty, dim=-1)
    length = c.norm(dim=-1)
    n = c / length[..., None]
    facing = (n * P).sum(-1)
    n = torch.where((facing > 0)[..., None], -n, n)
    ok = valid & okx & oky & (length > 0) & torch.isfinite(length) & (facing != 0)
    return torch.where(ok[..., None], n, torch.zeros_like(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_microbench.jsonl"))
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import camera_maps, fusion, normals
    V, h, w = args.views, args.height, args.width
    depths, K, E, images = make_scan(V, h, w)
    dev = torch.device("cuda:0")
    d_dev, i_dev = torch.from_numpy(depths).to(dev), torch.from_numpy(images).to(dev)
    A = torch.from_numpy(camera_maps.view_maps(camera_maps.decompose("microbench_normals", K, E))[:, :9].reshape(V, 3, 3)).to(dev)
    orientation = None
    try:
        with open(os.path.join(ROOT, "profiles", "preprocess_microbench.jsonl")) as f:
            orientation = json.loads(f.readline())["cfg5"]["kernels_bytes_per_s"] / 1e9
    except (OSError, ValueError, KeyError):
        pass
    common = {"views": V, "height": h, "width": w, "runs": args.runs, "commit": _commit(), "device": torch.cuda.get_device_name(0)}
    lines = []
    for step in (1, 3):
        def call():
            return normals.depth_normals(d_dev, K, E, step=step)
        walls = _wall(call, args.runs)
        ms, nbytes, floor, got = _kernel("pf_depth_normals_f32", call, args.runs)
        line = dict(common, bench="depth_normals", step=step, call_ms_median=sorted(walls)[len(walls) // 2], call_ms_min=min(walls),
                    call_ms_max=max(walls), kernel_ms=ms, kernel_algo_gbytes=nbytes / 1e9, kernel_gbytes_per_s=nbytes / ms / 1e6,
                    event_floor_ms=floor, defined_share=float((got != 0).any(dim=-1).float().mean()),
                    two_calls_equal=bool(torch.equal(got, call())), preprocess_kernels_gbytes_per_s=orientation)
        if not args.no_torch:
            route = _wall(lambda: torch_route(d_dev, A, step), max(2, args.runs // 4))
            ref = torch_route(d_dev, A, step)
            both = (ref != 0).any(dim=-1) & (got != 0).any(dim=-1)
            angle = torch.atan2(torch.cross(ref, got, dim=-1).norm(dim=-1), (ref * got).sum(-1))[both]
            line.update(torch_route_ms_median=sorted(route)[len(route) // 2],
                        torch_defined_equal=bool(torch.equal((ref != 0).any(dim=-1), (got != 0).any(dim=-1))),
                        torch_angle_max_deg=float(torch.rad2deg(angle).max()) if angle.numel() else None)
        lines.append(line)
    plain = _wall(lambda: fusion.fuse_depth_maps(d_dev, K, E, images=i_dev), args.runs)

    def fuse():
        return fusion.fuse_depth_maps(d_dev, K, E, images=i_dev, with_normals=True)
    oriented = _wall(fuse, args.runs)
    ms, _, floor, (pts, _, nrm) = _kernel("pf_fuse_normals_f32", fuse, args.runs)
    # what the fused-normal kernel moves: the emit byte of every pixel; per emitting pixel its V - 1 matches, its own normal,
    # one gathered normal per match (at most V - 1; counted in full, hence "upper") and the row out
    nbytes = V * h * w + int(pts.shape[0]) * (4 * (V - 1) + 12 * (V + 1))
    lines.append(dict(common, bench="fused_normals", points=int(pts.shape[0]),
                      normals_undefined=int((nrm == 0).all(dim=1).sum()), fuse_depth_maps_ms_median=sorted(plain)[len(plain) // 2],
                      fuse_depth_maps_with_normals_ms_median=sorted(oriented)[len(oriented) // 2], kernel_ms=ms,
                      kernel_algo_gbytes_upper=nbytes / 1e9, kernel_gbytes_per_s_upper=nbytes / ms / 1e6, event_floor_ms=floor))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
