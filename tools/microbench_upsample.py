"""Time the guided depth upsampling (pointmvsnet_amd/refine.py, csrc/depth_refine.hip) on the synthetic scan of 49 views, from
320 x 256 to 640 x 512 and from 800 x 576 to 1600 x 1152.

    python tools/microbench_upsample.py [--views 49] [--runs 5] [--sizes 256x320 576x800] [--scale 2] [--no-torch] [--no-fuse]

The scan is that of tools/microbench_fusion.py (a 7 x 7 grid of cameras facing a tilted plane, depth noise 0.3); the guides are
flat 32 x 32 blocks of seeded colours with +-6 of noise, made on the device.  One JSON line per size and setting -- ``radius``
2 and 4, ``anchor_radius`` 0 and 1: the pack kernel and the upsampling kernel apart under HIP events (median of the runs after a
warm-up), taps per second, and TB/s of ``3 + 4 + 8 / s^2`` algorithmic bytes per output pixel (its own guide colour in, its
depth out, its share of the records), next to a torch-only route of the same specification on the same GPU (shifted slices
of the low-resolution maps, ``repeat_interleave`` to the output grid, ``where``; its float arithmetic is the library's, so
``torch_holes_equal``, ``torch_counts_equal`` and ``torch_max_abs_diff`` say how far the two agree).  One more line per size:
``fuse_depth_maps`` on the low-resolution grid and on the upsampled one, with the point counts.  The lines are printed and
appended to ``profiles/upsample_microbench.jsonl``.  No ratio between the routes is a claim: the torch route exists to place
the number.
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


def _median(values):
    return sorted(values)[len(values) // 2]


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


def _kernels(fn, runs):
    """HIP-event times of every C-ABI entry inside ``fn``, one sample per run: ({entry: [ms, ...]}, event floor, fn's result)."""
    from pointmvsnet_amd import _lib
    fn()                                                                       # warm-up
    torch.cuda.synchronize()
    timer = _lib.KernelTimer()
    _lib.set_timer(timer)
    try:
        for _ in range(runs):
            out = fn()
    finally:
        _lib.set_timer(None)
    floor = next(iter(timer.summary().values()))["event_floor_ms"]            # synchronises
    times = {}
    for name, e0, e1, _, _, _ in timer.records:
        times.setdefault(name, []).append(e0.elapsed_time(e1))
    return times, floor, out


def make_guides(V, H, W, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    blocks = torch.randint(0, 256, (V, (H + 31) // 32, (W + 31) // 32, 3), generator=g, device=dev, dtype=torch.int16)
    flat = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W]
    noise = torch.randint(-6, 7, (V, H, W, 3), generator=g, device=dev, dtype=torch.int16)
    return (flat + noise).clamp_(0, 255).to(torch.uint8).contiguous()


def _shifted(t, dy, dx, fill):
    """``out[:, y, x] = t[:, y + dy, x + dx]`` where inside the map, else ``fill``."""
    h, w = t.shape[1:3]
    out = torch.full_like(t, fill)
    if abs(dy) >= h or abs(dx) >= w:
        return out
    dst = (slice(None), slice(max(-dy, 0), min(h - dy, h)), slice(max(-dx, 0), min(w - dx, w)))
    src = (slice(None), slice(max(dy, 0), min(h + dy, h)), slice(max(dx, 0), min(w + dx, w)))
    out[dst] = t[src]
    return out


def torch_route(depths, guides, s, radius, anchor_radius, ws, wc, rel_jump=0.02, depth_min=1e-3, depth_max=1e5):
    """The specification of pointmvsnet_amd/refine.py with library operators: depths (V, h, w), guides (V, s h, s w, 3),
    ws (s, 2 radius + 1) and wc (766,) on the GPU -> (out (V, H, W) float32, count (V, H, W) int32)."""
    V, h, w = depths.shape
    H, W = h * s, w * s
    dev = depths.device
    py, px = torch.arange(H, device=dev) % s, torch.arange(W, device=dev) % s
    own = guides.to(torch.int16)
    tap_colour = guides[:, s // 2::s, s // 2::s].contiguous()
    up = lambda t: t.repeat_interleave(s, 1).repeat_interleave(s, 2)

    def tap(tx, ty):
        d = up(_shifted(depths, ty, tx, float("nan")))
        c = up(_shifted(tap_colour, ty, tx, 0)).to(torch.int16)
        a = (c - own).abs_().sum(-1, dtype=torch.int32)
        wt = (ws[py, ty + radius][:, None] * ws[px, tx + radius][None, :]) * wc[a]
        return d, (d > depth_min) & (d < depth_max), wt

    dc, centre_valid, w_best = tap(0, 0)
    d0 = dc.clone()
    for ty in range(-anchor_radius, anchor_radius + 1):
        for tx in range(-anchor_radius, anchor_radius + 1):
            d, valid, wt = tap(tx, ty)
            better = valid & (wt > w_best)
            w_best = torch.where(better, wt, w_best)
            d0 = torch.where(better, d, d0)
    jump = rel_jump * d0
    wsum, ssum = torch.zeros_like(d0), torch.zeros_like(d0)
    count = torch.zeros((V, H, W), dtype=torch.int32, device=dev)
    zero = torch.zeros((), device=dev)
    for ty in range(-radius, radius + 1):
        for tx in range(-radius, radius + 1):
            d, valid, wt = tap(tx, ty)
            diff = d - d0
            linked = valid & (diff.abs() <= jump)
            wsum = wsum + torch.where(linked, wt, zero)
            ssum = ssum + torch.where(linked, wt * diff, zero)
            count += linked
    out = torch.where(wsum > 0, d0 + ssum / wsum, d0)
    return torch.where(centre_valid, out, zero), torch.where(centre_valid, count, torch.zeros_like(count))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--sizes", nargs="+", default=["256x320", "576x800"], help="low-resolution HEIGHTxWIDTH of the depth maps")
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-fuse", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_microbench.jsonl"))
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import build, fusion, refine
    dev = torch.device("cuda:0")
    V, s = args.views, args.scale
    usage = None
    try:
        with open(build.USAGE_FILE) as f:
            usage = {("count" if "ILb1E" in name else "plain" if "upsample" in name else "pack"):
                     {k: u[k] for k in ("vgprs", "sgprs", "scratch_bytes_per_lane")}
                     for name, u in json.load(f)["depth_refine.hip"].items() if "upsample" in name or "guide_pack" in name}
    except (OSError, ValueError, KeyError):
        pass
    lines = []
    for size in args.sizes:
        h, w = (int(v) for v in size.split("x"))
        H, W = h * s, w * s
        depths, K, E, _ = make_scan(V, h, w)
        d_dev = torch.from_numpy(depths).to(dev)
        guides = make_guides(V, H, W, dev)
        common = {"views": V, "height": h, "width": w, "scale": s, "out_height": H, "out_width": W, "runs": args.runs,
                  "commit": _commit(), "device": torch.cuda.get_device_name(0), "resource_usage": usage}
        for radius in (2, 4):
            for anchor in (0, 1):
                kw = dict(radius=radius, anchor_radius=anchor)
                times, floor, got = _kernels(lambda: refine.upsample_depth_maps(d_dev, guides, **kw), args.runs)
                pack_ms, up_ms = _median(times["pf_guide_pack_f32"]), _median(times["pf_depth_upsample_f32"])
                taps = float(V) * H * W * ((2 * radius + 1) ** 2 + (2 * anchor + 1) ** 2)
                nbytes = float(V) * H * W * (3 + 4 + 8.0 / (s * s))
                footprint = (16 // s if 16 % s == 0 else 16 // s + 2) + 2 * radius
                pitch = ((footprint + 15) // 32) * 32 + 16 if s == 1 else footprint
                walls = _wall(lambda: refine.upsample_depth_maps(d_dev, guides, **kw), args.runs)
                counted = refine.upsample_depth_maps(d_dev, guides, return_count=True, **kw)
                line = dict(common, bench="upsample_depth_maps", radius=radius, anchor_radius=anchor, pack_ms=pack_ms,
                            upsample_ms=up_ms, upsample_ms_min=min(times["pf_depth_upsample_f32"]),
                            upsample_ms_max=max(times["pf_depth_upsample_f32"]), event_floor_ms=floor,
                            taps_per_s=taps / up_ms * 1e3, algo_gbytes=nbytes / 1e9, algo_tbytes_per_s=nbytes / up_ms / 1e9,
                            lds_bytes_per_block=footprint * pitch * 8 + 4 * (768 + s * (2 * radius + 1)),
                            call_ms_median=_median(walls), holes=int((got == 0).sum()),
                            counted_arm_equal=bool(torch.equal(counted[0], got)),
                            two_calls_equal=bool(torch.equal(got, refine.upsample_depth_maps(d_dev, guides, **kw))))
                if not args.no_torch:
                    ws = torch.from_numpy(refine.spatial_table(s, radius, 1.0)).to(dev)
                    wc = torch.from_numpy(refine.colour_table(12.0)).to(dev)
                    route = _wall(lambda: torch_route(d_dev, guides, s, radius, anchor, ws, wc), 2)
                    ref, ref_count = torch_route(d_dev, guides, s, radius, anchor, ws, wc)
                    line.update(torch_route_ms_median=_median(route), torch_holes_equal=bool(torch.equal(ref == 0, got == 0)),
                                torch_counts_equal=bool(torch.equal(ref_count, counted[1])),
                                torch_max_abs_diff=float((ref - got).abs().max()),
                                torch_bitwise_equal=bool(torch.equal(ref, got)))
                    del ref, ref_count
                lines.append(line)
                print(json.dumps(line), flush=True)
                del got, counted
        if not args.no_fuse:
            low_images = guides[:, s // 2::s, s // 2::s].contiguous()
            hi = refine.upsample_depth_maps(d_dev, guides)
            K_hi = refine.upsampled_intrinsics(K, s)
            low = _wall(lambda: fusion.fuse_depth_maps(d_dev, K, E, images=low_images), args.runs)
            high = _wall(lambda: fusion.fuse_depth_maps(hi, K_hi, E, images=guides), args.runs)
            line = dict(common, bench="fuse_depth_maps_on_both_grids", fuse_low_ms_median=_median(low),
                        fuse_high_ms_median=_median(high),
                        points_low=int(fusion.fuse_depth_maps(d_dev, K, E, images=low_images)[0].shape[0]),
                        points_high=int(fusion.fuse_depth_maps(hi, K_hi, E, images=guides)[0].shape[0]))
            lines.append(line)
            print(json.dumps(line), flush=True)
            del hi
        del guides, d_dev
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
