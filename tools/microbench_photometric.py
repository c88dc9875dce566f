"""Time the photometric consistency check (pointmvsnet_amd/photometric.py, csrc/photo_filter.hip) on a synthetic scan of 49
views at 640 x 480 whose images are rendered from one world texture.  Meant to be run on the MI355X.

    python tools/microbench_photometric.py [--views 49] [--height 480] [--width 640] [--runs 5] [--radii 1 2 3]
                                           [--sources 10 48] [--torch-sources 10] [--tag NAME]

The scan is that of tools/microbench_fusion.py (a 7 x 7 grid of cameras facing a tilted plane, depth noise 0.3); every
view's image is the plane's texture -- three sinusoids per channel, periods of 7, 5 and 12 pixel footprints in three
directions -- seen through the view's own depth map.  ``--sources M``: every view's M nearest cameras (48: all others).
One JSON line per M and radius: the two packs and the kernel under HIP events (median of the runs after a warm-up), the
nominal taps (views x pixels x listed sources x window) and taps per second, what the filter keeps, the kernel's registers,
LDS and scratch from the build's resource file, and the library that ran (``PF_LIB_PATH`` selects another build of it).
For orientation only, for the M in ``--torch-sources``: the torch-only route of the same specification, one
``grid_sample`` per tap on the whole scan, timed once after a warm-up at radius 1, with its largest |ncc| difference from
the kernel.  The lines are printed and appended to ``profiles/photometric_microbench.jsonl``.  No ratio is a claim.
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

TEXTURE = [(7.0, -50.0), (5.0, 20.0), (12.0, 60.0)]       # (period in pixel footprints, direction on the plane in degrees)


def _commit():
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def _median(values):
    return sorted(values)[len(values) // 2]


def render_images(depths, K, E, dev, seed=0):
    """(V, h, w, 3) uint8 on ``dev``: the world texture at the point every pixel sees through its depth (float64)."""
    V, h, w = depths.shape
    n = np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    e1 = np.cross(n, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    foot = 600.0 / K[0, 0, 0]
    phase = np.random.default_rng(seed).uniform(0, 2 * np.pi, (3, 3))
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    pix = torch.from_numpy(np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3)).to(dev)
    images = torch.empty((V, h, w, 3), dtype=torch.uint8, device=dev)
    for v in range(V):
        R, t = E[v, :, :3], E[v, :, 3]
        to_plane = torch.from_numpy(np.stack([R.T @ e1, R.T @ e2], 1)).to(dev)       # camera coordinates -> (a, b); R^-1 = R^T
        cam = (pix @ torch.from_numpy(np.linalg.inv(K[v]).T).to(dev)) * depths[v].reshape(-1, 1).double() - \
            torch.from_numpy(t).to(dev)
        ab = cam @ to_plane
        for ch in range(3):
            value = torch.full((h * w,), 128.0, dtype=torch.float64, device=dev)
            for k, (period, ang) in enumerate(TEXTURE):
                along = ab[:, 0] * np.cos(np.deg2rad(ang)) + ab[:, 1] * np.sin(np.deg2rad(ang))
                value = value + 38.0 * torch.sin(along * (2 * np.pi / (period * foot)) + phase[ch, k])
            images[v, :, :, ch] = torch.round(value.clamp(0, 255)).reshape(h, w).to(torch.uint8)
    return images


def nearest_sources(E, M):
    """(V, M) int32: every view's M nearest camera centres, nearest first."""
    C = np.stack([-e[:, :3].T @ e[:, 3] for e in E])
    dist = np.linalg.norm(C[:, None] - C[None], axis=2)
    np.fill_diagonal(dist, np.inf)
    return np.argsort(dist, axis=1, kind="stable")[:, :M].astype(np.int32)


def _kernels(fn, runs):
    """HIP-event time of every C-ABI entry inside ``fn``: ({entry: [ms per run]}, event floor), after a warm-up."""
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


def torch_route(depths, grey, table, rows, radius, var_min, depth_min=1e-3, depth_max=1e5):
    """The specification with torch operations alone: per source slot and tap one ``grid_sample`` over all views.  Returns
    ncc (V, M, h, w) with NaN where a source is not usable.  For orientation; its bits are not the kernel's."""
    import torch.nn.functional as F
    V, h, w = depths.shape
    M = table.shape[1]
    r, n = radius, (2 * radius + 1) ** 2
    dev = depths.device
    g = grey.to(torch.int32)
    gf = grey.to(torch.float32)[:, None]
    inner = (slice(None), slice(r, h - r), slice(r, w - r))
    c = g[inner]
    SR, SRR = torch.zeros_like(c), torch.zeros_like(c)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            R = g[:, r + dy:h - r + dy, r + dx:w - r + dx] - c
            SR += R
            SRR += R * R
    VR = n * SRR - SR * SR
    d = depths[inner]
    scorable = (d > depth_min) & (d < depth_max) & (VR >= var_min)
    ys, xs = torch.meshgrid(torch.arange(r, h - r, device=dev), torch.arange(r, w - r, device=dev), indexing="ij")
    ncc = torch.full((V, M, h, w), float("nan"), device=dev)
    cf = c.float()
    for m in range(M):
        j = table[:, m]
        listed = (j >= 0) & (j != torch.arange(V, device=dev))
        src = gf[j.clamp(min=0).long()]
        row = rows[:, m].view(V, 16, 1, 1)
        S1, S2, SX = torch.zeros_like(cf), torch.zeros_like(cf), torch.zeros_like(cf)
        inside_all = torch.ones_like(scorable)
        for dy in range(-r, r + 1):
            py = (ys + dy).float() + 0.5
            for dx in range(-r, r + 1):
                R = (g[:, r + dy:h - r + dy, r + dx:w - r + dx] - c).float()
                px = (xs + dx).float() + 0.5
                qx = (row[:, 0] * px + row[:, 1] * py + row[:, 2]) * d + row[:, 9]
                qy = (row[:, 3] * px + row[:, 4] * py + row[:, 5]) * d + row[:, 10]
                z = (row[:, 6] * px + row[:, 7] * py + row[:, 8]) * d + row[:, 11]
                rz = 1.0 / z
                u, v = qx * rz, qy * rz
                x0, y0 = torch.floor(u - 0.5), torch.floor(v - 0.5)
                inside_all &= (z > 0) & (x0 >= 0) & (x0 + 1 <= w - 1) & (y0 >= 0) & (y0 + 1 <= h - 1)
                grid = torch.stack([u * (2.0 / w) - 1.0, v * (2.0 / h) - 1.0], -1)
                s = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0] - cf
                S1 += s
                S2 += s * s
                SX += R * s
        VS = n * S2 - S1 * S1
        COV = n * SX - SR.float() * S1
        ok = scorable & inside_all & (VS >= float(var_min)) & listed.view(V, 1, 1)
        val = (COV / torch.sqrt(VR.float() * VS)).clamp(-1.0, 1.0)
        ncc[:, m, r:h - r, r:w - r] = torch.where(ok, val, torch.full_like(val, float("nan")))
    return ncc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--radii", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--sources", type=int, nargs="+", default=[10, 48], help="source views per view (M)")
    ap.add_argument("--torch-sources", type=int, nargs="*", default=[10], help="the M for which the torch-only route runs too")
    ap.add_argument("--tag", default=None, help="a name for the build that ran, kept in the lines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_microbench.jsonl"))
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import _lib, build, geometric, photometric
    dev = torch.device("cuda:0")
    V, h, w = args.views, args.height, args.width
    depths, K, E, _ = make_scan(V, h, w)
    d_dev = torch.from_numpy(depths).to(dev)
    i_dev = render_images(d_dev, K, E, dev)
    usage = None
    try:
        with open(build.USAGE_FILE) as f:
            names = {"ILi0E": "ncc_runtime_radius", "ILi1E": "ncc_radius_1", "ILi2E": "ncc_radius_2", "ILi3E": "ncc_radius_3",
                     "grey_pack": "grey_pack", "grey_quads": "grey_quads"}
            usage = {label: u for name, u in json.load(f)["photo_filter.hip"].items() for key, label in names.items()
                     if key in name and "photo_" in name}
    except (OSError, ValueError, KeyError):
        pass
    lines = []
    for M in args.sources:
        M = min(M, V - 1)
        table = nearest_sources(E, M)
        for radius in args.radii:
            n = (2 * radius + 1) ** 2
            run = lambda: photometric.photometric_consistency(d_dev, i_dev, K, E, sources=table, radius=radius)   # noqa: E731
            sums, floor = _kernels(run, args.runs)
            ncc_ms, pack_ms = _median(sums["pf_photo_ncc_f32"]), _median(sums["pf_grey_pack_u8"])
            quads_ms = _median(sums["pf_grey_quads_u8"])
            t0 = time.perf_counter()
            out = run()
            torch.cuda.synchronize()
            wall_ms = (time.perf_counter() - t0) * 1e3
            _, rep = photometric.photometric_filter(d_dev, i_dev, K, E, sources=table, radius=radius)
            taps = float(V) * h * w * M * n
            lds = (16 + 2 * radius) ** 2
            line = dict(bench="photometric", tag=args.tag, views=V, height=h, width=w, sources=M, radius=radius, runs=args.runs,
                        commit=_commit(), device=torch.cuda.get_device_name(0), library=os.path.basename(_lib.LIB_PATH),
                        grey_pack_ms=pack_ms, grey_quads_ms=quads_ms, ncc_ms=ncc_ms, ncc_ms_all=sums["pf_photo_ncc_f32"], event_floor_ms=floor,
                        call_wall_ms=wall_ms, nominal_taps=taps, tera_taps_per_s=taps / ncc_ms / 1e9,
                        dynamic_lds_bytes=lds, resource_usage=usage, report=rep["total"], score_sum=float(out[0].double().sum()),
                        two_calls_equal=bool(
                            all(torch.equal(a, b) for a, b in zip(out, run()))))
            if M in args.torch_sources:
                var_min = rep["settings"]["var_min"]
                rows = torch.from_numpy(geometric.source_maps(K, E, table)[:, :, 0].copy()).to(dev)
                t_dev = torch.from_numpy(table).to(dev)
                grey = photometric.grey_images(i_dev)
                if radius == 1:
                    torch_route(d_dev, grey, t_dev, rows, radius, var_min)                               # warm-up
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = torch_route(d_dev, grey, t_dev, rows, radius, var_min)
                torch.cuda.synchronize()
                line["torch_route_wall_ms"] = (time.perf_counter() - t0) * 1e3
                mine = photometric.photometric_consistency(d_dev, i_dev, K, E, sources=table, radius=radius,
                                                           return_per_source=True)[4]
                both = ~torch.isnan(ref) & ~torch.isnan(mine)
                line["torch_route_usable_pairs_differing"] = int((torch.isnan(ref) != torch.isnan(mine)).sum())
                line["torch_route_largest_ncc_difference"] = float((ref - mine)[both].abs().max()) if bool(both.any()) else 0.0
                del ref, mine, both
                torch.cuda.empty_cache()
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
