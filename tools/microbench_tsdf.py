"""Time the TSDF integration and the marching-tetrahedra extraction (pointmvsnet_amd/tsdf.py, csrc/tsdf.hip) on a DTU-sized job.

    python tools/microbench_tsdf.py [--views 49] [--height 480] [--width 640] [--voxels 1.0 0.5] [--runs 5] [--no-torch]

The depth maps are those of the 49-view 640 x 480 synthetic scan of tools/microbench_fusion.py (a tilted plane at depth
600, noise 0.3), with its random colours; the volume is ``volume_bounds`` of them grown by ``trunc = 4 voxel``.  Per voxel
size every C-ABI entry is timed on its own (HIP events around the call on its stream, ``_lib.KernelTimer``; one warm-up
call, then the median of ``--runs``), the integration apart from the extraction, next to the whole ``integrate`` call and
the whole ``extract_mesh`` call on the volume's precomputed ``tsdf()``, ``weight()`` and ``colour()`` (events around the
Python call, ended by a synchronisation; ``extract_mesh`` includes torch's cumsum and sorted unique and two host
synchronisations); ``accessors_ms`` is what ``TSDFVolume.extract`` adds to that, the three accessors (elementwise torch over
the whole state).  ``sample_views_per_s`` is samples x views over the integration kernel's time; ``gathered_bytes_per_s``
counts 4 bytes for every (sample, view) that reads a depth (``gathers``) and 3 more for every one that also reads a colour,
``|sdf| <= trunc`` (``colour_reads``), both counted by the torch route: the bytes the kernel asks for, not what the memory
system moves.  The torch-only route on the same GPU is the same
specification with library operators, without colour: per view a matmul projection, ``floor``, a gather and masked
updates.  Its float arithmetic is the library's, so ``torch_weight_equal_share`` and ``torch_tsdf_max_abs_diff`` say how
far the two agree.  Prints one JSON line per voxel size and appends it to profiles/tsdf_microbench.jsonl.
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


def torch_route(origin, voxel, dims, depths, proj, trunc, depth_min=1e-3, depth_max=1e5):
    """``(S, W, gathers, colour_reads)`` of the integration with library operators (no colour sums); ``gathers`` = (sample,
    view) pairs that read a depth, ``colour_reads`` = those of them that would also read a colour (step 6)."""
    dev = depths.device
    V, h, w = depths.shape
    axes = [origin[a] + torch.arange(dims[a], device=dev, dtype=torch.float32) * voxel for a in range(3)]
    Z, Y, X = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    pos = torch.stack([X, Y, Z], dim=-1).view(-1, 3)
    P = proj.view(V, 3, 4)
    S = torch.zeros(pos.shape[0], device=dev)
    W = torch.zeros(pos.shape[0], dtype=torch.int32, device=dev)
    gathers = torch.zeros((), dtype=torch.int64, device=dev)
    colour_reads = torch.zeros((), dtype=torch.int64, device=dev)
    for v in range(V):
        q = pos @ P[v, :, :3].t() + P[v, :, 3]
        z = q[:, 2]
        ok = (z > depth_min) & (z < depth_max)
        zs = torch.where(ok, z, torch.ones_like(z))
        u, t = q[:, 0] / zs, q[:, 1] / zs
        ok &= (u >= 0) & (u < w) & (t >= 0) & (t < h)
        pix = torch.where(ok, torch.floor(t).long() * w + torch.floor(u).long(), torch.zeros_like(W, dtype=torch.int64))
        gathers += ok.sum()
        d = depths[v].reshape(-1)[pix]
        sdf = d - z
        ok &= (d > depth_min) & (d < depth_max) & ~(sdf < -trunc)
        colour_reads += (ok & (sdf.abs() <= trunc)).sum()
        S += torch.where(ok, torch.clamp(sdf, max=trunc) / trunc, torch.zeros_like(S))
        W += ok
    return S, W, gathers, colour_reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--voxels", type=float, nargs="+", default=[1.0, 0.5])
    ap.add_argument("--min-weight", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import _lib, render, tsdf
    V, h, w = args.views, args.height, args.width
    depths_np, K, E, images_np = make_scan(V, h, w)
    dev = torch.device(args.device)
    depths, images = torch.from_numpy(depths_np).to(dev), torch.from_numpy(images_np).to(dev)
    proj = torch.from_numpy(render.world_maps(K, E)).to(dev)
    n = np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    plane_c = n @ np.array([0.0, 0.0, 600.0])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for voxel in args.voxels:
        trunc = 4.0 * voxel
        origin, dims = tsdf.dims_for(tsdf.volume_bounds(depths, K, E, pad=trunc), voxel)
        samples = dims[0] * dims[1] * dims[2]
        timer = _lib.KernelTimer()
        _lib.set_timer(timer)
        integrate_ms, extract_ms, accessors_ms = [], [], []
        for run in range(args.runs + 1):                                            # the first is the warm-up
            vol = tsdf.TSDFVolume(origin, voxel, dims, trunc, with_colour=True, device=dev)
            vol.tsdf()                                                              # allocate outside the timed call
            torch.cuda.synchronize()
            integrate_ms.append(event_ms(lambda: vol.integrate(depths, K, E, images=images))[0])
            ms, state = event_ms(lambda: (vol.tsdf(), vol.weight(), vol.colour()))
            accessors_ms.append(ms)
            ms, mesh = event_ms(lambda: tsdf.extract_mesh(state[0], state[1], origin, voxel, args.min_weight, state[2]))
            extract_ms.append(ms)
        _lib.set_timer(None)
        torch.cuda.synchronize()
        kernels = {}
        for name, e0, e1, _, _, _ in timer.records:
            kernels.setdefault(name, []).append(e0.elapsed_time(e1))
        kernel_ms = {name: median(ms[1:]) for name, ms in kernels.items()}
        vertices, faces, colours, keys = mesh
        off = (vertices.double().cpu().numpy() @ n - plane_c) if len(vertices) else np.zeros(1)
        again = vol.extract(args.min_weight)
        out = {"views": V, "height": h, "width": w, "voxel": voxel, "trunc": trunc, "dims": list(dims), "samples": samples,
               "runs": args.runs, "min_weight": args.min_weight, "with_colour": True,
               "state_bytes": samples * 24, "integrate_kernel_ms": kernel_ms["pf_tsdf_integrate_f32"],
               "integrate_call_ms": median(integrate_ms[1:]),
               "sample_views_per_s": samples * V / (kernel_ms["pf_tsdf_integrate_f32"] * 1e-3),
               "count_kernel_ms": kernel_ms.get("pf_tsdf_count_triangles"), "emit_kernel_ms": kernel_ms.get("pf_tsdf_emit_triangles"),
               "vertex_kernel_ms": kernel_ms.get("pf_tsdf_vertices_f32"), "extract_mesh_call_ms": median(extract_ms[1:]),
               "accessors_ms": median(accessors_ms[1:]),
               "vertices": int(vertices.shape[0]), "faces": int(faces.shape[0]),
               "vertex_plane_distance_max": float(np.abs(off).max()), "vertex_plane_distance_mean": float(np.abs(off).mean()),
               "two_extractions_equal": bool(torch.equal(again[0], vertices) and torch.equal(again[1], faces))}
        if not args.no_torch:
            torch_route(origin, voxel, dims, depths, proj, trunc)                   # warm-up
            times = []
            for _ in range(max(1, args.runs // 2)):
                ms, (S, W, gathers, colour_reads) = event_ms(lambda: torch_route(origin, voxel, dims, depths, proj, trunc))
                times.append(ms)
            gathers, colour_reads = int(gathers), int(colour_reads)
            ref = torch.where(W > 0, S / W.float(), torch.ones_like(S)).view(vol.S.shape)
            same = W.view(vol.W.shape) == vol.W
            out.update(torch_route_ms=median(times), gathers=gathers, colour_reads=colour_reads,
                       gathered_bytes_per_s=(4 * gathers + 3 * colour_reads) / (kernel_ms["pf_tsdf_integrate_f32"] * 1e-3),
                       torch_weight_equal_share=float(same.float().mean()),
                       torch_tsdf_max_abs_diff=float((ref - vol.tsdf())[same].abs().max()))
        line = json.dumps(out)
        print(line, flush=True)
        with open(os.path.join(ROOT, "profiles", "tsdf_microbench.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
