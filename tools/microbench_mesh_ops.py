"""Time the mesh clean-up and scoring kernels (pointmvsnet_amd/mesh_ops.py, csrc/mesh_ops.hip) on a DTU-sized TSDF mesh.

    python tools/microbench_mesh_ops.py [--views 49] [--height 480] [--width 640] [--voxels 1.0 0.5] [--pitch 0.2] [--runs 5]
                                        [--no-orientation]

The mesh is ``TSDFVolume.extract`` of the 49-view 640 x 480 synthetic scan of tools/microbench_tsdf.py (a tilted plane at
depth 600, noise 0.3) at every ``--voxels`` pitch.  Per mesh, after one warm-up, the median of ``--runs`` of HIP-event
times (events on the stream around the call, ended by a synchronisation):

* connected components: the whole ``mesh_components`` call, its ``rounds``, and the call taken apart -- the hook launches,
  the compress launches (event pairs around each launch, ``_lib.KernelTimer``) and the host's flag reads (wall clock around
  the ``int(flag)`` of every round, which is where the host waits for the round's two launches);
* ``remove_small_components(min_faces=--min-faces)`` (components again, torch's unique / sort / cumsum and the gathers);
* ``vertex_normals`` (the whole call, and its kernel apart from torch's stable sort that builds the corner table);
* ``sample_surface`` at ``--pitch`` (the whole call, the count and the emit kernel).

For orientation, unless ``--no-orientation``: ``scipy.sparse.csgraph.connected_components`` on the host on the same faces
(the CPU step this replaces; wall clock, the transfer of the faces not included) and a torch-only normal route on the
same GPU -- float32 face normals scattered with three ``index_add_`` calls and normalised, whose atomics sum in no fixed
order, so it is a yardstick for time and not for bits (``torch_normals_max_abs_diff`` says how far the two agree).
Prints one JSON line per voxel size and appends it to profiles/mesh_ops_microbench.jsonl.
"""
import argparse
import json
import os
import sys
import time

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


def torch_normals(vertices, faces):
    """Area-weighted vertex normals with library operators: float32 throughout, three index_add_ scatters."""
    f = faces.long()
    pa, pb, pc = vertices[f[:, 0]], vertices[f[:, 1]], vertices[f[:, 2]]
    n = torch.cross(pb - pa, pc - pa, dim=1)
    n = torch.where(torch.isfinite(n).all(dim=1, keepdim=True), n, torch.zeros_like(n))
    s = torch.zeros_like(vertices)
    for k in range(3):
        s.index_add_(0, f[:, k], n)
    length = s.norm(dim=1, keepdim=True)
    return torch.where(length > 0, s / length.clamp(min=1e-30), torch.zeros_like(s))


def scipy_components_ms(faces_np, nv):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    rows = np.concatenate([faces_np[:, 0], faces_np[:, 1]])
    cols = np.concatenate([faces_np[:, 1], faces_np[:, 2]])
    count, _ = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nv, nv)), directed=False)
    return (time.perf_counter() - t0) * 1e3, int(count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--voxels", type=float, nargs="+", default=[1.0, 0.5])
    ap.add_argument("--min-weight", type=int, default=2)
    ap.add_argument("--min-faces", type=int, default=100)
    ap.add_argument("--pitch", type=float, default=0.2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-orientation", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    from microbench_fusion import make_scan
    from pointmvsnet_amd import _lib, mesh_ops, tsdf
    V, h, w = args.views, args.height, args.width
    depths_np, K, E, images_np = make_scan(V, h, w)
    dev = torch.device(args.device)
    depths, images = torch.from_numpy(depths_np).to(dev), torch.from_numpy(images_np).to(dev)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for voxel in args.voxels:
        trunc = 4.0 * voxel
        origin, dims = tsdf.dims_for(tsdf.volume_bounds(depths, K, E, pad=trunc), voxel)
        vol = tsdf.TSDFVolume(origin, voxel, dims, trunc, with_colour=True, device=dev)
        vol.integrate(depths, K, E, images=images)
        vertices, faces, colours, _ = vol.extract(args.min_weight)
        del vol
        nv, nf = int(vertices.shape[0]), int(faces.shape[0])
        read_ms = []
        real_components = mesh_ops._components

        def timed_components(faces32, Nv):                     # the module's loop with a clock around every flag read
            label = torch.arange(Nv, dtype=torch.int32, device=faces32.device)
            flags = torch.zeros((mesh_ops._FLAGS,), dtype=torch.int32, device=faces32.device)
            rounds, waited = 0, 0.0
            while Nv and faces32.shape[0]:
                flag = flags[rounds % mesh_ops._FLAGS:]
                mesh_ops._cc_hook(faces32, Nv, label, flag)
                mesh_ops._cc_compress(label)
                rounds += 1
                t0 = time.perf_counter()
                changed = int(flag[0])
                waited += time.perf_counter() - t0
                if not changed or rounds == mesh_ops._FLAGS:
                    break
            read_ms.append(waited * 1e3)
            return label, rounds

        calls = {"components": [], "removal": [], "normals": [], "sampling": []}
        timer = _lib.KernelTimer()
        for run in range(args.runs + 1):                        # the first is the warm-up
            torch.cuda.synchronize()
            ms, (vl, fl, rounds) = event_ms(lambda: mesh_ops.mesh_components(faces, nv, return_rounds=True))
            calls["components"].append(ms)
            ms, removed = event_ms(lambda: mesh_ops.remove_small_components(vertices, faces, min_faces=args.min_faces,
                                                                            colours=colours))
            calls["removal"].append(ms)
            _lib.set_timer(timer)                               # the launches on their own: event pairs around each
            mesh_ops._components = timed_components
            try:
                mesh_ops.mesh_components(faces, nv)
            finally:
                mesh_ops._components = real_components
            ms, normals = event_ms(lambda: mesh_ops.vertex_normals(vertices, faces))
            calls["normals"].append(ms)
            ms, samples = event_ms(lambda: mesh_ops.sample_surface(vertices, faces, args.pitch))
            calls["sampling"].append(ms)
            _lib.set_timer(None)
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

        labels, counts = mesh_ops.component_sizes(fl)
        out = {"views": V, "height": h, "width": w, "voxel": voxel, "dims": list(dims), "vertices": nv, "faces": nf,
               "runs": args.runs, "components": int(labels.numel()), "largest_component_faces": int(counts.max()) if nf else 0,
               "rounds": rounds, "components_call_ms": median(calls["components"][1:]),
               "hook_launches_ms": kernel_ms("pf_mesh_cc_hook"), "compress_launches_ms": kernel_ms("pf_mesh_cc_compress"),
               "face_labels_kernel_ms": kernel_ms("pf_mesh_face_labels"), "host_flag_reads_ms": median(read_ms[1:]),
               "min_faces": args.min_faces, "removal_call_ms": median(calls["removal"][1:]),
               "faces_after_removal": int(removed[1].shape[0]), "vertices_after_removal": int(removed[0].shape[0]),
               "normals_call_ms": median(calls["normals"][1:]), "normals_kernel_ms": kernel_ms("pf_mesh_vertex_normals_f32"),
               "normals_undefined": int((normals == 0).all(dim=1).sum()),
               "pitch": args.pitch, "samples": int(samples[0].shape[0]), "sampling_call_ms": median(calls["sampling"][1:]),
               "sample_count_kernel_ms": kernel_ms("pf_mesh_sample_count_f32"),
               "sample_emit_kernel_ms": kernel_ms("pf_mesh_sample_emit_f32")}
        if not args.no_orientation:
            faces_np = faces.cpu().numpy().astype(np.int64)
            host = [scipy_components_ms(faces_np, nv) for _ in range(3)]
            torch_normals(vertices, faces)                      # warm-up
            times = []
            for _ in range(args.runs):
                ms, ref = event_ms(lambda: torch_normals(vertices, faces))
                times.append(ms)
            out.update(scipy_components_ms=median([m for m, _ in host]), scipy_components=host[0][1],
                       torch_normals_ms=median(times), torch_normals_max_abs_diff=float((ref - normals).abs().max()))
        line = json.dumps(out)
        print(line, flush=True)
        with open(os.path.join(ROOT, "profiles", "mesh_ops_microbench.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
