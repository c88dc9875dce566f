"""Time the two routes from decoded uint8 views to ``img_list`` on the GPU (pointmvsnet_amd/utils/preprocess.py).

    python tools/microbench_preprocess.py [--runs 20] [--host-runs 3]

Per configuration -- cfg 2: 3 views of 1600 x 1200 -> 640 x 512 at the scale the loader chooses (512/1200, cropped from
683 columns); cfg 5: 7 views of 1600 x 1200 -> 1600 x 1152 at scale 1 -- on seeded uniform uint8 images:

  (a) the host route: NumPy resize + crop + float32 standardisation (``preprocess_views`` without a device; wall clock,
      median of ``--host-runs``), then the float32 ``img_list`` from pinned memory to the GPU (HIP events);
  (b) the uint8 views from pinned memory to the GPU and the two kernels of csrc/preprocess.hip, timed together by one
      HIP event pair, plus the upload alone and the kernels alone (medians of ``--runs`` after 3 warm-up runs).

Prints one JSON line: the times, the kernels' algorithmic bytes per second against the measured-copy figure of
BASELINE.md section 4 (6.29 TB/s) and, if ``cv2`` is importable, the largest grey-level difference and the share of
differing values of ``resize_linear`` against ``cv2.resize(..., interpolation=cv2.INTER_LINEAR)`` on one view.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BYTES_PER_S = 6.29e12          # measured device copy
CONFIGS = {"cfg2": (3, 512, 640), "cfg5": (7, 1152, 1600)}
SRC_H, SRC_W, BASE = 1200, 1600, 64


def _median(vals):
    return sorted(vals)[len(vals) // 2]


def _event_ms(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return _median(out)


def measure(name, runs, host_runs):
    from pointmvsnet_amd.utils import preprocess as P
    V, height, width = CONFIGS[name]
    dev = torch.device("cuda:0")
    scale = max(float(height) / SRC_H, float(width) / SRC_W)
    views = np.random.default_rng(V).integers(0, 256, (V, SRC_H, SRC_W, 3), dtype=np.uint8)
    # (a) host preprocessing, then 12 bytes per pixel over PCIe
    host = []
    for _ in range(host_runs):
        t0 = time.perf_counter()
        img_host, _, _ = P.preprocess_views(views, scale, height, width, BASE)
        host.append((time.perf_counter() - t0) * 1e3)
    pinned_f32 = img_host.pin_memory()
    on_dev_f32 = torch.empty_like(img_host, device=dev)
    a_upload = _event_ms(lambda: on_dev_f32.copy_(pinned_f32, non_blocking=True), runs)
    # (b) 3 bytes per pixel over PCIe, then the kernels
    pinned_u8 = torch.from_numpy(views).pin_memory()
    on_dev_u8 = torch.empty_like(pinned_u8, device=dev)
    b_upload = _event_ms(lambda: on_dev_u8.copy_(pinned_u8, non_blocking=True), runs)
    b_kernels = _event_ms(lambda: P.preprocess_views_gpu(on_dev_u8, scale, height, width, BASE), runs)

    def route_b():
        on_dev_u8.copy_(pinned_u8, non_blocking=True)
        return P.preprocess_views_gpu(on_dev_u8, scale, height, width, BASE)

    b_total = _event_ms(route_b, runs)
    img_dev, _, _ = route_b()
    H, W = int(img_dev.shape[2]), int(img_dev.shape[3])
    algo = V * 3 * SRC_H * SRC_W + V * H * W * (3 + 3 + 12)
    gap = float((img_dev.cpu() - img_host).abs().max())
    return {"views": V, "src": [SRC_H, SRC_W], "out": [H, W], "scale": scale,
            "a_host_numpy_ms": _median(host), "a_upload_f32_ms": a_upload, "a_total_ms": _median(host) + a_upload,
            "b_upload_u8_ms": b_upload, "b_kernels_ms": b_kernels, "b_total_ms": b_total,
            "b_over_a": b_total / (_median(host) + a_upload),
            "kernels_algo_bytes": algo, "kernels_bytes_per_s": algo / (b_kernels * 1e-3),
            "kernels_share_of_copy": algo / (b_kernels * 1e-3) / COPY_BYTES_PER_S,
            "max_abs_gpu_minus_host_img_list": gap}


def against_opencv():
    try:
        import cv2
    except ImportError:
        return None
    from pointmvsnet_amd.utils import preprocess as P
    view = np.random.default_rng(0).integers(0, 256, (SRC_H, SRC_W, 3), dtype=np.uint8)
    out = {}
    for scale in (0.8, 512.0 / 1200.0):
        ours = P.resize_linear(view, scale)
        theirs = cv2.resize(view, None, fx=scale, fy=scale, interpolation=cv2.INTER_LINEAR)
        if ours.shape != theirs.shape:
            out["%.4f" % scale] = {"shapes": [list(ours.shape), list(theirs.shape)]}
            continue
        diff = np.abs(ours.astype(int) - theirs.astype(int))
        out["%.4f" % scale] = {"max_grey_levels": int(diff.max()), "share_differing": float((diff != 0).mean())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "microbench_preprocess.py needs a GPU"
    out = {"tool": "microbench_preprocess", "device": torch.cuda.get_device_name(0), "copy_bytes_per_s": COPY_BYTES_PER_S}
    for name in CONFIGS:
        out[name] = measure(name, args.runs, args.host_runs)
    out["resize_vs_opencv"] = against_opencv()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
