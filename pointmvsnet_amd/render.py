"""Rendering a point cloud into the depth maps of its views on the GPU, and per-view depth errors against such maps.

The inverse of ``fusion.depth_to_points`` and of the fusers' back-projection: a cloud and cameras in, one depth map per view
out.  The reference scores depth maps only against ground-truth depth maps (``PointMVSNetMetric`` on ``gt_depth_img``);
DTU's test scans ship a ground-truth *cloud* and no depth maps, so there a bad accuracy / completeness pair cannot be traced
to a view, a stage or a filter.  Rendering the ground-truth cloud into the accumulated views gives every view the map that
``depth_map_errors`` scores its raw and filtered predictions against, and rendering a fused cloud back into its views shows
what survived the fusion.  The reference has no such step, so **the specification below is this project's own**; it runs as
two HIP kernels (csrc/cloud_render.hip).  Pixel centres are at ``(x + 0.5, y + 0.5)``, as everywhere else in this pipeline
(``fusion.py``), so the pixel that contains an image position ``(u, v)`` is ``(floor(u), floor(v))``.

The splat
---------
``proj[v] = K_v [R_v | t_v]`` (3 x 4, row-major ``p0 .. p11``) is composed in float64 and handed to the kernel as float32
(``world_maps``).  A 64-bit cell per pixel of every view starts as all-ones.  Per point ``n = (X, Y, Z)`` and view ``v``, in
float32 with exactly this operation order (no fused multiply-add):

1. ``qx = ((p0 X + p1 Y) + p2 Z) + p3``, ``qy = ((p4 X + p5 Y) + p6 Z) + p7``, ``z = ((p8 X + p9 Y) + p10 Z) + p11``.
2. Skip unless ``depth_min < z < depth_max``.  This is false for NaN.
3. ``u = qx / z``, ``v = qy / z``.  Skip unless ``-splat <= u < w + splat`` and ``-splat <= v < h + splat``.
4. ``(xc, yc) = (floor(u), floor(v))``, the pixel that contains the projection.
5. Every pixel ``(x, y)`` of the map with ``|x - xc| <= splat`` and ``|y - yc| <= splat`` takes
   ``cell = min(cell, (float_bits(z) << 32) | n)`` as an unsigned 64-bit minimum.

``z > 0``, so its bit pattern orders like its value: **the nearest point wins, and among points of bit-equal** ``z`` **the
lowest index**.  A minimum does not depend on the order of arrival, so the result is a pure function of the input: two
runs give identical bytes, and a permuted cloud gives the same depth map.  The depth map is the winner's ``z`` (0 where no
point landed), the index map its row in ``points`` (-1 where none).  ``splat`` is a square radius in pixels, 0 to 8: 0 fills
only the pixel that contains the projection; 1 closes the gaps of a cloud sampled about as densely as the pixels, at the
price of a silhouette grown by one pixel.

Non-finite coordinates are not an error: such a point fails the tests of steps 2 and 3 in every view and writes nothing.
The defaults ``depth_min=1e-3`` and ``depth_max=1e5`` are the fusers'.

Depth errors
------------
``depth_map_errors(pred, gt, thresholds)``: a pixel is *compared* where ``gt > 0`` and ``pred > 0``; its error is
``|pred - gt|`` in the maps' own precision.  Per view and in total: ``n_gt`` (pixels with ``gt > 0``), ``n_pred``,
``n_compared``, ``coverage = n_compared / n_gt``, ``abs_err_mean`` (a float64 sum over the compared pixels),
``abs_err_median`` (the lower median, as in ``evaluation.py``) and ``within[k] = #(error < thresholds[k]) / n_compared``
(the comparison in float64).  A ratio or score over an empty set is ``nan``.

Out of scope
------------
Mesh rasterisation; hole filling; any suppression of points seen "through" the gaps of a nearer surface beyond what the
splat radius closes; rendering colours; wiring a ground-truth cloud into ``DTUDataset``.
"""
import numpy as np
import torch

from . import _lib, camera_maps as cm

_WHO = "render_depth_maps"
PROJ_FLOATS, MAX_SPLAT, MAX_POINTS = 12, 8, 2 ** 32 - 2   # PF_RENDER_* of include/pointflow_hip.h


def world_maps(intrinsics, extrinsics):
    """``(V, 12)`` float32: ``K [R | t]`` row-major of ``intrinsics`` (V, 3, 3) and ``extrinsics`` (V, 3, 4) or (V, 4, 4),
    composed in float64, one view per step (a form vectorised over the views rounds differently: ``camera_maps.pair_row``)."""
    return _world_maps(cm.decompose("world_maps", intrinsics, extrinsics))


def _world_maps(cams):
    K, R, t = cams[:3]
    out = np.zeros((K.shape[0], PROJ_FLOATS))
    for v in range(K.shape[0]):
        out[v] = (K[v] @ np.concatenate([R[v], t[v][:, None]], axis=1)).reshape(PROJ_FLOATS)
    return out.astype(np.float32)


def render_depth_maps(points, intrinsics, extrinsics, height, width, splat=0, depth_min=1e-3, depth_max=1e5,
                      return_index=False):
    """Render ``points`` (N, 3) float32 on the GPU into the ``height`` x ``width`` depth maps of the cameras ``intrinsics``
    (V, 3, 3, of that grid) and ``extrinsics`` (V, 3, 4) or (V, 4, 4) by the specification in this module's docstring.

    Returns ``depth`` (V, h, w) float32 on the device of ``points``, 0 where no point lands; with ``return_index`` also the
    int64 (V, h, w) map of the winning points' rows, -1 where empty.  Works on the current stream without a host
    synchronisation; a non-finite point is skipped, not reported.  There is no CPU path."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("%s: points must be an (N, 3) float32 tensor" % _WHO)
    h, w, splat = int(height), int(width), int(splat)
    if h != height or w != width or h < 0 or w < 0:
        raise ValueError("%s: height and width must be non-negative integers" % _WHO)
    if not 0 <= splat <= MAX_SPLAT:
        raise ValueError("%s: splat must be in [0, %d]" % (_WHO, MAX_SPLAT))
    N = int(points.shape[0])
    if N > MAX_POINTS:
        raise ValueError("%s: at most 2^32 - 2 points" % _WHO)
    proj = _world_maps(cm.decompose(_WHO, intrinsics, extrinsics))
    V = int(proj.shape[0])
    if h * w > (2 ** 31 - 1) // 4 or V > 65535:
        raise ValueError("%s: %d maps of %d x %d are outside what the kernel is built for" % (_WHO, V, h, w))
    _lib.require_gpu(points)
    dev = points.device
    with _lib.on_device(dev):
        depth = torch.zeros((V, h, w), dtype=torch.float32, device=dev)
        index = torch.full((V, h, w), -1, dtype=torch.int64, device=dev) if return_index else None
        if N and V and h and w:
            points = points.contiguous()
            proj = torch.from_numpy(proj).to(dev)
            zbuf = torch.full((V, h, w), -1, dtype=torch.int64, device=dev)       # all-ones, on the stream of the launch
            # the cloud once, a cell read and written per view; the atomics beyond that depend on the scene
            _lib.call("pf_cloud_splat_f32", _lib.ptr(points), N, _lib.ptr(proj), V, h, w, splat, float(depth_min),
                      float(depth_max), _lib.ptr(zbuf), _lib.stream(), algo_bytes=12 * N + 16 * V * h * w)
            index32 = torch.empty((V, h, w), dtype=torch.int32, device=dev) if return_index else None
            _lib.call("pf_cloud_zbuf_decode", _lib.ptr(zbuf), V, h, w, _lib.ptr(depth), _lib.ptr(index32), _lib.stream(),
                      algo_bytes=V * h * w * (8 + 4 + (4 if return_index else 0)))
            if return_index:
                index = index32.to(torch.int64)
                if N > 2 ** 31:                                                   # rows past 2^31 - 1 come back as bit patterns
                    index = torch.where(index < -1, index + 2 ** 32, index)
    return (depth, index) if return_index else depth


def _row(err, n_gt, n_pred, thresholds):
    """One row of ``depth_map_errors`` from the 1-D errors of the compared pixels."""
    n = int(err.numel())
    nan = float("nan")
    err64 = err.double()
    return {"n_gt": n_gt, "n_pred": n_pred, "n_compared": n, "coverage": n / float(n_gt) if n_gt else nan,
            "abs_err_mean": float(err64.sum() / n) if n else nan, "abs_err_median": float(torch.median(err)) if n else nan,
            "within": [float((err64 < t).sum()) / n if n else nan for t in thresholds]}


def depth_map_errors(pred, gt, thresholds):
    """Score the depth maps ``pred`` (V, h, w) against ``gt`` (V, h, w) (0 = no depth in either) by the rules of this
    module's docstring; ``thresholds`` is a sequence of lengths in the maps' units.  Plain torch on the maps' device (CPU
    tensors work).  Returns ``{"thresholds": [...], "per_view": [row, ...], "total": row}`` of Python numbers and lists, a
    row being ``n_gt``, ``n_pred``, ``n_compared``, ``coverage``, ``abs_err_mean``, ``abs_err_median`` and ``within`` (one
    share per threshold, in their order)."""
    if not isinstance(pred, torch.Tensor) or not isinstance(gt, torch.Tensor) or pred.dim() != 3 or pred.shape != gt.shape:
        raise ValueError("depth_map_errors: pred and gt must be (V, h, w) tensors of one shape")
    thresholds = [float(t) for t in thresholds]
    gt = gt.to(pred.device)
    has_gt, has_pred = gt > 0, pred > 0
    compared = has_gt & has_pred
    err = (pred - gt).abs()
    n_gt, n_pred = has_gt.flatten(1).sum(1).tolist(), has_pred.flatten(1).sum(1).tolist()
    rows = [_row(err[v][compared[v]], int(n_gt[v]), int(n_pred[v]), thresholds) for v in range(int(pred.shape[0]))]
    return {"thresholds": thresholds, "per_view": rows, "total": _row(err[compared], int(sum(n_gt)), int(sum(n_pred)), thresholds)}
