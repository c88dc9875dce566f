"""Depth-map fusion on the GPU: the filtered depth maps of all views of a scan -> one point cloud.

The reference ends its pipeline by converting its files for ``fusibile``, an external CUDA program, and running it
(reference tools/depthfusion.py:173-192).  There is no fusibile for ROCm, so this module states the step itself and runs it
as HIP kernels (csrc/fusion.hip).  **The specification below is this project's own**: it is modelled on the parameters
depthfusion.py passes to fusibile (``disp_thresh``, ``num_consistent``, ``depth_min``, ``depth_max``); bit parity with
fusibile is neither claimed nor tested.  Known departures from what is known of fusibile:

* pixel ``(x, y)`` has its centre at ``(x + 0.5, y + 0.5)`` -- the convention of ``get_pixel_grids`` and of
  ``eval_file_logger.depth_to_points``, so an unfused point equals the matching row of the ``.xyz`` file the logger
  writes -- where fusibile uses integer centres;
* the partner pixel is the one that CONTAINS the projection (floor), its depth is not interpolated;
* no normal test (the reference disables it with ``normal_thresh=360``); the normals that ``with_normals=True`` adds to
  the cloud are those of ``normals.py``, estimated from the depth maps and never compared between views;
* the output order is fixed: view-major, then row-major.  Two runs give identical bytes.

Stage A, per reference view ``i`` and pixel ``p = (x, y)`` with ``depth_min < d_i(p) < depth_max``:

1. ``X = R_i^-1 (K_i^-1 (x + 0.5, y + 0.5, 1) d_i(p) - t_i)``.
2. For every other view ``j`` in ascending order: ``q = K_j (R_j X + t_j)``, ``z = q.z``, ``(xj, yj) = floor(q.xy / z)``;
   skip ``j`` if ``z <= 0``, ``(xj, yj)`` is outside the map or ``d_j(xj, yj)`` is not inside ``(depth_min, depth_max)``.
3. With ``f_j = K_j[0, 0]`` and ``b_ij = |C_i - C_j|`` (camera centres ``C = -R^-1 t``), ``j`` is *consistent* iff
   ``|f_j b_ij / z - f_j b_ij / d_j(xj, yj)| < disp_threshold``.
4. A consistent ``j`` contributes ``X_j``, the back-projection of the centre of ``(xj, yj)`` at ``d_j(xj, yj)``, and the
   match ``yj * w + xj`` (else ``-1``).
5. ``count`` = consistent views, ``point`` = mean of ``X`` and the consistent ``X_j`` (summed in ascending ``j``),
   ``colour`` likewise (rounded to the nearest byte at the end).

Stage B, sequential over the views: pixel ``p`` of view ``i`` emits iff no earlier view has claimed it and
``count >= num_consistent``; an emitting pixel claims its matches.  The emitted points are compacted in order.

The matrices of every view pair are composed here in float64 and handed to the kernels as float32.
"""
import os.path as osp

import numpy as np
import torch

from . import _lib, camera_maps as cm, normals as nm
from .camera_maps import PAIR_FLOATS, VIEW_FLOATS  # noqa: F401
from .utils.io import load_cam_dtu, load_pfm, write_ply

def camera_maps(intrinsics, extrinsics):
    """``(view_maps (V, 12), pair_maps (V, V, 16))`` float32 arrays in the layout of ``pf_fuse_stage_a_f32``, composed in
    float64 from ``intrinsics`` (V, 3, 3) and ``extrinsics`` (V, 3, 4) or (V, 4, 4) (world -> camera)."""
    return _maps_of(cm.decompose("fuse_depth_maps", intrinsics, extrinsics))


def _maps_of(cams):
    V = cams[0].shape[0]
    pair_maps = np.zeros((V, V, PAIR_FLOATS))
    for i, j in np.ndindex(V, V):
        cm.pair_row(cams, i, j, pair_maps[i, j], with_fb=True)
    return cm.view_maps(cams), pair_maps.astype(np.float32)


def fuse_depth_maps(depths, intrinsics, extrinsics, images=None, disp_threshold=0.12, num_consistent=3, depth_min=1e-3,
                    depth_max=1e5, return_stages=False, with_normals=False, normal_step=1, normal_rel_jump=0.01):
    """Fuse ``depths`` (V, h, w) float32 on the GPU (0 = no depth; a sequence of (h, w) maps is stacked, maps of different
    sizes are an error, as in fusibile) with cameras ``intrinsics`` (V, 3, 3, of that h x w grid) and ``extrinsics``
    (V, 3, 4) or (V, 4, 4), optionally ``images`` (V, h, w, 3) uint8, by the specification in this module's docstring.

    Returns ``(points (N, 3) float32, colours (N, 3) uint8 or None)`` on the device of ``depths``; with
    ``return_stages`` a third value, the dict of the Stage A tensors ``count`` (V, h, w) int32, ``point`` (V, h, w, 3),
    ``colour`` (V, h, w, 3) or None, ``match`` (V, V-1, h, w) int32 and the Stage B mask ``emit`` (V, h, w) bool.
    With ``with_normals`` the points' unit normals (N, 3) float32 follow ``colours`` (``(0, 0, 0)`` where undefined), from
    ``normals.depth_normals(depths, ..., step=normal_step, rel_jump=normal_rel_jump)`` summed over a point's matches
    (``normals.py``), and the stages gain those maps as ``normal`` (V, h, w, 3).  There is no CPU path."""
    if with_normals:
        normal_step, normal_rel_jump = nm.check_step("fuse_depth_maps", normal_step, normal_rel_jump)
    depths, images, V, h, w, dev = cm.normalise_inputs("fuse_depth_maps", depths, images, num_consistent)
    maps = _maps_of(cm.decompose("fuse_depth_maps", intrinsics, extrinsics, V))
    with _lib.on_device(dev):
        view_maps, pair_maps = (torch.from_numpy(a).to(dev) for a in maps)
        count = torch.empty((V, h, w), dtype=torch.int32, device=dev)
        point = torch.empty((V, h, w, 3), dtype=torch.float32, device=dev)
        colour = torch.empty((V, h, w, 3), dtype=torch.uint8, device=dev) if images is not None else None
        match = torch.empty((V, max(V - 1, 0), h, w), dtype=torch.int32, device=dev)
        # per pixel: its own depth, V-1 gathered depths, the outputs (count, point, V-1 matches) and the colours
        algo = V * h * w * (4 * V + 16 + 4 * (V - 1) + (3 * V + 3 if images is not None else 0))
        _lib.call("pf_fuse_stage_a_f32", _lib.ptr(depths), _lib.ptr(images), _lib.ptr(view_maps), _lib.ptr(pair_maps),
                  V, h, w, float(disp_threshold), float(depth_min), float(depth_max), _lib.ptr(count), _lib.ptr(point),
                  _lib.ptr(colour), _lib.ptr(match), _lib.stream(), algo_bytes=algo)
        used = torch.zeros((V, h, w), dtype=torch.uint8, device=dev)
        emit = torch.empty((V, h, w), dtype=torch.uint8, device=dev)
        for i in range(V):
            _lib.call("pf_fuse_mark", _lib.ptr(count), _lib.ptr(match), _lib.ptr(used), _lib.ptr(emit), V, i, h, w,
                      int(num_consistent), _lib.stream())
        points, colours = cm.compact(emit, point, colour)
        if with_normals:
            normal = nm.normal_maps(depths, view_maps, normal_step, normal_rel_jump, depth_min, depth_max)
            normals = nm.fused_normals(normal, match, emit)
    out = (points, colours) + ((normals,) if with_normals else ())
    if not return_stages:
        return out
    stages = {"count": count, "point": point, "colour": colour, "match": match, "emit": emit.bool()}
    if with_normals:
        stages["normal"] = normal
    return out + (stages,)


def _load_image(path, h, w):
    """``path`` as (h, w, 3) uint8 RGB (nearest-resized like reference tools/depthfusion.py:147-149), or None when the file
    or a decoder (OpenCV, else Pillow) is missing."""
    if not osp.exists(path):
        return None
    try:
        import cv2
        img = cv2.imread(path)[:, :, ::-1]
    except ImportError:
        try:
            from PIL import Image
        except ImportError:
            return None
        img = np.asarray(Image.open(path).convert("RGB"))
    if img.shape[:2] != (h, w):
        from .utils.eval_file_logger import _resize_nearest
        img = _resize_nearest(img, h, w)
    return np.ascontiguousarray(img, dtype=np.uint8)


def fuse_scene_folder(scene_folder, name, view_num, disp_threshold=0.12, num_consistent=3, depth_min=1e-3, depth_max=1e5,
                      out_path=None, device=None):
    """Fuse what ``eval_file_logger`` / ``probability_filter`` wrote into ``scene_folder`` for views ``0 .. view_num-1``:
    ``%08d_<name>_prob_filtered.pfm``, ``cam_%08d_<name>.txt`` (its intrinsics are those of the depth map's grid) and, when
    every view has one and a decoder is importable, ``%08d.jpg``.  Writes ``final3d_model.ply`` into the folder (or
    ``out_path``) and returns ``(points, colours)`` as ``fuse_depth_maps`` does."""
    depths, K, E, images = [], [], [], []
    for v in range(view_num):
        depth = load_pfm(osp.join(scene_folder, "{:08d}_{}_prob_filtered.pfm".format(v, name)))[0]
        if depths and depth.shape != depths[0].shape:
            raise ValueError("fuse_scene_folder: view %d is %s, view 0 is %s" % (v, depth.shape, depths[0].shape))
        depths.append(np.ascontiguousarray(depth, dtype=np.float32))
        with open(osp.join(scene_folder, "cam_{:08d}_{}.txt".format(v, name))) as f:
            cam = load_cam_dtu(f)
        E.append(cam[0])
        K.append(cam[1, :3, :3])
        if images is not None:
            img = _load_image(osp.join(scene_folder, "{:08d}.jpg".format(v)), *depth.shape)
            images = None if img is None else images + [img]
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    points, colours = fuse_depth_maps(
        torch.from_numpy(np.stack(depths)).to(dev), np.stack(K), np.stack(E),
        images=None if not images else torch.from_numpy(np.stack(images)).to(dev), disp_threshold=disp_threshold,
        num_consistent=num_consistent, depth_min=depth_min, depth_max=depth_max)
    write_ply(out_path or osp.join(scene_folder, "final3d_model.ply"), points.cpu().numpy(),
              None if colours is None else colours.cpu().numpy())
    return points, colours
