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

Mesh rasterisation
------------------
``render_mesh_depth_maps``: vertices, faces and cameras in, one depth map (and face-index and barycentric map) per view out;
three HIP kernels (csrc/mesh_render.hip) and the decode of the splat.  A surface has neither holes nor gaps that the back
of the scene shows through, and its silhouette is not grown.  The specification is this project's own; parity with OpenGL,
Open3D or nvdiffrast is neither claimed nor tested.

**Screen coordinates.**  ``proj`` is ``world_maps`` as for the splat.  Per vertex ``(X, Y, Z)`` and view, in float32 with
this operation order:

* ``qx``, ``qy``, ``z`` exactly as step 1 of the splat; ``u = qx / z``, ``v = qy / z``.
* The vertex is *valid* in the view iff ``depth_min < z < depth_max`` and ``-G <= u < w + G`` and ``-G <= v < h + G``, tested
  as floats before any conversion (false for NaN).  The guard band is ``G = 16384``.
* Its fixed-point position is ``xi = (int)rintf(u * 256.0f)``, ``yi = (int)rintf(v * 256.0f)``: 8 sub-pixel bits, round half
  to even.
* ``height`` and ``width`` are at most 16384 for this entry point.  Then every coordinate is within 2^23 in magnitude, every
  difference within 2^24 and every edge function within 2^49: **all coverage arithmetic is exact in int64**.

**A face in a view** is rasterised iff all of the following hold; otherwise it writes nothing (no clipping against the near
plane or the guard band; a non-finite vertex is skipped, not reported):

* its three indices lie in ``[0, Nv)`` (a face with another index is never read through);
* its three vertices are valid in that view;
* ``area2 = (bx-ax)(cy-ay) - (by-ay)(cx-ax)`` is not 0.

A face is *front-facing* iff ``area2 < 0``.  With positive focal lengths and the x-right / y-down / z-forward camera frame
this is the winding ``tsdf.extract_mesh`` gives to faces seen from outside.  ``cull=None`` (default) renders both sides,
``cull="back"`` only front-facing faces, ``cull="front"`` only the others.  For ``area2 < 0``, swap ``b`` and ``c`` before
what follows, so ``area2 > 0``.

**Coverage.**  For the oriented edge ``p -> q`` with ``d = q - p``, the edge function at ``s`` is
``E(s) = dx (sy - py) - dy (sx - px)``.  A pixel ``(x, y)`` of the map, with centre ``s = (256 x + 128, 256 y + 128)``, is
covered iff for each of the three edges ``a -> b``, ``b -> c``, ``c -> a``: ``E(s) > 0``, or ``E(s) == 0`` and the edge *owns
its boundary*.  An edge owns its boundary iff ``dy > 0``, or ``dy == 0`` and ``dx < 0``.  Exactly one of ``d`` and ``-d``
owns, so a pixel centre on an edge shared by two faces on opposite sides of it belongs to exactly one of them.  Only pixels
inside the face's bounding box clamped to the map are candidates.

**Depth.**  Let ``Ea``, ``Eb``, ``Ec`` be the edge functions opposite ``a``, ``b``, ``c`` at ``s`` (of ``b -> c``, ``c -> a``,
``a -> b``).  They are non-negative integers and sum to ``area2``.  In float32:

* ``ra = 1.0f / za``, ``rb = 1.0f / zb``, ``rc = 1.0f / zc``;
* ``inv = ((float)Ea * ra + (float)Eb * rb) + (float)Ec * rc``;
* ``z = (float)area2 / inv``.

This is the perspective-correct depth of the (snapped) triangle's plane.  No term is negative, so there is no cancellation
and ``z > 0``.

**Z-buffer.**  The cell takes the unsigned 64-bit minimum of ``(float_bits(z) << 32) | face_index``, as in the splat: the
nearest face wins; among bit-equal depths the lowest face index wins; the result is a pure function of the input.  Two runs
give identical bytes, and a permuted face list gives the same depth map.  At most ``2^32 - 2`` faces.  A face whose clamped
bounding box holds more than ``MESH_LANE_PIXELS`` pixels is walked by a whole wave instead of one lane; the minimum is
order-free, so the result does not depend on that number.

**Barycentrics.**  Where the index map is filled, ``bary = ((float)Ea*ra / inv, (float)Eb*rb / inv, (float)Ec*rc / inv)`` in
the face's *stored* vertex order (the swap undone), else zeros.  They are perspective-correct weights on the face's three
vertices: ``interpolate_vertex_attributes`` turns them into colour or normal maps with plain torch.

Out of scope
------------
Hole filling; any suppression of points seen "through" the gaps of a nearer surface beyond what the splat radius closes;
rendering colours in the splat; wiring a ground-truth cloud into ``DTUDataset``.  For meshes: clipping against the near plane
or the guard band; anti-aliasing, or any sample but the pixel centre; shading; textures beyond per-vertex attributes.
"""
import numpy as np
import torch

from . import _lib, camera_maps as cm

_WHO = "render_depth_maps"
PROJ_FLOATS, MAX_SPLAT, MAX_POINTS = 12, 8, 2 ** 32 - 2   # PF_RENDER_* of include/pointflow_hip.h
MESH_GUARD_BAND, MESH_MAX_SIDE, MESH_MAX_FACES, MESH_LANE_PIXELS = 16384, 16384, 2 ** 32 - 2, 64      # PF_MESH_*
_CULL = {None: 0, "back": 1, "front": 2}                  # PF_MESH_CULL_*


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


def _mesh_arguments(who, vertices, faces, intrinsics, extrinsics, height, width):
    """The checks that need no device: ``(Nv, Nf, h, w, proj float32 (V, 12))``."""
    if (not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3
            or vertices.dtype != torch.float32):
        raise ValueError("%s: vertices must be an (Nv, 3) float32 tensor" % who)
    if faces is not None and (not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3
                              or faces.dtype not in (torch.int32, torch.int64)):
        raise ValueError("%s: faces must be an (Nf, 3) int32 or int64 tensor" % who)
    h, w = int(height), int(width)
    if h != height or w != width or h < 0 or w < 0:
        raise ValueError("%s: height and width must be non-negative integers" % who)
    if h > MESH_MAX_SIDE or w > MESH_MAX_SIDE:
        raise ValueError("%s: height and width must be at most %d" % (who, MESH_MAX_SIDE))
    Nv, Nf = int(vertices.shape[0]), 0 if faces is None else int(faces.shape[0])
    if Nv > 2 ** 31 - 1:
        raise ValueError("%s: at most 2^31 - 1 vertices" % who)
    if Nf > MESH_MAX_FACES:
        raise ValueError("%s: at most 2^32 - 2 faces" % who)
    proj = _world_maps(cm.decompose(who, intrinsics, extrinsics))
    if h * w > (2 ** 31 - 1) // 4 or proj.shape[0] > 65535:
        raise ValueError("%s: %d maps of %d x %d are outside what the kernel is built for" % (who, proj.shape[0], h, w))
    return Nv, Nf, h, w, proj


def _faces32(faces, Nv, dev):
    """``faces`` as contiguous int32 on ``dev``; an int64 index outside ``[0, Nv)`` becomes -1 (it must not wrap into range)."""
    faces = faces.to(dev)
    if faces.dtype == torch.int64:
        faces = torch.where((faces >= 0) & (faces < Nv), faces, torch.full_like(faces, -1)).to(torch.int32)
    return faces.contiguous()


def mesh_screen_coordinates(vertices, intrinsics, extrinsics, height, width, depth_min=1e-3, depth_max=1e5):
    """The rasteriser's table of screen coordinates (module docstring, "Screen coordinates") of ``vertices`` (Nv, 3) float32 on
    the GPU in every view: ``xy`` (V, Nv, 2) int32 with 8 sub-pixel bits (0 where not valid), ``z`` (V, Nv) float32 as
    computed, ``valid`` (V, Nv) bool.  The rasteriser does not read this table, it re-projects with the same device
    function; this is for tests and inspection."""
    who = "mesh_screen_coordinates"
    Nv, _, h, w, proj = _mesh_arguments(who, vertices, None, intrinsics, extrinsics, height, width)
    V = int(proj.shape[0])
    _lib.require_gpu(vertices)
    dev = vertices.device
    with _lib.on_device(dev):
        xy = torch.zeros((V, Nv, 2), dtype=torch.int32, device=dev)
        z = torch.zeros((V, Nv), dtype=torch.float32, device=dev)
        valid = torch.zeros((V, Nv), dtype=torch.uint8, device=dev)
        if Nv and V:
            proj = torch.from_numpy(proj).to(dev)
            _lib.call("pf_mesh_screen_f32", _lib.ptr(vertices.contiguous()), Nv, _lib.ptr(proj), V, h, w, float(depth_min),
                      float(depth_max), _lib.ptr(xy), _lib.ptr(z), _lib.ptr(valid), _lib.stream(),
                      algo_bytes=12 * Nv + 13 * V * Nv)
    return xy, z, valid.bool()


def render_mesh_depth_maps(vertices, faces, intrinsics, extrinsics, height, width, depth_min=1e-3, depth_max=1e5, cull=None,
                           return_index=False, return_barycentric=False, lane_pixels=None):
    """Rasterise the triangle mesh ``vertices`` (Nv, 3) float32, ``faces`` (Nf, 3) int32 or int64 on the GPU into the
    ``height`` x ``width`` depth maps of the cameras ``intrinsics`` (V, 3, 3, of that grid) and ``extrinsics`` (V, 3, 4) or
    (V, 4, 4) by the specification in this module's docstring ("Mesh rasterisation").  ``cull``: None, "back" or "front".

    Returns ``depth`` (V, h, w) float32 on the device of ``vertices``, 0 where no face covers the pixel centre; then, with
    ``return_index``, the int64 (V, h, w) map of the winning faces' rows (-1 where empty) and, with ``return_barycentric``,
    ``bary`` (V, h, w, 3) float32, the perspective-correct weights of the winner's three vertices in their stored order
    (zeros where empty).  Works on the current stream without a host synchronisation; a face with a non-finite vertex or an
    index outside ``[0, Nv)`` is skipped, not reported.  There is no CPU path.  ``lane_pixels`` overrides
    ``MESH_LANE_PIXELS`` for measurements; the result does not depend on it."""
    who = "render_mesh_depth_maps"
    Nv, Nf, h, w, proj = _mesh_arguments(who, vertices, faces, intrinsics, extrinsics, height, width)
    if faces is None:
        raise ValueError("%s: faces must be an (Nf, 3) int32 or int64 tensor" % who)
    if cull not in _CULL:
        raise ValueError("%s: cull must be None, \"back\" or \"front\"" % who)
    if lane_pixels is not None and (int(lane_pixels) != lane_pixels or not 0 <= lane_pixels < 2 ** 31):
        raise ValueError("%s: lane_pixels must be a non-negative integer" % who)
    V = int(proj.shape[0])
    _lib.require_gpu(vertices)
    dev = vertices.device
    with _lib.on_device(dev):
        depth = torch.zeros((V, h, w), dtype=torch.float32, device=dev)
        index = torch.full((V, h, w), -1, dtype=torch.int64, device=dev) if return_index else None
        bary = torch.zeros((V, h, w, 3), dtype=torch.float32, device=dev) if return_barycentric else None
        if Nv and Nf and V and h and w:
            vertices = vertices.contiguous()
            faces = _faces32(faces, Nv, dev)
            proj = torch.from_numpy(proj).to(dev)
            zbuf = torch.full((V, h, w), -1, dtype=torch.int64, device=dev)       # all-ones, on the stream of the launch
            # the mesh once, a cell read per covered (face, pixel, view); the atomics beyond that depend on the scene
            head = (_lib.ptr(vertices), Nv, _lib.ptr(faces), Nf, _lib.ptr(proj), V, h, w, float(depth_min), float(depth_max))
            if lane_pixels is None:
                _lib.call("pf_mesh_raster_f32", *(head + (_CULL[cull], _lib.ptr(zbuf), _lib.stream())),
                          algo_bytes=12 * Nv + 12 * Nf + 16 * V * h * w)
            else:
                _lib.call("pf_mesh_raster_tuned_f32", *(head + (_CULL[cull], int(lane_pixels), _lib.ptr(zbuf), _lib.stream())),
                          algo_bytes=12 * Nv + 12 * Nf + 16 * V * h * w)
            need_index = return_index or return_barycentric
            index32 = torch.empty((V, h, w), dtype=torch.int32, device=dev) if need_index else None
            _lib.call("pf_cloud_zbuf_decode", _lib.ptr(zbuf), V, h, w, _lib.ptr(depth), _lib.ptr(index32), _lib.stream(),
                      algo_bytes=V * h * w * (8 + 4 + (4 if need_index else 0)))
            if return_barycentric:
                _lib.call("pf_mesh_bary_f32", *(head + (_lib.ptr(index32), _lib.ptr(bary), _lib.stream())),
                          algo_bytes=V * h * w * (4 + 12 + 48))
            if return_index:
                index = index32.to(torch.int64)
                if Nf > 2 ** 31:                                                  # rows past 2^31 - 1 come back as bit patterns
                    index = torch.where(index < -1, index + 2 ** 32, index)
    out = (depth,) + ((index,) if return_index else ()) + ((bary,) if return_barycentric else ())
    return out if len(out) > 1 else depth


def interpolate_vertex_attributes(index, bary, faces, attributes):
    """Per-pixel attributes from the maps of ``render_mesh_depth_maps``: ``(V, h, w, C)`` float32
    ``= sum_k bary[..., k] * attributes[faces[index, k]]``, zeros where ``index < 0``.  ``index`` (V, h, w) integer, ``bary``
    (V, h, w, 3), ``faces`` (Nf, 3) integer, ``attributes`` (Nv, C) float32.  Plain torch on the maps' device (CPU tensors
    work).  With ``colours.float()`` it gives an image of the mesh, with vertex normals a normal map."""
    who = "interpolate_vertex_attributes"
    if not isinstance(index, torch.Tensor) or index.dim() != 3 or index.dtype.is_floating_point or index.dtype == torch.bool:
        raise ValueError("%s: index must be a (V, h, w) integer tensor" % who)
    if not isinstance(bary, torch.Tensor) or bary.shape != index.shape + (3,) or bary.dtype != torch.float32:
        raise ValueError("%s: bary must be a float32 tensor of index's shape + (3,)" % who)
    if (not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point
            or faces.dtype == torch.bool):
        raise ValueError("%s: faces must be an (Nf, 3) integer tensor" % who)
    if not isinstance(attributes, torch.Tensor) or attributes.dim() != 2 or attributes.dtype != torch.float32:
        raise ValueError("%s: attributes must be an (Nv, C) float32 tensor" % who)
    dev = index.device
    out = torch.zeros(index.shape + (int(attributes.shape[1]),), dtype=torch.float32, device=dev)
    if faces.shape[0] == 0 or index.numel() == 0:
        return out
    filled = index >= 0
    corners = faces.to(dev).long()[index.long().clamp(min=0)]                      # (V, h, w, 3) vertex rows
    attributes, bary = attributes.to(dev), bary.to(dev)
    for k in range(3):
        out = out + bary[..., k, None] * attributes[corners[..., k]]
    return torch.where(filled[..., None], out, torch.zeros_like(out))
