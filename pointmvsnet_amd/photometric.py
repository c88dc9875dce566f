"""Photometric consistency of depth maps on the GPU: windowed zero-mean normalised cross-correlation (ZNCC).

Every other stage between the network and the cloud judges a depth by geometry or by the network's own confidence.  This
one looks at the images again: warp a small window of the reference image into a source view through the pixel's depth
and correlate the two windows, the photometric check of COLMAP, Gipuma and OpenMVS.  The reference has nothing of the
kind and OpenCV is not a dependency, so **the specification below is this project's own**; parity with COLMAP or any other
code is neither claimed nor tested.  It runs as HIP kernels (csrc/photo_filter.hip).  Pixel centres are at
``(x + 0.5, y + 0.5)``, as everywhere else in this pipeline.  Float32 operations run in the stated order.

**Grey images.**  ``grey_images(images)`` takes ``(V, h, w, 3)`` uint8 RGB and returns ``(V, h, w)`` uint8 with
``g = (77 R + 150 G + 29 B + 128) >> 8``: exact integer arithmetic with a maximum of 255.

**Inputs.**  ``depths`` is ``(V, h, w)`` float32 with 0 meaning no depth; ``images`` are on the same grid and the cameras
are of that grid.  ``sources`` is ``(V, M)`` with ``-1`` pads, ``None`` meaning all other views in ascending order (the
rules of ``geometric_filter``).  ``radius`` is ``r`` in 1..5 and ``n = (2 r + 1)^2``; with ``r <= 5`` every integer below
fits in int32.  ``min_variance`` (default 25.0, in grey levels squared, in ``(0, 65025]``) becomes the integer
``var_min = ceil(n * n * min_variance)`` on the host.  ``ncc_threshold`` defaults to 0.6, ``num_consistent`` to 2,
``depth_min`` and ``depth_max`` to ``1e-3`` and ``1e5``.

**Reference window** of pixel ``p = (x, y)`` in view ``i``, where ``d = d_i(p)`` and ``c = g_i(y, x)``:

1. For every tap ``(dx, dy)`` in ``[-r, r]^2``, ``R = g_i(y + dy, x + dx) - c``, an integer.
2. ``SR = sum R`` and ``SRR = sum R^2``.
3. ``VR = n * SRR - SR * SR``, an exact integer.
4. ``p`` is *scorable* iff all three hold:

   - ``depth_min < d < depth_max``;
   - ``r <= x < w - r`` and ``r <= y < h - r`` (no border replication);
   - ``VR >= var_min``, an exact integer decision.

**Per source slot** ``m``, with ``j = sources[i, m]``, skipping ``-1`` and ``j == i``.  The taps are taken with ``dy``
ascending in the outer loop and ``dx`` ascending in the inner loop:

1. ``px = float(x + dx) + 0.5f``, and ``py`` likewise.
2. ``(qx, qy, z) = (M (px, py, 1)) d + T`` with the pair row ``i -> j`` of ``camera_maps.pair_row``, evaluated as
   ``(m0 px + m1 py + m2) d + m9`` and so on, left to right.  The window is fronto-parallel at the centre's depth.  Every
   tap goes through the full map; there is no incremental stepping.
3. ``rz = 1.0f / z``, ``u = qx * rz``, ``v = qy * rz``: one division per tap.
4. ``fx = u - 0.5f``, ``fy = v - 0.5f``, ``x0 = floorf(fx)``, ``y0 = floorf(fy)``.
5. The tap is *inside* iff ``z > 0 && x0 >= 0 && x0 + 1 <= w - 1 && y0 >= 0 && y0 + 1 <= h - 1``
   (``geometric_filter``'s test).
6. ``s`` is the bilinear value of ``g_j`` as float32, minus ``float(c)``; horizontal first, then vertical, with
   ``wx = fx - x0`` and ``wy = fy - y0``: ``top = t00 * (1 - wx) + t01 * wx``, ``bot`` likewise on row ``y0 + 1``, then
   ``top * (1 - wy) + bot * wy``.
7. ``S1 += s``, ``S2 += s * s`` and ``SX += float(R) * s``, all float32.

After the taps: ``VS = n * S2 - S1 * S1`` and ``COV = n * SX - float(SR) * S1``.  The source is *usable* iff ``p`` is
scorable, every tap is inside, and ``VS >= float(var_min)``.  ``ncc = fminf(1, fmaxf(-1, COV / sqrtf(float(VR) * VS)))``.

Subtracting ``c`` from both windows is deliberate: ZNCC is shift-invariant, and it keeps the one-pass sums at the size
of the window's contrast rather than its brightness.

**Per pixel.**  ``usable`` is the number of usable sources; ``count`` the number with ``ncc >= ncc_threshold``; ``score``
the float32 sum of the usable ``ncc`` in slot order divided by ``float(usable)``, 0 when ``usable`` is 0;
``mask = scorable && count >= num_consistent``.  With ``return_per_source`` the ``(V, M, h, w)`` array ``ncc`` is also
returned; it holds NaN wherever the source is not usable.

The matrices are composed in float64 and handed to the kernel as float32, by ``geometric``'s own helpers.

Out of scope: slanted windows from ``depth_normals``, per-tap depths, bilateral window weights, using the score inside
``fuse_depth_maps``' matching, cleaning the probability maps.
"""
import math

import numpy as np
import torch

from . import _lib, camera_maps as cm, geometric as geo

_WHO = "photometric_consistency"
MAX_RADIUS = 5


def _settings(who, radius, min_variance, ncc_threshold, num_consistent, depth_min, depth_max):
    """``(radius, var_min)`` after the checks that need no GPU."""
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError("%s: radius must be an integer in 1..%d" % (who, MAX_RADIUS))
    radius = int(radius)
    min_variance = float(min_variance)
    if not 0.0 < min_variance <= 255.0 * 255.0:
        raise ValueError("%s: min_variance must be in (0, 65025] grey levels squared" % who)
    if not -1.0 <= float(ncc_threshold) <= 1.0:
        raise ValueError("%s: ncc_threshold must be in [-1, 1]" % who)
    if isinstance(num_consistent, bool) or int(num_consistent) != num_consistent or int(num_consistent) < 1:
        raise ValueError("%s: num_consistent must be an integer of at least 1" % who)
    if not 0.0 <= float(depth_min) < float(depth_max):
        raise ValueError("%s: 0 <= depth_min < depth_max is required" % who)
    n = (2 * radius + 1) ** 2
    return radius, int(math.ceil(n * n * min_variance))


def _check_images(who, images, V, h, w):
    if not isinstance(images, torch.Tensor):
        images = torch.as_tensor(np.asarray(images))
    if tuple(images.shape) != (V, h, w, 3) or images.dtype != torch.uint8:
        raise ValueError("%s: images must be (V, h, w, 3) uint8 of the depth maps' size" % who)
    return images


def grey_images(images):
    """``(V, h, w)`` uint8 grey planes of ``images`` (V, h, w, 3) uint8 RGB on the GPU:
    ``g = (77 R + 150 G + 29 B + 128) >> 8``.  There is no CPU path."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
        raise ValueError("grey_images: images must be a (V, h, w, 3) uint8 tensor")
    _lib.require_gpu(images)
    images = images.contiguous()
    with _lib.on_device(images.device):
        grey = torch.empty(tuple(images.shape[:3]), dtype=torch.uint8, device=images.device)
        _lib.call("pf_grey_pack_u8", _lib.ptr(images), grey.numel(), _lib.ptr(grey), _lib.stream(),
                  algo_bytes=4 * grey.numel())
    return grey


def photometric_consistency(depths, images, intrinsics, extrinsics, sources=None, radius=2, min_variance=25.0,
                            ncc_threshold=0.6, num_consistent=2, depth_min=1e-3, depth_max=1e5, return_per_source=False):
    """Score ``depths`` (V, h, w) float32 on the GPU (0 = no depth; a sequence of (h, w) maps is stacked) against the
    ``images`` (V, h, w, 3) uint8 RGB of the same grid, with cameras ``intrinsics`` (V, 3, 3, of that grid) and
    ``extrinsics`` (V, 3, 4) or (V, 4, 4) and the source views ``sources`` (V, M) (integers, ``-1`` pads; None: all other
    views), by the specification in this module's docstring.

    Returns ``(score (V, h, w) float32, mask (V, h, w) bool, count (V, h, w) int32, usable (V, h, w) int32)`` and, with
    ``return_per_source``, ``ncc (V, M, h, w)`` float32 (NaN where a source is not usable).  Everything is on the device of
    ``depths``.  There is no CPU path."""
    return _consistency(_WHO, depths, images, intrinsics, extrinsics, sources, radius, min_variance, ncc_threshold,
                        num_consistent, depth_min, depth_max, return_per_source)[0]


def _consistency(who, depths, images, intrinsics, extrinsics, sources, radius, min_variance, ncc_threshold, num_consistent,
                 depth_min, depth_max, return_per_source):
    """The outputs above; then the float32 maps, the kernel's own ``scorable`` map (bit 1 of its mask byte) and the settings."""
    radius, var_min = _settings(who, radius, min_variance, ncc_threshold, num_consistent, depth_min, depth_max)
    depths = cm.stack_depths(who, depths, num_consistent)
    V, h, w = (int(s) for s in depths.shape)
    if images is None:
        raise ValueError("%s: images are needed" % who)
    images = _check_images(who, images, V, h, w)
    table = geo._source_table(sources, V)                              # a bad table is reported before a missing GPU
    cams = cm.decompose(who, intrinsics, extrinsics, V)
    depths, images, V, h, w, dev = cm.normalise_inputs(who, depths, images, num_consistent)
    pair_maps, M = geo._source_maps(cams, table), int(table.shape[1])
    with _lib.on_device(dev):
        grey = grey_images(images)
        quads = torch.empty((V, h, w), dtype=torch.int32, device=dev)           # a tap's 2 x 2 bytes as one dword
        _lib.call("pf_grey_quads_u8", _lib.ptr(grey), V, h, w, _lib.ptr(quads), _lib.stream(), algo_bytes=5 * V * h * w)
        src, pairs = torch.from_numpy(table).to(dev), torch.from_numpy(pair_maps).to(dev)
        score = torch.empty((V, h, w), dtype=torch.float32, device=dev)
        count = torch.empty((V, h, w), dtype=torch.int32, device=dev)
        usable = torch.empty((V, h, w), dtype=torch.int32, device=dev)
        mask = torch.empty((V, h, w), dtype=torch.uint8, device=dev)
        ncc = torch.empty((V, M, h, w), dtype=torch.float32, device=dev) if return_per_source else None
        # per pixel: its depth and quad, the outputs; per listed source its plane of quads once (the taps are cached)
        listed = int(((table >= 0) & (table != np.arange(V)[:, None])).sum())
        algo = h * w * (V * (4 + 4 + 4 + 4 + 4 + 1) + (4 * V * M if return_per_source else 0) + 4 * listed)
        _lib.call("pf_photo_ncc_f32", _lib.ptr(depths), _lib.ptr(quads), _lib.ptr(src), _lib.ptr(pairs), V, M, h, w, radius,
                  var_min, float(ncc_threshold), int(num_consistent), float(depth_min), float(depth_max), _lib.ptr(ncc),
                  _lib.ptr(score), _lib.ptr(count), _lib.ptr(usable), _lib.ptr(mask), _lib.stream(), algo_bytes=algo,
                  tag="r%d" % radius)
        out = (score, (mask & 1).bool(), count, usable) + ((ncc,) if return_per_source else ())
    return out, (depths, (mask & 2).bool(), var_min, radius)


def photometric_filter(depths, images, intrinsics, extrinsics, sources=None, radius=2, min_variance=25.0,
                       ncc_threshold=0.6, num_consistent=2, depth_min=1e-3, depth_max=1e5):
    """``(filtered (V, h, w) float32, report)``: ``depths`` with every pixel off ``photometric_consistency``'s mask set to
    0.  A pixel that is not scorable -- at the border, or in a window without texture -- has no photometric evidence and is
    removed with the rest; the report tells the two apart.  ``report`` holds, per view (lists) and in total, the number of
    ``valid`` pixels (``depth_min < d < depth_max``), of ``scorable`` ones, of those ``kept`` and of the valid ones
    ``removed``: ``{"views": {...}, "total": {...}, "settings": {...}}``."""
    who = "photometric_filter"
    out, (depths32, scorable, var_min, radius) = _consistency(who, depths, images, intrinsics, extrinsics, sources, radius,
                                                          min_variance, ncc_threshold, num_consistent, depth_min, depth_max,
                                                          False)
    mask = out[1]
    with _lib.on_device(depths32.device):
        valid = (depths32 > float(np.float32(depth_min))) & (depths32 < float(np.float32(depth_max)))
        filtered = torch.where(mask, depths32, torch.zeros_like(depths32))
        counts = torch.stack([valid.flatten(1).sum(1), scorable.flatten(1).sum(1), mask.flatten(1).sum(1),
                              (valid & ~mask).flatten(1).sum(1)]).cpu().numpy()
    names = ("valid", "scorable", "kept", "removed")
    report = {"views": {k: [int(c) for c in counts[a]] for a, k in enumerate(names)},
              "total": {k: int(counts[a].sum()) for a, k in enumerate(names)},
              "settings": {"radius": radius, "min_variance": float(min_variance), "var_min": var_min,
                           "ncc_threshold": float(ncc_threshold), "num_consistent": int(num_consistent)}}
    return filtered, report
