"""Guided upsampling of depth maps on the GPU: a joint bilateral filter steered by the image the network saw.

The depth maps of this pipeline live on half the image's grid or less, and ``ScanAccumulator`` used to throw three quarters
of every ``ref_img`` away.  This module brings a filtered depth map up to the image's own grid (or, at scale 1, smooths it
on its own grid) between ``scan.filter_depth_maps`` and the fusers; it runs as HIP kernels (csrc/depth_refine.hip).  **The
specification below is this project's own**; parity with OpenCV's ``ximgproc`` filters, Open3D or any paper's code is
neither claimed nor tested.  Pixel centres are at ``(x + 0.5, y + 0.5)``, as everywhere else in this pipeline.

Inputs.  ``depths`` (V, h, w) float32, 0 = no depth; ``guides`` (V, H, W, 3) uint8 with ``H = s h`` and ``W = s w`` for one
integer scale ``1 <= s <= 8``.  The output is (V, H, W) float32; the count map (V, H, W) int32 is the number of linked taps.

Tables, built on the host in float64 and stored as float32; an entry below ``2^-24`` is set to 0:

* ``ws[p][j + R]`` for phase ``p`` in ``[0, s)`` and tap offset ``j`` in ``[-R, R]``, ``R = radius``:
  ``exp(-delta^2 / (2 sigma_space^2))`` with ``delta = j + .5 - (p + .5) / s``, the distance in low-resolution pixels between
  the tap's centre and the output pixel's centre;
* ``wc[a]`` for ``a`` in ``[0, 765]``: ``exp(-(a / 3)^2 / (2 sigma_colour^2))``.

Taps.  Output pixel ``(X, Y)`` has the containing low-resolution pixel ``c = (X // s, Y // s)`` and the phases
``(px, py) = (X % s, Y % s)``.  Tap ``(tx, ty)`` is the low-resolution pixel ``q = c + (tx, ty)``.

* A tap outside the map does not exist: there is no border replication.
* The tap's colour is that of the guide pixel that contains the tap's centre, ``guide[qy s + s // 2][qx s + s // 2]``.
* ``a`` is the sum of the three absolute channel differences to the output pixel's own guide colour ``guide[Y][X]``.
* The weight is ``w = (ws[py][ty] * ws[px][tx]) * wc[a]``, in float32 in that order.
* ``valid(q)``: ``depth_min < d(q) < depth_max``.

Anchor.  If ``c`` is not valid the output is 0 and the count 0: holes stay holes, and the confidence filter's decisions are
kept.  Otherwise the anchor starts at ``c``; the taps with ``|tx|, |ty| <= anchor_radius`` are visited in row-major order
(``ty`` outer) and a valid tap with a strictly larger ``w`` becomes the anchor.  ``d0`` is the anchor's depth.  The anchor
is what lets the guide move a depth edge off the low-resolution pixel border: an output pixel whose colour is that of the
neighbouring low-resolution pixel takes its depth from there.  With ``anchor_radius=0`` the edge stays where nearest
replication puts it.

Mean.  A tap is linked if it is valid and ``|d(q) - d0| <= rel_jump * d0``; the float32 subtraction, the float32 product
and the comparison are done as written.  Over the taps with ``|tx|, |ty| <= radius`` in row-major order, linked taps only,
in float32: ``W += w`` and ``S += w * (d(q) - d0)``.  The result is ``d0 + S / W`` if ``W > 0``, else ``d0``.

Summing offsets from ``d0`` is deliberate and not the same as summing depths: ``d - d0`` is exact for ``rel_jump <= 0.5``
(Sterbenz), so rounding acts at the size of the jump and not at the size of the depth.  Every decision and every operation
is float32 exactly as written (the library is built with ``-ffp-contract=off``), so a NumPy float32 statement reproduces the
result bit for bit.  There are no atomics: the result is a pure function of the input.

Limits: ``0 <= radius <= 8``, ``0 <= anchor_radius <= min(radius, 2)``, ``0 <= rel_jump <= 0.5``, both sigmas ``> 0``.

Cameras.  ``upsampled_intrinsics(K, s) = diag(s, s, 1) @ K``: with centres at ``(x + .5, y + .5)`` the centre of output
pixel ``X`` is ``s`` times its position on the low-resolution grid, so this is exact.

Out of scope: hole filling (``depth_segments.fill_gaps`` closes small gaps before this stage), upsampling of probabilities
or normals, non-integer or anisotropic scales, ``mesh()`` on upsampled maps.
"""
import numpy as np
import torch

from . import _lib, camera_maps as cm

_WHO = "upsample_depth_maps"
MAX_SCALE, MAX_RADIUS, MAX_ANCHOR_RADIUS = 8, 8, 2
_TINY = 2.0 ** -24


def spatial_table(s, radius, sigma_space):
    """``ws`` of the module docstring: (s, 2 radius + 1) float32, entry ``[p][j + radius]``."""
    p = np.arange(int(s), dtype=np.float64)[:, None]
    j = np.arange(-int(radius), int(radius) + 1, dtype=np.float64)[None, :]
    delta = j + 0.5 - (p + 0.5) / float(s)
    t = np.exp(-delta * delta / (2.0 * float(sigma_space) ** 2))
    t[t < _TINY] = 0.0
    return np.ascontiguousarray(t, dtype=np.float32)


def colour_table(sigma_colour):
    """``wc`` of the module docstring: (766,) float32."""
    a = np.arange(766, dtype=np.float64) / 3.0
    t = np.exp(-a * a / (2.0 * float(sigma_colour) ** 2))
    t[t < _TINY] = 0.0
    return np.ascontiguousarray(t, dtype=np.float32)


def upsampled_intrinsics(intrinsics, s):
    """``diag(s, s, 1) @ K`` for ``K`` (3, 3) or (V, 3, 3), in float64: the cameras of the upsampled grid."""
    if isinstance(s, bool) or int(s) != s or int(s) < 1:
        raise ValueError("upsampled_intrinsics: s must be an integer of at least 1")
    K = cm.host_f64(intrinsics)
    if K.shape[-2:] != (3, 3):
        raise ValueError("upsampled_intrinsics: intrinsics must be (3, 3) or (V, 3, 3)")
    return np.diag([float(int(s)), float(int(s)), 1.0]) @ K


def check_settings(who, radius, anchor_radius, sigma_space, sigma_colour, rel_jump):
    """The limits of the module docstring as ValueErrors of ``who``; ``(radius, anchor_radius, sigma_space, sigma_colour,
    rel_jump)`` as ints and floats."""
    for name, v in (("radius", radius), ("anchor_radius", anchor_radius)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s: %s must be an integer" % (who, name))
    radius, anchor_radius = int(radius), int(anchor_radius)
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError("%s: radius must be in [0, %d]" % (who, MAX_RADIUS))
    if not 0 <= anchor_radius <= min(radius, MAX_ANCHOR_RADIUS):
        raise ValueError("%s: anchor_radius must be in [0, min(radius, %d)]" % (who, MAX_ANCHOR_RADIUS))
    if not (float(sigma_space) > 0.0 and float(sigma_colour) > 0.0 and np.isfinite(sigma_space) and np.isfinite(sigma_colour)):
        raise ValueError("%s: sigma_space and sigma_colour must be positive" % who)
    if not 0.0 <= float(rel_jump) <= 0.5:
        raise ValueError("%s: rel_jump must be in [0, 0.5]" % who)
    return radius, anchor_radius, float(sigma_space), float(sigma_colour), float(rel_jump)


def scale_of(who, low_hw, high_hw):
    """The integer ``s`` with ``high_hw == s * low_hw`` on both axes, ``1 <= s <= 8``, or the ValueError of ``who``."""
    (h, w), (H, W) = (int(v) for v in low_hw), (int(v) for v in high_hw)
    if h == 0 or w == 0:
        s = max(H // h if h else 0, W // w if w else 0, 1)
    else:
        s = H // h
    if s < 1 or s > MAX_SCALE or H != s * h or W != s * w:
        raise ValueError("%s: the guides' size %s must be the depth maps' size %s times one integer in [1, %d]"
                         % (who, (H, W), (h, w), MAX_SCALE))
    return s


def upsample_depth_maps(depths, guides, radius=2, anchor_radius=1, sigma_space=1.0, sigma_colour=12.0, rel_jump=0.02,
                        depth_min=1e-3, depth_max=1e5, return_count=False):
    """``depths`` (V, h, w) float32 on the GPU (0 = no depth; a sequence of (h, w) maps is stacked) upsampled to the grid of
    ``guides`` (V, H, W, 3) uint8 on the same device, ``H = s h`` and ``W = s w`` for one integer ``1 <= s <= 8``, by the
    specification in this module's docstring.  ``s = 1`` is an edge-preserving smoothing of the map on its own grid.

    Returns (V, H, W) float32 on the device of ``depths``, 0 where the containing low-resolution pixel has no depth; with
    ``return_count`` also (V, H, W) int32, the number of linked taps per pixel.  There is no CPU path."""
    depths = cm.stack_depths(_WHO, depths, 1)
    radius, anchor_radius, sigma_space, sigma_colour, rel_jump = check_settings(
        _WHO, radius, anchor_radius, sigma_space, sigma_colour, rel_jump)
    if not isinstance(guides, torch.Tensor):
        guides = torch.stack([torch.as_tensor(g) for g in guides])
    if depths.dtype != torch.float32:
        raise ValueError("%s: depths must be float32" % _WHO)
    V, h, w = (int(v) for v in depths.shape)
    if guides.dim() != 4 or int(guides.shape[0]) != V or int(guides.shape[3]) != 3 or guides.dtype != torch.uint8:
        raise ValueError("%s: guides must be (V, H, W, 3) uint8 with the V of depths" % _WHO)
    H, W = int(guides.shape[1]), int(guides.shape[2])
    s = scale_of(_WHO, (h, w), (H, W))
    if V < 1:
        raise ValueError("%s: no views" % _WHO)
    _lib.require_gpu(depths, guides)                      # bad arguments are reported before a missing GPU
    dev = depths.device
    if guides.device != dev:
        raise ValueError("%s: depths and guides must be on the same device" % _WHO)
    depths, guides = depths.contiguous(), guides.contiguous()
    with _lib.on_device(dev):
        out = torch.empty((V, H, W), dtype=torch.float32, device=dev)
        count = torch.empty((V, H, W), dtype=torch.int32, device=dev) if return_count else None
        if h and w:
            ws = torch.from_numpy(spatial_table(s, radius, sigma_space)).to(dev)
            wc = torch.from_numpy(colour_table(sigma_colour)).to(dev)
            records = torch.empty((V, h, w, 2), dtype=torch.int32, device=dev)
            # per low-resolution pixel: its depth and 3 guide bytes in, 8 bytes out
            _lib.call("pf_guide_pack_f32", _lib.ptr(depths), _lib.ptr(guides), V, h, w, s, _lib.ptr(records), _lib.stream(),
                      algo_bytes=15 * V * h * w, tag="s %d" % s)
            # per output pixel: its own guide colour in, its depth out, and its share of the records
            _lib.call("pf_depth_upsample_f32", _lib.ptr(records), _lib.ptr(guides), _lib.ptr(ws), _lib.ptr(wc), V, h, w, s,
                      radius, anchor_radius, rel_jump, float(depth_min), float(depth_max), _lib.ptr(out), _lib.ptr(count),
                      _lib.stream(), algo_bytes=(7 + (4 if return_count else 0)) * V * H * W + 8 * V * h * w,
                      tag="s %d r %d a %d%s" % (s, radius, anchor_radius, " count" if return_count else ""))
    return (out, count) if return_count else out
