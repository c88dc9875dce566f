"""Image and camera preprocessing of a DTU scene: decoded uint8 views -> the ``img_list`` that ``PointMVSNet.forward`` takes.

The reference prepares float32 images on the host (``cv2.resize`` -> ``crop_dtu_input`` -> ``norm_image``, reference
dataset.py:269-287, utils/preprocess.py) and uploads 12 bytes per pixel.  Here the decoded **uint8** views go to the GPU
(3 bytes per pixel) and csrc/preprocess.hip resizes, crops and standardises them; the same steps exist in NumPy for a host
without a GPU.  Same function names as reference utils/preprocess.py where the behaviour is the same; written from the
behaviour, not from its text.

Specification
-------------
Channel order is kept as decoded (the reference feeds ``cv2.imread``'s BGR to the network).

* **Resize** by ``scale`` (skipped when ``scale == 1``).  **This part is the project's own**: the reference goes through
  OpenCV's fixed-point uint8 kernel, which is not restated here; bit parity with ``cv2.resize`` is neither claimed nor
  tested (tools/microbench_preprocess.py reports the difference wherever OpenCV is installed).  Destination size per axis:
  ``round_half_even(src * scale)``.  Destination index ``d`` samples the source coordinate ``(d + 0.5) / scale - 0.5``
  (half-pixel centres, the geometry of ``cv2.INTER_LINEAR``): ``s = floor``, weight = the fraction; ``s < 0`` -> index 0,
  weight 0; ``s >= src - 1`` -> index ``src - 1``, weight 0.  The tables (index int32, weight) are composed in float64 and
  used as float32 (the convention of ``fusion.camera_maps``).  A pixel is
  ``(1-wy)*((1-wx)*p00 + wx*p01) + wy*((1-wx)*p10 + wx*p11)``, rounded half-to-even to uint8; the kernel evaluates it in
  float32, ``resize_linear`` below in float64 with the float32 tables.
* **Crop**: the centre crop of reference ``crop_dtu_input``: per axis ``new = target if size > target else
  floor(size / base) * base``, ``start = floor((size - new) / 2)``; the principal point moves by ``-start``.
* **Standardise** (``norm_image``): per view and channel over the cropped image ``(p - mean) / (sqrt(var) + 1e-7)`` with the
  population variance.  On the GPU the sums of ``p`` and ``p*p`` are 64-bit integers (exact, so two runs give identical bits
  whatever the order of the additions); mean = S1/N and var = (N S2 - S1^2)/N^2 are derived from them in float64 and each
  output is the float64 expression rounded once to float32.  On the host ``norm_image`` does the reference's float32 NumPy
  operations in the reference's order and equals it bit for bit (tests/golden/preprocess.npz); the two differ by the
  rounding error of that float32 arithmetic.

Bytes per scene on the GPU route: the source is read once (3 B per source pixel), the uint8 image (also the ``ref_img`` of
the evaluation writer) is written and read back (3 + 3 B per output pixel: the second pass looks the standardised value of
a byte up instead of blending again), and 12 B per output pixel of float32 are written.
"""
import math

import numpy as np
import torch

from .. import _lib

TILE_X = 256           # PF_PREPROCESS_TILE_X of include/pointflow_hip.h


# ---------------------------------------------------------------------------------------------------------------------
# host arithmetic (the reference's names)
# ---------------------------------------------------------------------------------------------------------------------
def norm_image(img):
    """Standardise an (h, w, c) image per channel in float32, like the reference's function of this name."""
    pixels = img.astype(np.float32)
    variance = np.var(pixels, axis=(0, 1), keepdims=True)
    centre = np.mean(pixels, axis=(0, 1), keepdims=True)
    return (pixels - centre) / (np.sqrt(variance) + 1e-7)


def mask_depth_image(depth_image, min_depth, max_depth):
    """``depth`` where ``min_depth < depth <= max_depth``, else 0, as (h, w, 1): what the reference obtains from
    ``cv2.threshold`` with THRESH_TOZERO (keeps values above the threshold) and then THRESH_TOZERO_INV (keeps values not
    above it)."""
    depth_image = np.asarray(depth_image)
    keep = (depth_image > min_depth) & (depth_image <= max_depth)
    return np.where(keep, depth_image, np.zeros((), depth_image.dtype))[:, :, None]


def scale_camera(cam, scale=1):
    """A copy of the (2, 4, 4) camera whose focal lengths and principal point are multiplied by ``scale``."""
    out = np.array(cam, copy=True)
    for r, c in ((0, 0), (1, 1), (0, 2), (1, 2)):
        out[1][r][c] = cam[1][r][c] * scale
    return out


def crop_window(size, target, base_image_size):
    """``(start, new_size)`` of the centre crop along one axis (``target`` None: no crop)."""
    size = int(size)
    if target is None:
        return 0, size
    new = int(target) if size > target else int(math.floor(size / base_image_size) * base_image_size)
    return int(math.floor((size - new) / 2)), new


def crop_camera(cam, start_h, start_w):
    """The camera of the cropped image: the principal point moves by the crop offsets (in place, like the reference)."""
    cam[1][0][2] = cam[1][0][2] - start_w
    cam[1][1][2] = cam[1][1][2] - start_h
    return cam


def scaled_size(size, scale):
    return int(size) if scale == 1 else int(round(int(size) * float(scale)))       # round(): half to even


def resize_tables(src_size, scale):
    """``(index int32, weight float32)`` of every destination index along one axis (module docstring)."""
    src_size = int(src_size)
    n = scaled_size(src_size, scale)
    if scale == 1:
        return np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
    pos = (np.arange(n, dtype=np.float64) + 0.5) / float(scale) - 0.5
    idx = np.floor(pos)
    wgt = pos - idx
    low, high = idx < 0, idx >= src_size - 1
    idx = np.where(low, 0, np.where(high, src_size - 1, idx))
    wgt = np.where(low | high, 0.0, wgt)
    return idx.astype(np.int32), wgt.astype(np.float32)


def blend_tables(img, yi, yw, xi, xw):
    """The specification's blend of ``img`` (h, w, c) uint8 at the table entries, in float64 -> (values float64, uint8)."""
    src = np.asarray(img, dtype=np.float64)
    y0, x0 = yi.astype(np.int64), xi.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, src.shape[0] - 1), np.minimum(x0 + 1, src.shape[1] - 1)
    wy, wx = yw.astype(np.float64)[:, None, None], xw.astype(np.float64)[None, :, None]
    top = (1.0 - wx) * src[y0][:, x0] + wx * src[y0][:, x1]
    bot = (1.0 - wx) * src[y1][:, x0] + wx * src[y1][:, x1]
    val = (1.0 - wy) * top + wy * bot
    return val, np.rint(val).astype(np.uint8)                                      # np.rint: half to even


def resize_linear(img, scale):
    """``img`` (h, w, c) uint8 resized by ``scale``: the float64 statement of the specification."""
    if scale == 1:
        return np.array(img, copy=True)
    yi, yw = resize_tables(img.shape[0], scale)
    xi, xw = resize_tables(img.shape[1], scale)
    return blend_tables(img, yi, yw, xi, xw)[1]


# ---------------------------------------------------------------------------------------------------------------------
# all views of a scene
# ---------------------------------------------------------------------------------------------------------------------
_TABLE_CACHE = {}


def _tables(h_src, w_src, scale, height, width, base_image_size):
    """Row / column tables of the resized AND cropped image, the crop offsets and the kernel's span."""
    sy, H = crop_window(scaled_size(h_src, scale), height, base_image_size)
    sx, W = crop_window(scaled_size(w_src, scale), width, base_image_size)
    yi, yw = resize_tables(h_src, scale)
    xi, xw = resize_tables(w_src, scale)
    yi, yw, xi, xw = yi[sy:sy + H], yw[sy:sy + H], xi[sx:sx + W], xw[sx:sx + W]
    first = np.arange(0, W, TILE_X)
    last = np.minimum(first + TILE_X - 1, W - 1)
    span = int(np.max(np.minimum(xi[last] + 1, w_src - 1) - xi[first] + 1)) if W > 0 else 1
    return (yi, yw, xi, xw), (sy, sx), (H, W), span


def _device_tables(key, dev):
    hit = _TABLE_CACHE.get((key, dev))
    if hit is None:
        (yi, yw, xi, xw), offsets, size, span = _tables(*key)
        idx = torch.from_numpy(np.concatenate([yi, xi])).to(dev)
        wgt = torch.from_numpy(np.concatenate([yw, xw])).to(dev)
        if len(_TABLE_CACHE) >= 16:
            _TABLE_CACHE.clear()
        hit = _TABLE_CACHE[(key, dev)] = (idx, wgt, offsets, size, span)
    return hit


def preprocess_views_gpu(src, scale=1, height=None, width=None, base_image_size=64):
    """``src`` (V, h, w, 3) uint8 on a GPU -> ``(img_list (V, 3, H, W) float32, ref_img_u8 (V, H, W, 3) uint8,
    (start_h, start_w))`` on that GPU, by csrc/preprocess.hip: two launches for all the views, no CPU path."""
    _lib.require_gpu(src)
    if src.dim() != 4 or src.shape[3] != 3 or src.dtype != torch.uint8:
        raise ValueError("preprocess_views: images must be (V, h, w, 3) uint8")
    src = src.contiguous()
    dev = src.device
    V, h_src, w_src = (int(s) for s in src.shape[:3])
    key = (h_src, w_src, float(scale), height, width, base_image_size)
    with _lib.on_device(dev):
        idx, wgt, offsets, (H, W), span = _device_tables(key, dev)
        if V == 0 or H <= 0 or W <= 0:
            raise ValueError("preprocess_views: nothing left of %d views of %d x %d" % (V, h_src, w_src))
        ref = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
        out = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
        sums = torch.empty((V, 3, 2), dtype=torch.int64, device=dev)
        _lib.call("pf_preprocess_resize_u8", _lib.ptr(src), V, h_src, w_src, _lib.ptr(idx[H:]), _lib.ptr(wgt[H:]),
                  _lib.ptr(idx), _lib.ptr(wgt), H, W, span, _lib.ptr(ref), _lib.ptr(sums), _lib.stream(),
                  algo_bytes=V * 3 * (h_src * w_src + H * W))
        _lib.call("pf_preprocess_standardise_f32", _lib.ptr(ref), _lib.ptr(sums), V, H, W, _lib.ptr(out), _lib.stream(),
                  algo_bytes=V * H * W * (3 + 12))
    return out, ref, offsets


def preprocess_views(images_u8, scale=1, height=None, width=None, base_image_size=64, device=None):
    """All views of a scene: resize by ``scale``, centre-crop to at most ``height`` x ``width`` (None: no crop) and
    standardise, by the specification in this module's docstring.

    ``images_u8``: a (V, h, w, 3) uint8 tensor or array, or a sequence of (h, w, 3) uint8 arrays of one size.  The kernels
    run when ``device`` names a GPU, or when ``device`` is None and the images are a GPU tensor; otherwise NumPy does it on
    the host.  Returns ``(img_list (V, 3, H, W) float32 tensor, ref_img_u8 (V, H, W, 3) uint8 tensor, (start_h, start_w))``
    on that device."""
    if isinstance(images_u8, torch.Tensor):
        dev = images_u8.device if device is None else torch.device(device)
    else:
        dev = torch.device("cpu" if device is None else device)
        views = [np.asarray(v) for v in images_u8]
        if len(set(v.shape for v in views)) > 1:
            raise ValueError("preprocess_views: the views have different sizes")
        images_u8 = torch.from_numpy(np.ascontiguousarray(np.stack(views)))
    if images_u8.dim() != 4 or images_u8.shape[3] != 3 or images_u8.dtype != torch.uint8:
        raise ValueError("preprocess_views: images must be (V, h, w, 3) uint8")
    if dev.type != "cpu":
        return preprocess_views_gpu(images_u8.to(dev, non_blocking=True), scale, height, width, base_image_size)
    views = images_u8.cpu().numpy()
    sy, H = crop_window(scaled_size(views.shape[1], scale), height, base_image_size)
    sx, W = crop_window(scaled_size(views.shape[2], scale), width, base_image_size)
    cropped = [resize_linear(v, scale)[sy:sy + H, sx:sx + W] for v in views]
    img_list = torch.from_numpy(np.stack([norm_image(c) for c in cropped])).permute(0, 3, 1, 2).contiguous()
    return img_list, torch.from_numpy(np.ascontiguousarray(np.stack(cropped))), (sy, sx)
