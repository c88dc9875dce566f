"""From the network's predictions to the point cloud of a scan, on the GPU: batched confidence filter into the fusion.

The reference connects its stages through files: ``eval_file_logger`` writes every view's maps, ``tools/depthfusion.py``
reads them back, filters each depth map by its two confidence maps (``probability_filter``, depthfusion.py:153-170) and
hands the result to fusibile.  Here the predictions of all views stay on the device: ``ScanAccumulator`` collects them,
``filter_depth_maps`` filters the V views in one launch (csrc/scan_filter.hip) and ``fuse_depth_maps`` takes its output.

The filter
----------
``filtered = depth`` where ``flow_conf >= flow_prob_threshold`` and ``init_conf_resized >= init_prob_threshold``, else 0;
the comparisons are NumPy's ``depth[conf < thr] = 0``, so a NaN confidence keeps the depth.  The flow confidence of raw
``(V, 5, h, w)`` hypothesis probabilities is that of ``eval_file_logger`` (float64 index, float32 sum).  A confidence map
of the depth map's size is used as it is; any other size is resized, as the reference does with ``cv2.resize`` in the mode
of its ``-m/--inter_mode`` (default ``LANCZOS4``).

The resampling specification
----------------------------
**This project's own statement of what cv2.resize does to float32 images.**  On uint8 OpenCV runs fixed-point kernels; on
float32 it is plain separable float arithmetic with closed-form weights, which is stated here.  OpenCV is not a
dependency: bit parity with ``cv2.resize`` is neither claimed nor tested.  For destination size ``n`` from source size
``s``, per axis and destination index ``i``:

* ``NEAREST``: one tap at ``min(floor(i * (s / n)), s - 1)`` with weight 1 (the rule of
  ``eval_file_logger._resize_nearest``; the value itself, no product).
* the others: ``f = (i + 0.5) * (s / n) - 0.5``, ``i0 = floor(f)``, ``t = f - i0``; taps at ``i0 + k``, each **clamped to
  [0, s - 1]** (replicate border); no prefiltering when shrinking.

  - ``BILINEAR``: ``k = 0, 1``, weights ``(1 - t, t)``.
  - ``CUBIC``: ``k = -1 .. 2``, Keys' kernel with ``A = -0.75``:
    ``w(-1) = ((A (t + 1) - 5 A) (t + 1) + 8 A) (t + 1) - 4 A``, ``w(0) = ((A + 2) t - (A + 3)) t^2 + 1``,
    ``w(1) = ((A + 2) (1 - t) - (A + 3)) (1 - t)^2 + 1``, ``w(2) = 1 - w(-1) - w(0) - w(1)``.
  - ``LANCZOS4``: ``k = -3 .. 4``, ``L(t - k)`` with ``L(x) = sinc(x) sinc(x / 4)`` for ``|x| < 4`` (``sinc(x) =
    sin(pi x) / (pi x)``), divided by their sum; at ``t = 0`` exactly ``(0, 0, 0, 1, 0, 0, 0, 0)``.

``resize_taps`` composes the tables (first tap's index, weights) in float64; the kernel gets the weights as float32 and
evaluates horizontally first, then vertically, in float32, each sum in ascending tap order.  Departures from OpenCV that
are known: OpenCV computes its LANCZOS4 weights with a rotation recurrence in float32 and its CUBIC weights in float32,
so its results differ from this statement in the last bits; a zero weight times an infinite sample is NaN here as there.
"""
import numpy as np
import torch

from . import _lib, mesh_ops, mesh_simplify
from .cloud_filter import clean_cloud
from .depth_segments import check_clean_settings, clean_depth_maps
from .fusion import fuse_depth_maps
from .geometric import geometric_filter
from .normals import depth_normals
from .photometric import photometric_consistency, photometric_filter
from .refine import scale_of, upsample_depth_maps, upsampled_intrinsics
from .render import depth_map_errors, render_depth_maps, render_mesh_depth_maps
from .sparse_tsdf import MAX_VIRTUAL_SAMPLES, SparseTSDFVolume
from .tsdf import TSDFVolume, dims_for, volume_bounds
from .utils.eval_file_logger import _resize_nearest, _scene_paths
from .utils.io import write_ply

# name -> (PF_SCAN_* of include/pointflow_hip.h, taps per axis)
MODES = {"NEAREST": (0, 1), "BILINEAR": (1, 2), "CUBIC": (2, 4), "LANCZOS4": (4, 8)}


def _mode(mode):
    if mode not in MODES:
        raise ValueError("unknown interpolation mode %r (one of %s)" % (mode, ", ".join(sorted(MODES))))
    return MODES[mode]


def resize_taps(src, dst, mode):
    """The tap tables of one axis, ``(start (dst,) int64, weights (dst, T) float64)``: destination index ``i`` reads the
    source indices ``clip(start[i] + k, 0, src - 1)``, ``k = 0 .. T-1``, with ``weights[i, k]`` (module docstring)."""
    _, T = _mode(mode)
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1:
        raise ValueError("resize_taps: sizes must be at least 1")
    i = np.arange(dst, dtype=np.float64)
    scale = src / float(dst)
    if mode == "NEAREST":
        return np.minimum(np.floor(i * scale).astype(np.int64), src - 1), np.ones((dst, 1))
    f = (i + 0.5) * scale - 0.5
    i0 = np.floor(f)
    t = f - i0
    if mode == "BILINEAR":
        weights = np.stack([1.0 - t, t], axis=1)
    elif mode == "CUBIC":
        A = -0.75
        w0 = ((A * (t + 1.0) - 5.0 * A) * (t + 1.0) + 8.0 * A) * (t + 1.0) - 4.0 * A
        w1 = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0
        w2 = ((A + 2.0) * (1.0 - t) - (A + 3.0)) * (1.0 - t) * (1.0 - t) + 1.0
        weights = np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], axis=1)
    else:
        x = t[:, None] - np.arange(-3.0, 5.0)[None, :]
        weights = np.where(np.abs(x) < 4.0, np.sinc(x) * np.sinc(x / 4.0), 0.0)
        weights = weights / weights.sum(axis=1, keepdims=True)
        weights[t == 0.0] = np.eye(8)[3]
    return i0.astype(np.int64) - (T // 2 - 1), weights


def _tables(src_hw, dst_hw, mode, dev):
    """The four device tables of one map (ys, yw, xs, xw), or Nones when the map needs no resampling."""
    if tuple(src_hw) == tuple(dst_hw):
        return None, None, None, None
    out = []
    for s, n in zip(src_hw, dst_hw):
        start, weights = resize_taps(s, n, mode)
        out.append(torch.from_numpy(start.astype(np.int32)).to(dev))
        out.append(torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32)).to(dev))
    return tuple(out)


def filter_depth_maps(depths, flow_probs, init_probs, init_prob_threshold=0.2, flow_prob_threshold=0.1, mode="LANCZOS4",
                      return_kept=False, return_stages=False):
    """The confidence filter of the module docstring for all views at once, on the GPU.

    ``depths`` (V, h, w); ``flow_probs`` (V, 5, h, w) raw hypothesis probabilities or (V, fh, fw) confidences;
    ``init_probs`` (V, ih, iw) (a (V, 1, ih, iw) tensor is accepted).  Returns ``filtered`` (V, h, w) float32 contiguous,
    what ``fuse_depth_maps`` takes; with ``return_kept`` also the (V,) int32 count of pixels per view that the filter did
    not zero; with ``return_stages`` last the dict of the confidences the comparisons saw, ``flow_conf`` and ``init_conf``
    (V, h, w).  There is no CPU path."""
    code, T = _mode(mode)
    for name, t in (("depths", depths), ("flow_probs", flow_probs), ("init_probs", init_probs)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("filter_depth_maps: %s must be a tensor" % name)
    if depths.dim() != 3:
        raise ValueError("filter_depth_maps: depths must be (V, h, w)")
    V, h, w = (int(s) for s in depths.shape)
    if init_probs.dim() == 4 and init_probs.shape[1] == 1:
        init_probs = init_probs[:, 0]
    if init_probs.dim() != 3 or init_probs.shape[0] != V:
        raise ValueError("filter_depth_maps: init_probs must be (V, ih, iw) with the V of depths")
    raw = flow_probs.dim() == 4
    if raw and tuple(flow_probs.shape) != (V, 5, h, w):
        raise ValueError("filter_depth_maps: raw flow_probs must be (V, 5, h, w) of the depth maps' size")
    if not raw and (flow_probs.dim() != 3 or flow_probs.shape[0] != V):
        raise ValueError("filter_depth_maps: flow_probs must be (V, 5, h, w) or (V, fh, fw) with the V of depths")
    if min(init_probs.shape[1:]) < 1 or min(flow_probs.shape[-2:]) < 1:
        raise ValueError("filter_depth_maps: empty confidence maps")
    _lib.require_gpu(depths, flow_probs, init_probs)
    dev = depths.device
    depths = depths.contiguous().float()
    flow_probs = flow_probs.contiguous().float()
    init_probs = init_probs.contiguous().float()
    fh, fw = (h, w) if raw else (int(s) for s in flow_probs.shape[1:])
    ih, iw = (int(s) for s in init_probs.shape[1:])
    with _lib.on_device(dev):
        filtered = torch.empty((V, h, w), dtype=torch.float32, device=dev)
        kept = torch.zeros((V,), dtype=torch.int32, device=dev)
        stages = None
        if return_stages:
            stages = {"flow_conf": torch.empty((V, h, w), dtype=torch.float32, device=dev),
                      "init_conf": torch.empty((V, h, w), dtype=torch.float32, device=dev)}
        if V and h and w:
            if not _lib.load().pf_scan_filter_supported(code, h, w, fh, fw, ih, iw):
                raise ValueError("filter_depth_maps: sizes %s <- flow %s, init %s are outside what the kernel is built for "
                                 "(pf_scan_filter_supported, include/pointflow_hip.h)" % ((h, w), (fh, fw), (ih, iw)))
            flow_t = _tables((fh, fw), (h, w), mode, dev)
            init_t = _tables((ih, iw), (h, w), mode, dev)
            # per pixel: depth, the flow confidence's input, the coarse confidence's share, the output
            algo = V * (h * w * (4 + (20 if raw else 0) + 4) + (0 if raw else 4 * fh * fw) + 4 * ih * iw)
            _lib.call("pf_scan_filter_f32", _lib.ptr(depths), _lib.ptr(flow_probs if raw else None),
                      _lib.ptr(None if raw else flow_probs), fh, fw, _lib.ptr(init_probs), ih, iw, V, h, w, code,
                      *([_lib.ptr(t) for t in flow_t] + [_lib.ptr(t) for t in init_t]), float(flow_prob_threshold),
                      float(init_prob_threshold), _lib.ptr(filtered), _lib.ptr(kept),
                      _lib.ptr(stages["flow_conf"] if stages else None), _lib.ptr(stages["init_conf"] if stages else None),
                      _lib.stream(), algo_bytes=algo, tag=mode)
    out = (filtered,) + ((kept,) if return_kept else ()) + ((stages,) if return_stages else ())
    return out[0] if len(out) == 1 else out


class ScanAccumulator(object):
    """Collects the predictions of the ``view_num`` views of one scan on the device and turns them into the point cloud.

    ``add(data_batch, preds)`` after every forward; then ``filtered()``, ``cameras()``, ``normals()``, ``fuse()``,
    ``write_ply(path)``, ``mesh(voxel)``, ``write_mesh(path, voxel=...)``.
    ``name`` is the depth map that is fused (``preds[name]``, ``preds[name + "_prob"]``), ``mode`` and the thresholds are
    those of ``filter_depth_maps``; ``keep_images`` keeps the views' images for the cloud's colours; ``keep_guides`` also
    keeps every view's full ``ref_img`` as RGB on the device, what ``upsampled()`` and ``fuse(upsample=...)`` are guided
    by.  ``clean_depth``: a dict of ``depth_segments.clean_depth_maps``' keyword arguments (an empty one for its defaults);
    ``filtered()`` then returns the filtered maps with their speckles removed and their gaps filled, and everything that
    consumes ``filtered()`` follows: ``fuse``, ``geometric``, ``normals``, ``upsampled``, ``mesh`` and
    ``depth_errors(filtered=True)``.  The report of the latest cleaning is kept as ``last_depth_report``.  With ``None``
    every method returns what it returned without the option.  ``photometric()`` scores the maps against the kept images
    (``photometric.py``), and ``fuse(photo={...})`` removes what fails that check before fusing; the report of the latest such
    call is kept as ``last_photo_report``."""

    def __init__(self, view_num, name="flow2", mode="LANCZOS4", init_prob_threshold=0.2, flow_prob_threshold=0.1,
                 keep_images=True, keep_guides=False, clean_depth=None):
        _mode(mode)
        if int(view_num) < 1:
            raise ValueError("ScanAccumulator: view_num must be at least 1")
        if clean_depth is not None:
            if not isinstance(clean_depth, dict):
                raise ValueError("ScanAccumulator: clean_depth must be a dict of clean_depth_maps' keyword arguments or None")
            try:
                check_clean_settings("ScanAccumulator: clean_depth", **clean_depth)
            except TypeError as exc:
                raise ValueError("ScanAccumulator: clean_depth: %s" % exc)
            clean_depth = dict(clean_depth)
        self.clean_depth = clean_depth
        self.last_depth_report = None
        self.view_num, self.name, self.mode = int(view_num), name, mode
        self.init_prob_threshold, self.flow_prob_threshold = float(init_prob_threshold), float(flow_prob_threshold)
        self.keep_images, self.keep_guides = keep_images, bool(keep_guides)
        self._guides = None
        self._with_guide = 0
        self._seen = [False] * self.view_num
        self._depth = self._flow = self._init = self._images = None
        self.last_clean_report = None
        self.last_photo_report = None
        self.last_mesh_report = None
        self.last_simplify_report = None
        self.last_sparse_report = None
        self._with_image = 0
        self._K = np.zeros((self.view_num, 3, 3))
        self._E = np.zeros((self.view_num, 4, 4))

    def add(self, data_batch, preds, view_index=None):
        """Store one view.  ``view_index`` defaults to the index ``eval_file_logger`` derives from
        ``data_batch["ref_img_path"]`` (``rect_007_...`` -> 6)."""
        if view_index is None:
            path = data_batch["ref_img_path"]
            view_index = _scene_paths(path if isinstance(path, str) else path[0], "")[1]
        v = int(view_index)
        if not 0 <= v < self.view_num:
            raise ValueError("ScanAccumulator: view %d of %d" % (v, self.view_num))
        if self._seen[v]:
            raise ValueError("ScanAccumulator: view %d was added before" % v)
        for key in (self.name, self.name + "_prob", "coarse_prob_map"):
            if key not in preds:
                raise ValueError("ScanAccumulator: the predictions have no %r" % key)
        depth, flow, init = preds[self.name][0, 0], preds[self.name + "_prob"][0], preds["coarse_prob_map"][0, 0]
        _lib.require_gpu(depth, flow, init)
        if self._depth is None:
            dev, V = depth.device, self.view_num
            self._depth = torch.zeros((V,) + tuple(depth.shape), dtype=torch.float32, device=dev)
            self._flow = torch.zeros((V,) + tuple(flow.shape), dtype=torch.float32, device=dev)
            self._init = torch.zeros((V,) + tuple(init.shape), dtype=torch.float32, device=dev)
        for buf, t, what in ((self._depth, depth, "depth map"), (self._flow, flow, "flow probabilities"),
                             (self._init, init, "coarse confidence")):
            if tuple(t.shape) != tuple(buf.shape[1:]):
                raise ValueError("ScanAccumulator: view %d's %s is %s, the first view's %s"
                                 % (v, what, tuple(t.shape), tuple(buf.shape[1:])))
        # Enqueued on the current stream, no host synchronisation: GraphedForward / LanedForward hand out STATIC buffers that
        # the next replay on this stream overwrites, and the replay is ordered behind these copies (the hazard that the
        # comment in AsyncEvalWriter.submit describes; there the packs run on a side stream, here on the producer's own).
        self._depth[v].copy_(depth, non_blocking=True)
        self._flow[v].copy_(flow, non_blocking=True)
        self._init[v].copy_(init, non_blocking=True)
        h, w = (int(s) for s in depth.shape)
        cams = data_batch.get("cam_params_list_host")
        if cams is None:
            cams = data_batch["cam_params_list"].detach().cpu()
        cam = cams.numpy()[0, 0].copy()
        ref = data_batch.get("ref_img")
        ref_h = int(ref.shape[1]) if ref is not None else int(data_batch["img_list"].shape[3])
        cam[1, :2, :3] *= (float(h) / float(ref_h))            # cam_file of eval_file_logger_host, in the cameras' dtype
        self._K[v], self._E[v] = cam[1, :3, :3], cam[0]
        if self.keep_guides and ref is not None:
            full = torch.as_tensor(ref)[0]
            if full.dim() != 3 or full.shape[2] != 3 or full.dtype != torch.uint8:
                raise ValueError("ScanAccumulator: ref_img must be (1, H, W, 3) uint8")
            if self._guides is None:
                self._guides = torch.zeros((self.view_num,) + tuple(full.shape), dtype=torch.uint8, device=self._depth.device)
            if tuple(full.shape) != tuple(self._guides.shape[1:]):
                raise ValueError("ScanAccumulator: view %d's ref_img is %s, the first view's %s"
                                 % (v, tuple(full.shape), tuple(self._guides.shape[1:])))
            self._guides[v].copy_(full.flip(-1), non_blocking=True)          # BGR -> RGB, as the images below
            self._with_guide += 1
        if self.keep_images and ref is not None:
            img = torch.as_tensor(ref)[0]
            if img.dim() != 3 or img.shape[2] != 3 or img.dtype != torch.uint8:
                raise ValueError("ScanAccumulator: ref_img must be (1, H, W, 3) uint8")
            if tuple(img.shape[:2]) != (h, w):                 # _load_image: nearest-resized, then BGR -> RGB
                ys = np.arange(img.shape[0])[:, None]
                xs = np.arange(img.shape[1])[None, :]
                ys, xs = _resize_nearest(ys, h, 1)[:, 0], _resize_nearest(xs, 1, w)[0]
                img = img[torch.from_numpy(ys).to(img.device)][:, torch.from_numpy(xs).to(img.device)]
            if self._images is None:
                self._images = torch.zeros((self.view_num, h, w, 3), dtype=torch.uint8, device=self._depth.device)
            self._images[v].copy_(img.flip(-1), non_blocking=True)
            self._with_image += 1
        self._seen[v] = True

    def _require_complete(self, what):
        missing = [v for v, s in enumerate(self._seen) if not s]
        if missing:
            raise ValueError("ScanAccumulator.%s: views %s have not been added" % (what, missing))

    def predictions(self):
        """The stacked ``(depths (V, h, w), flow_probs (V, 5, h, w), init_probs (V, ih, iw))`` of the added views."""
        self._require_complete("predictions")
        return self._depth, self._flow, self._init

    def filtered(self, return_kept=False):
        """``filter_depth_maps`` of the accumulated views: (V, h, w); with ``clean_depth``, ``clean_depth_maps`` of that
        (``kept`` stays the confidence filter's own count)."""
        self._require_complete("filtered")
        out = filter_depth_maps(self._depth, self._flow, self._init, self.init_prob_threshold, self.flow_prob_threshold,
                                self.mode, return_kept=return_kept)
        if self.clean_depth is None:
            return out
        cleaned, self.last_depth_report = clean_depth_maps(out[0] if return_kept else out, **self.clean_depth)
        return (cleaned, out[1]) if return_kept else cleaned

    def cameras(self):
        """``(intrinsics (V, 3, 3) of the depth maps' grid, extrinsics (V, 4, 4))`` as float64 NumPy."""
        self._require_complete("cameras")
        return self._K.copy(), self._E.copy()

    def images(self):
        """(V, h, w, 3) uint8 RGB on the device, or None unless every view came with a ``ref_img``."""
        return self._images if self._with_image == self.view_num else None

    def guides(self):
        """(V, H, W, 3) uint8 RGB on the device, the views' full ``ref_img``; None unless the accumulator was built with
        ``keep_guides`` and every view came with a ``ref_img``."""
        return self._guides if self._with_guide == self.view_num else None

    def upsampled(self, **kwargs):
        """``(depths_hi (V, H, W), K_hi (V, 3, 3), E (V, 4, 4), guides (V, H, W, 3))``: ``refine.upsample_depth_maps`` of
        ``filtered()`` guided by the kept ``guides()`` (``kwargs``: its settings), with ``refine.upsampled_intrinsics`` of
        ``cameras()``.  A ValueError without guides, or when ``H, W`` are not one integer multiple of ``h, w``."""
        self._require_complete("upsampled")
        guides = self.guides()
        if guides is None:
            raise ValueError("ScanAccumulator.upsampled: no guides were kept (keep_guides=True and a ref_img with every view)")
        s = scale_of("ScanAccumulator.upsampled", self._depth.shape[1:], guides.shape[1:3])
        K, E = self.cameras()
        return upsample_depth_maps(self.filtered(), guides, **kwargs), upsampled_intrinsics(K, s), E, guides

    def geometric(self, sources=None, upsample=None, **kwargs):
        """``geometric.geometric_filter`` of ``filtered()``, ``cameras()`` and ``images()``: ``(depth_avg, mask, count)`` and,
        unless ``return_points=False``, ``points`` and ``colours``.  ``sources``: the (V, M) table of source views (None: all
        other views); ``kwargs``: its thresholds.  ``upsample``: a dict of ``refine.upsample_depth_maps``' keyword arguments;
        the filter then runs on ``upsampled()`` with the guides as the images."""
        self._require_complete("geometric")
        if upsample is not None:
            depths, K, E, guides = self.upsampled(**upsample)
            return geometric_filter(depths, K, E, images=guides, sources=sources, **kwargs)
        K, E = self.cameras()
        return geometric_filter(self.filtered(), K, E, images=self.images(), sources=sources, **kwargs)

    def photometric(self, sources=None, upsample=None, **kwargs):
        """``photometric.photometric_consistency`` of ``filtered()``, ``cameras()`` and ``images()``: ``(score, mask, count,
        usable)`` and, with ``return_per_source``, ``ncc``.  ``sources``: the (V, M) table of source views (None: all other
        views); ``kwargs``: its settings.  ``images()`` are the views' images nearest-resized to the depth maps' grid, so
        the windows compare subsampled images; ``upsample``: a dict of ``refine.upsample_depth_maps``' keyword arguments, with
        which the check runs on ``upsampled()`` with the guides as the images -- the images as they were taken, the honest
        resolution for a photometric test.  A ValueError without images."""
        self._require_complete("photometric")
        if upsample is not None:
            depths, K, E, images = self.upsampled(**upsample)
        else:
            (K, E), depths, images = self.cameras(), self.filtered(), self.images()
        if images is None:
            raise ValueError("ScanAccumulator.photometric: no images were kept (keep_images=True and a ref_img with every view)")
        return photometric_consistency(depths, images, K, E, sources=sources, **kwargs)

    def normals(self, step=1, rel_jump=0.01):
        """``normals.depth_normals`` of ``filtered()`` and ``cameras()``: (V, h, w, 3) unit normals facing their camera."""
        self._require_complete("normals")
        K, E = self.cameras()
        return depth_normals(self.filtered(), K, E, step=step, rel_jump=rel_jump)

    def fuse(self, disp_threshold=0.12, num_consistent=3, depth_min=1e-3, depth_max=1e5, method="disparity",
             with_normals=False, normal_step=1, normal_rel_jump=0.01, clean=None, upsample=None, photo=None, **kwargs):
        """``(points (N, 3) float32, colours (N, 3) uint8 or None)``: with ``method="disparity"`` through
        ``fuse_depth_maps``; with ``method="roundtrip"`` the cloud of ``geometric()`` (``disp_threshold`` is not used;
        ``kwargs``: ``sources``, ``pix_threshold``, ``rel_depth_threshold``).  With ``with_normals`` a third value, the
        points' normals (N, 3) float32 as the method's fuser defines them (``normals.py``).  ``clean``: a dict of
        ``cloud_filter.clean_cloud``'s keyword arguments, applied to the cloud of either method with its colours and
        normals carried through; its report is kept as ``last_clean_report`` (None after a call without ``clean``).  ``None``
        leaves the fuser's cloud as it is.  ``upsample``: a dict of ``refine.upsample_depth_maps``' keyword arguments (an empty
        one for its defaults); either method then fuses ``upsampled()`` -- the maps on the guides' grid with that grid's
        intrinsics, colours taken from the guides -- and ``with_normals`` and ``clean`` act on that cloud.  It needs an
        accumulator built with ``keep_guides``.  ``photo``: a dict of ``photometric.photometric_filter``'s keyword arguments
        (``sources`` among them; an empty one for its defaults); the maps -- the upsampled ones under ``upsample``, with the
        guides as their images -- then pass that filter before either method's fuser, and its report is kept as
        ``last_photo_report`` (None after a call without ``photo``).  It needs the views' images."""
        if method not in ("disparity", "roundtrip"):
            raise ValueError("ScanAccumulator.fuse: unknown method %r (disparity or roundtrip)" % (method,))
        if clean is not None and not isinstance(clean, dict):
            raise TypeError("ScanAccumulator.fuse: clean must be a dict of clean_cloud's keyword arguments or None")
        if upsample is not None and not isinstance(upsample, dict):
            raise TypeError("ScanAccumulator.fuse: upsample must be a dict of upsample_depth_maps' keyword arguments or None")
        if photo is not None and not isinstance(photo, dict):
            raise TypeError("ScanAccumulator.fuse: photo must be a dict of photometric_filter's keyword arguments or None")
        if upsample is not None and not self.keep_guides:
            raise ValueError("ScanAccumulator.fuse: upsample needs an accumulator built with keep_guides=True")
        self._require_complete("fuse")
        normal_kwargs = {}
        if with_normals:
            normal_kwargs = {"with_normals": True, "normal_step": normal_step, "normal_rel_jump": normal_rel_jump}
        if method == "disparity" and kwargs:
            raise TypeError("ScanAccumulator.fuse: %s belong to method=\"roundtrip\"" % ", ".join(sorted(kwargs)))
        if upsample is not None:
            depths, K, E, images = self.upsampled(**upsample)
        else:
            (K, E), depths, images = self.cameras(), self.filtered(), self.images()
        self.last_photo_report = None
        if photo is not None:
            if images is None:
                raise ValueError("ScanAccumulator.fuse: photo needs the views' images (keep_images=True and a ref_img with "
                                 "every view)")
            depths, self.last_photo_report = photometric_filter(depths, images, K, E, **photo)
        if method == "roundtrip":
            kwargs.update(normal_kwargs)
            fused = geometric_filter(depths, K, E, images=images, num_consistent=num_consistent, depth_min=depth_min,
                                     depth_max=depth_max, **kwargs)[3:6 if with_normals else 5]
        else:
            fused = fuse_depth_maps(depths, K, E, images=images, disp_threshold=disp_threshold,
                                    num_consistent=num_consistent, depth_min=depth_min, depth_max=depth_max, **normal_kwargs)
        self.last_clean_report = None
        if clean is None:
            return fused
        points, colours, normals, self.last_clean_report = clean_cloud(
            fused[0], fused[1], fused[2] if with_normals else None, **clean)
        return (points, colours) + ((normals,) if with_normals else ())

    def depth_errors(self, gt_points, thresholds, splat=1, filtered=True, gt_faces=None):
        """``render.depth_map_errors`` of the accumulated depth maps -- ``filtered()``, or the raw ``predictions()[0]`` with
        ``filtered=False`` -- against ``gt_points`` (N, 3) float32 on the GPU (the scan's ground-truth cloud) rendered into
        ``cameras()`` at the depth maps' size with ``render.render_depth_maps(..., splat=splat)``.  With ``gt_faces`` (Nf, 3)
        ``gt_points`` are the vertices of the scan's ground-truth *mesh* and the ground truth is rasterised
        (``render.render_mesh_depth_maps``; ``splat`` is ignored): no holes, and no back of the scene seen through a nearer
        surface."""
        self._require_complete("depth_errors")
        K, E = self.cameras()
        pred = self.filtered() if filtered else self._depth
        h, w = int(pred.shape[1]), int(pred.shape[2])
        if gt_faces is not None:
            return depth_map_errors(pred, render_mesh_depth_maps(gt_points, gt_faces, K, E, h, w), thresholds)
        return depth_map_errors(pred, render_depth_maps(gt_points, K, E, h, w, splat=splat), thresholds)

    def render_mesh(self, vertices, faces, **kwargs):
        """``render.render_mesh_depth_maps`` of a mesh into ``cameras()`` at the depth maps' size (``kwargs``: its depth
        range, ``cull``, ``return_index``, ``return_barycentric``).  With ``mesh()``'s own vertices and faces: the fused,
        hole-filled depth map of every view."""
        self._require_complete("render_mesh")
        K, E = self.cameras()
        return render_mesh_depth_maps(vertices, faces, K, E, int(self._depth.shape[1]), int(self._depth.shape[2]), **kwargs)

    def mesh(self, voxel, trunc=None, min_weight=2, bounds=None, filtered=True, with_colour=True,
             min_component_faces=None, keep_largest=None, with_normals=False, sparse=False, simplify_cell=None,
             simplify_placement="quadric"):
        """``(vertices (Nv, 3) float32, faces (Nf, 3) int32, colours (Nv, 3) uint8 or None)``: the accumulated depth maps --
        ``filtered()``, or the raw ``predictions()[0]`` with ``filtered=False`` -- integrated into a ``tsdf.TSDFVolume`` of
        pitch ``voxel`` and truncation ``trunc`` (default ``4 * voxel``) over the box ``bounds = (lo, hi)`` (default:
        ``tsdf.volume_bounds`` of the maps used, grown by ``trunc``), and its zero surface through the cells whose corners
        were all seen by ``min_weight`` views (``tsdf.extract_mesh``).  Colours need the views' images.  With ``sparse`` the
        same call goes through a ``sparse_tsdf.SparseTSDFVolume`` (the same vertices and colours byte for byte and the same
        faces in another order; ``min_weight >= 1``; the grid may then have more than 2^31 samples), whose ``report()`` is
        kept as ``last_sparse_report`` (None after a dense call).

        ``min_component_faces`` and ``keep_largest`` drop the mesh's small connected components
        (``mesh_ops.remove_small_components``: ``min_faces``, ``keep_largest``); the report -- ``components``,
        ``vertices_before`` / ``_after``, ``faces_before`` / ``_after``, ``rounds`` -- is kept as ``last_mesh_report`` (None
        after a call with neither).  With ``simplify_cell`` the mesh that is left is simplified by vertex clustering on a grid
        of that edge (``mesh_simplify.simplify_mesh`` with ``placement=simplify_placement``), after the small pieces have
        gone, so that floaters add no quadrics; its report is kept as ``last_simplify_report`` (None after a call without).
        With ``with_normals`` a fourth value, the vertex normals (Nv, 3) float32 of the mesh that is returned
        (``mesh_ops.vertex_normals``)."""
        mesh_ops._check_selection("ScanAccumulator.mesh", min_component_faces, keep_largest)
        if simplify_cell is not None:
            mesh_simplify.check_simplify_arguments("ScanAccumulator.mesh", simplify_cell, simplify_placement)
        elif simplify_placement not in mesh_simplify.PLACEMENTS:
            raise ValueError("ScanAccumulator.mesh: placement must be one of %s" % ", ".join(mesh_simplify.PLACEMENTS))
        self._require_complete("mesh")
        voxel = float(voxel)
        trunc = 4.0 * voxel if trunc is None else float(trunc)
        K, E = self.cameras()
        depths = self.filtered() if filtered else self._depth
        if bounds is None:
            bounds = volume_bounds(depths, K, E, pad=trunc)
        origin, dims = dims_for(bounds, voxel, max_samples=MAX_VIRTUAL_SAMPLES if sparse else None)
        images = self.images() if with_colour else None
        volume = (SparseTSDFVolume if sparse else TSDFVolume)(origin, voxel, dims, trunc, with_colour=images is not None,
                                                              device=depths.device)
        volume.integrate(depths, K, E, images=images)
        vertices, faces, colours = volume.extract(min_weight)[:3]
        self.last_sparse_report = volume.report() if sparse else None
        self.last_mesh_report = None
        if min_component_faces is not None or keep_largest is not None:
            Nv, Nf = int(vertices.shape[0]), int(faces.shape[0])
            faces32 = mesh_ops._faces32("ScanAccumulator.mesh", faces, Nv, vertices)
            with _lib.on_device(faces32.device):
                label, rounds = mesh_ops._components(faces32, Nv)
                face_keep, components = mesh_ops._select_faces(mesh_ops._face_labels(faces32, Nv, label),
                                                               min_component_faces, keep_largest)
                vertices, faces, colours = mesh_ops._compact(vertices, faces, face_keep, colours, None)[:3]
            self.last_mesh_report = {"components": components, "vertices_before": Nv, "vertices_after": int(vertices.shape[0]),
                                     "faces_before": Nf, "faces_after": int(faces.shape[0]), "rounds": rounds}
        self.last_simplify_report = None
        if simplify_cell is not None:
            vertices, faces, colours, self.last_simplify_report = mesh_simplify.simplify_mesh(
                vertices, faces, simplify_cell, colours=colours, placement=simplify_placement)
        if with_normals:
            return vertices, faces, colours, mesh_ops.vertex_normals(vertices, faces)
        return vertices, faces, colours

    def write_mesh(self, path, **mesh_kwargs):
        """``mesh(**mesh_kwargs)`` written to ``path`` as a PLY with faces (and, ``with_normals``, the vertex normals); returns
        what ``mesh`` returned."""
        mesh = self.mesh(**mesh_kwargs)
        vertices, faces, colours = mesh[:3]
        write_ply(path, vertices.cpu().numpy(), None if colours is None else colours.cpu().numpy(),
                  mesh[3].cpu().numpy() if len(mesh) > 3 else None, faces=faces.cpu().numpy())
        return mesh

    def write_ply(self, path, **fuse_kwargs):
        """Fuse (``fuse_kwargs``: those of ``fuse``, ``method``, ``with_normals`` and ``clean`` among them) and write the cloud to
        ``path``; returns what ``fuse`` returned: ``(points, colours)`` and, ``with_normals``, the normals."""
        fused = self.fuse(**fuse_kwargs)
        write_ply(path, fused[0].cpu().numpy(), None if fused[1] is None else fused[1].cpu().numpy(),
                  fused[2].cpu().numpy() if len(fused) > 2 else None)
        return fused


def reconstruct_scan(model, batches, img_scales=(0.125, 0.25, 0.5), inter_scales=(1.0, 0.75, 0.15), view_num=None,
                     fuse_kwargs=None, **accumulator_kwargs):
    """Run ``model`` on every ``data_batch`` of one scan (any iterable; one view as the reference each), accumulate the
    views and fuse them: ``(points, colours, accumulator)``, or ``(points, colours, normals, accumulator)`` when
    ``fuse_kwargs`` asks ``with_normals``.  A ``clean`` entry of ``fuse_kwargs`` cleans the cloud (``ScanAccumulator.fuse``); an
    ``upsample`` entry fuses the guided-upsampled maps and needs ``keep_guides=True`` among ``accumulator_kwargs``; a
    ``photo`` entry passes the maps through ``photometric.photometric_filter`` first.

    A ``torch.nn.Module`` is called as the evaluation forward, ``model(data_batch, img_scales, inter_scales, isFlow=True,
    isTest=True)`` under ``torch.no_grad()``; anything else (a ``GraphedForward``) as ``model(data_batch)``.  ``view_num``
    defaults to ``len(batches)``; a batch may carry its ``view_index``, else ``ref_img_path`` tells it, else its position."""
    if view_num is None:
        batches = list(batches)
        view_num = len(batches)
    acc = ScanAccumulator(view_num, **accumulator_kwargs)
    with torch.no_grad():
        for position, data_batch in enumerate(batches):
            if isinstance(model, torch.nn.Module):
                preds = model(data_batch, img_scales, inter_scales, isFlow=True, isTest=True)
            else:
                preds = model(data_batch)
            index = data_batch.get("view_index")
            if index is None and "ref_img_path" not in data_batch:
                index = position
            acc.add(data_batch, preds, view_index=index)
    return tuple(acc.fuse(**(fuse_kwargs or {}))) + (acc,)
