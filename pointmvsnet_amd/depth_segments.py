"""Depth-map segments on the GPU: connected components on the pixel grid, speckle removal and gap filling.

The confidence filter and the fusers decide pixel by pixel; ``clean_cloud`` removes floaters only once they are points.
Two artefacts are only visible on the depth map's own grid, which names a depth's true surface neighbours: *speckles*,
islands of a few dozen pixels that pass the confidence filter, agree with each other and sit at the wrong depth, and
*pin-holes*, runs of a few pixels that the filter zeroed inside a smooth surface.  This module removes the first and
interpolates over the second, between ``filter_depth_maps`` and everything that consumes its maps.  It runs as six HIP
kernels (csrc/depth_segments.hip).  **The specification below is this project's own**; parity with OpenCV
(``filterSpeckles``), OpenMVS (``nSpeckleSize``) or COLMAP is neither claimed nor tested.  Every decision is float32
exactly as written (the library is built with ``-ffp-contract=off``), so a NumPy float32 statement reproduces every output
bit for bit, and every result is a pure function of the input: two runs give identical bytes.

Input
-----
``depths`` (V, h, w) float32 on the GPU.  ``valid(q)``: ``depth_min < d(q) < depth_max`` (``0 <= depth_min < depth_max``);
NaN, +-inf and 0 are not valid.  ``V * h * w`` must be below ``2^31``; more is a ValueError.  ``V == 0`` and ``h * w == 0``
return empty outputs and launch nothing.  Arguments are checked before a GPU is needed.  There is no CPU path.

Link
----
Two 4-neighbours ``p``, ``q`` of the same view are linked iff both are valid and
``|d(p) - d(q)| <= rel_jump * min(d(p), d(q))``; the subtraction, the product and the comparison are float32.  The rule is
symmetric on purpose -- unlike the one-sided ``rel_jump`` rule of ``depth_normals`` -- so that segments are well defined.
There are never links across the right / left edge of a row, across the last / first row of consecutive views, or to a
pixel outside the map.  ``0 <= rel_jump <= 0.5``.

Segments
--------
A segment is a connected component of the link graph.  ``depth_segments(depths, rel_jump=0.01, depth_min=1e-3,
depth_max=1e5, return_sizes=False)`` returns ``labels`` (V, h, w) int32: a valid pixel's label is the flat index into the
(V, h, w) array of the first pixel of its segment in row-major order; a pixel that is not valid has label ``-1``.  With
``return_sizes`` it also returns ``sizes`` (V, h, w) int32, the number of pixels of the pixel's segment (0 where not valid).

The route: one block per tile of ``TILE_W x TILE_H`` pixels finds the components of the links inside its tile in LDS and
writes every pixel's tile-local root as a global flat index; then the hook-and-compress scheme of ``mesh_components`` joins
the pieces over the edges that cross tile borders only.  A *round* is a merge launch over those edges and a compress
launch; the host reads one counter per round (the edges whose ends had two different roots) and stops on a clean round,
whose compress launch it leaves out: a merge that found nothing to unite stored nothing.
``last_segment_stats()`` tells the rounds, the border edges per view and the border edges united of the latest call
(the edges per view follow from the shape; the other two also depend on the order in which the merge's threads ran).
Sizes are integer sums -- they do not depend on the order: pieces are counted per tile in LDS, then one ``atomicAdd`` per
piece goes to the segment's root.

Speckles
--------
``remove_speckles(depths, min_size=100, rel_jump=0.01, depth_min=1e-3, depth_max=1e5, return_removed=False)`` returns the
map with every pixel of a segment smaller than ``min_size`` set to 0.  All other valid pixels keep their bits;
``min_size <= 1`` removes nothing.  A pixel that is not valid on input (NaN included) comes out as 0.  ``removed`` is
(V, h, w) uint8.

Gaps
----
``fill_gaps(depths, max_gap=7, rel_jump=0.01, depth_min=1e-3, depth_max=1e5, return_filled=False)``, ``0 <= max_gap <= 32``,
treats each pixel ``(x, y)`` of the input that is not valid as follows.  The horizontal candidate exists iff there is a
nearest valid pixel ``xl < x`` and a nearest valid pixel ``xr > x`` in the same row, ``xr - xl - 1 <= max_gap``, and the
ends agree at the gap's length: ``|dl - dr| <= (rel_jump * float(xr - xl)) * min(dl, dr)``.  Its value is
``dl + (float(x - xl) / float(xr - xl)) * (dr - dl)``.  The vertical candidate is the same along the column.  The output is
the mean ``0.5f * (dh + dv)`` if both candidates exist, the single one if one exists, and 0 if neither does.  A gap that
touches the map's border has no outer end and is not filled.  Valid pixels keep their bits.  The kernel reads only its
input, so fills do not cascade.  ``filled`` is (V, h, w) uint8.

Chain
-----
``clean_depth_maps(depths, min_size=100, max_gap=7, rel_jump=0.01, depth_min=1e-3, depth_max=1e5)`` runs speckles and then
gaps: a removed speckle inside a surface is then interpolated over, as in OpenMVS.  It returns ``(depths, report)``;
``report`` holds ``valid_in``, ``segments``, ``removed_segments``, ``removed_pixels``, ``filled_pixels`` and ``valid_out``
as Python ints, and the segmentation's ``last_segment_stats()``: ``rounds``, ``border_edges_per_view`` and
``border_unions``.  ``rounds`` and ``border_unions`` are diagnostics of the run, not results: how many border edges meet two
different roots, rather than two pieces that another edge has joined a moment before, depends on the order in which the
merge launch's threads run.  Every other entry, like every tensor, is a pure function of the input.  ``min_size <= 1`` or
``max_gap == 0`` skips that step; ``segments`` and ``removed_*`` are what the speckle step saw, 0 when it was skipped.

Out of scope
------------
8-connectivity; image-guided inpainting of large holes; cleaning of the probability maps.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_COUNT = 2 ** 31 - 1                        # PF_DEPTH_SEGMENTS_MAX of include/pointflow_hip.h
MAX_GAP = 32                                   # PF_DEPTH_GAP_MAX
_FLAGS = 32                                    # round counters per allocation, re-zeroed when used up

_tile = None
_last_stats = {"rounds": 0, "border_edges_per_view": 0, "border_unions": 0}


def tile_size():
    """``(TILE_W, TILE_H)``, the tile of the library's tile kernel (``pf_depth_tile_size``)."""
    global _tile
    if _tile is None:
        tw, th = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().pf_depth_tile_size(ctypes.byref(tw), ctypes.byref(th)), "pf_depth_tile_size")
        _tile = (int(tw.value), int(th.value))
    return _tile


def __getattr__(name):                         # TILE_W, TILE_H: read from the library when first asked for
    if name == "TILE_W":
        return tile_size()[0]
    if name == "TILE_H":
        return tile_size()[1]
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def last_segment_stats():
    """``rounds`` (merge launch, compress launch, one counter read), ``border_edges_per_view`` and ``border_unions`` (the
    border edges that found two different roots, over all rounds) of the latest segmentation."""
    return dict(_last_stats)


def _check(who, depths, rel_jump, depth_min, depth_max):
    """``(V, h, w, rel_jump, depth_min, depth_max)`` from the checks that need no device."""
    if not isinstance(depths, torch.Tensor) or depths.dim() != 3:
        raise ValueError("%s: depths must be a (V, h, w) tensor" % who)
    if depths.dtype != torch.float32:
        raise ValueError("%s: depths must be float32" % who)
    V, h, w = (int(s) for s in depths.shape)
    if V * h * w > MAX_COUNT:
        raise ValueError("%s: V * h * w must be below 2^31" % who)
    rel_jump, depth_min, depth_max = float(rel_jump), float(depth_min), float(depth_max)
    if not 0.0 <= rel_jump <= 0.5:
        raise ValueError("%s: rel_jump must be in [0, 0.5]" % who)
    if not 0.0 <= depth_min < depth_max:
        raise ValueError("%s: 0 <= depth_min < depth_max" % who)
    return V, h, w, rel_jump, depth_min, depth_max


def _int(who, name, value, lo, hi=None):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError("%s: %s must be an integer" % (who, name))
    if value < lo or (hi is not None and value > hi):
        raise ValueError("%s: %s must be %s" % (who, name, ("in [%d, %d]" % (lo, hi)) if hi is not None else "at least %d" % lo))
    return int(value)


def check_clean_settings(who, min_size=100, max_gap=7, rel_jump=0.01, depth_min=1e-3, depth_max=1e5):
    """The settings of ``clean_depth_maps`` checked without a device (``ScanAccumulator`` calls this when it is built)."""
    _int(who, "min_size", min_size, 0)
    _int(who, "max_gap", max_gap, 0, MAX_GAP)
    if not 0.0 <= float(rel_jump) <= 0.5:
        raise ValueError("%s: rel_jump must be in [0, 0.5]" % who)
    if not 0.0 <= float(depth_min) < float(depth_max):
        raise ValueError("%s: 0 <= depth_min < depth_max" % who)


def _segments(depths, V, h, w, rel_jump, depth_min, depth_max, with_piece):
    """``(label (V, h, w) int32, piece or None)`` of contiguous depths on the current device, after the merge rounds."""
    global _last_stats
    dev, n = depths.device, V * h * w
    label = torch.empty((V, h, w), dtype=torch.int32, device=dev)
    piece = torch.empty((V, h, w), dtype=torch.int32, device=dev) if with_piece else None
    stats = {"rounds": 0, "border_edges_per_view": 0, "border_unions": 0}
    if n:
        tw, th = tile_size()
        # per pixel: its depth in, its label (and its piece count) out
        _lib.call("pf_depth_tile_segments_f32", _lib.ptr(depths), V, h, w, rel_jump, depth_min, depth_max, _lib.ptr(label),
                  _lib.ptr(piece), _lib.stream(), algo_bytes=n * (12 if with_piece else 8))
        edges = ((w - 1) // tw) * h + ((h - 1) // th) * w
        stats["border_edges_per_view"] = edges
        rounds, flags = 0, None
        while edges:
            if rounds % _FLAGS == 0:
                flags = torch.zeros((_FLAGS,), dtype=torch.int32, device=dev)
            flag = flags[rounds % _FLAGS:]
            # per border edge two depths and, on a compressed forest, two label loads per end
            _lib.call("pf_depth_border_merge_f32", _lib.ptr(depths), V, h, w, rel_jump, depth_min, depth_max,
                      _lib.ptr(label), _lib.ptr(flag), _lib.stream(), algo_bytes=V * edges * 24)
            rounds += 1
            united = int(flag[0])                                  # the round's one host read
            stats["border_unions"] += united
            if not united:                                         # a clean merge stored nothing: the labels are still the
                break                                              # roots that the tile kernel or the last compress left
            _lib.call("pf_depth_label_compress", _lib.ptr(label), n, _lib.stream(), algo_bytes=n * 12)
            if rounds > V * edges + 1:                             # every changed round joins two trees
                raise RuntimeError("depth_segments: %d rounds on %d border edges" % (rounds, V * edges))
        stats["rounds"] = rounds
    _last_stats = stats
    return label, piece


def _sizes(label, piece):
    """``size`` (n,) int32: at a segment's root its number of pixels."""
    n = label.numel()
    size = torch.zeros((n,), dtype=torch.int32, device=label.device)
    if n:
        _lib.call("pf_depth_segment_sizes", _lib.ptr(label), _lib.ptr(piece), n, _lib.ptr(size), _lib.stream(),
                  algo_bytes=n * 8)
    return size


def _mask(depths, label, size, min_size, depth_min, depth_max, sizes=None, out=None, removed=None):
    n = label.numel()
    if n:
        nbytes = 8 + (4 if sizes is not None else 0) + (8 if out is not None or removed is not None else 0)
        _lib.call("pf_depth_speckle_mask_f32", _lib.ptr(depths), _lib.ptr(label), _lib.ptr(size), n, min_size, depth_min,
                  depth_max, _lib.ptr(sizes), _lib.ptr(out), _lib.ptr(removed), _lib.stream(), algo_bytes=n * nbytes)


def depth_segments(depths, rel_jump=0.01, depth_min=1e-3, depth_max=1e5, return_sizes=False):
    """The segments of the module docstring: ``labels`` (V, h, w) int32 on the device of ``depths`` (V, h, w) float32, and
    with ``return_sizes`` also ``sizes`` (V, h, w) int32.  Synchronises with the host once per round."""
    who = "depth_segments"
    V, h, w, rel_jump, depth_min, depth_max = _check(who, depths, rel_jump, depth_min, depth_max)
    _lib.require_gpu(depths)
    depths = depths.contiguous()
    with _lib.on_device(depths.device):
        label, piece = _segments(depths, V, h, w, rel_jump, depth_min, depth_max, bool(return_sizes))
        if not return_sizes:
            return label
        sizes = torch.empty((V, h, w), dtype=torch.int32, device=depths.device)
        _mask(None, label, _sizes(label, piece), 0, depth_min, depth_max, sizes=sizes)
    return label, sizes


def _remove(depths, V, h, w, min_size, rel_jump, depth_min, depth_max, want_removed):
    """``(out, removed or None, label, size)`` of contiguous depths; ``label`` and ``size`` are None when nothing can be
    removed (``min_size <= 1``): the map then only loses the pixels that are not valid."""
    dev = depths.device
    out = torch.empty((V, h, w), dtype=torch.float32, device=dev)
    removed = torch.zeros((V, h, w), dtype=torch.uint8, device=dev) if want_removed else None
    if min_size <= 1:
        # no segment is smaller than one pixel: a zero-gap fill is exactly "valid pixels keep their bits, the others are 0"
        if V * h * w:
            _lib.call("pf_depth_gap_fill_f32", _lib.ptr(depths), V, h, w, 0, rel_jump, depth_min, depth_max, _lib.ptr(out),
                      None, _lib.stream(), algo_bytes=V * h * w * 8)
        return out, removed, None, None
    label, piece = _segments(depths, V, h, w, rel_jump, depth_min, depth_max, True)
    size = _sizes(label, piece)
    _mask(depths, label, size, min_size, depth_min, depth_max, out=out, removed=removed)
    return out, removed, label, size


def remove_speckles(depths, min_size=100, rel_jump=0.01, depth_min=1e-3, depth_max=1e5, return_removed=False):
    """The speckle removal of the module docstring: (V, h, w) float32, and with ``return_removed`` also ``removed``
    (V, h, w) uint8."""
    who = "remove_speckles"
    V, h, w, rel_jump, depth_min, depth_max = _check(who, depths, rel_jump, depth_min, depth_max)
    min_size = _int(who, "min_size", min_size, 0)
    _lib.require_gpu(depths)
    depths = depths.contiguous()
    with _lib.on_device(depths.device):
        out, removed = _remove(depths, V, h, w, min(min_size, MAX_COUNT), rel_jump, depth_min, depth_max,
                               bool(return_removed))[:2]
    return (out, removed) if return_removed else out


def _fill(depths, V, h, w, max_gap, rel_jump, depth_min, depth_max, want_filled):
    dev = depths.device
    out = torch.empty((V, h, w), dtype=torch.float32, device=dev)
    filled = torch.empty((V, h, w), dtype=torch.uint8, device=dev) if want_filled else None
    if V * h * w:
        # per pixel: its depth in and out, and for a hole the walks along its row and column
        _lib.call("pf_depth_gap_fill_f32", _lib.ptr(depths), V, h, w, max_gap, rel_jump, depth_min, depth_max,
                  _lib.ptr(out), _lib.ptr(filled), _lib.stream(), algo_bytes=V * h * w * (9 if want_filled else 8),
                  tag="gap %d" % max_gap)
    return out, filled


def fill_gaps(depths, max_gap=7, rel_jump=0.01, depth_min=1e-3, depth_max=1e5, return_filled=False):
    """The gap filling of the module docstring: (V, h, w) float32, and with ``return_filled`` also ``filled`` (V, h, w)
    uint8."""
    who = "fill_gaps"
    V, h, w, rel_jump, depth_min, depth_max = _check(who, depths, rel_jump, depth_min, depth_max)
    max_gap = _int(who, "max_gap", max_gap, 0, MAX_GAP)
    _lib.require_gpu(depths)
    depths = depths.contiguous()
    with _lib.on_device(depths.device):
        out, filled = _fill(depths, V, h, w, max_gap, rel_jump, depth_min, depth_max, bool(return_filled))
    return (out, filled) if return_filled else out


def clean_depth_maps(depths, min_size=100, max_gap=7, rel_jump=0.01, depth_min=1e-3, depth_max=1e5):
    """Speckles, then gaps (module docstring): ``(depths (V, h, w) float32, report)``.  One more host synchronisation than
    the segmentation's rounds: the report's counts are read together."""
    who = "clean_depth_maps"
    V, h, w, rel_jump, depth_min, depth_max = _check(who, depths, rel_jump, depth_min, depth_max)
    check_clean_settings(who, min_size, max_gap, rel_jump, depth_min, depth_max)
    min_size, max_gap = min(int(min_size), MAX_COUNT), int(max_gap)
    _lib.require_gpu(depths)
    depths = depths.contiguous()
    dev = depths.device
    with _lib.on_device(dev):
        def count(mask):
            return mask.sum(dtype=torch.int64)

        def valid(t):
            return (t > depth_min) & (t < depth_max)

        zero = torch.zeros((), dtype=torch.int64, device=dev)
        counts = {"valid_in": count(valid(depths)), "segments": zero, "removed_segments": zero, "removed_pixels": zero,
                  "filled_pixels": zero}
        stats = {"rounds": 0, "border_edges_per_view": 0, "border_unions": 0}
        out = depths
        if min_size > 1:
            out, removed, label, size = _remove(depths, V, h, w, min_size, rel_jump, depth_min, depth_max, True)
            stats = last_segment_stats()
            roots = label.view(-1) == torch.arange(V * h * w, dtype=torch.int32, device=dev)
            counts["segments"] = count(roots)
            counts["removed_segments"] = count(roots & (size < min_size))
            counts["removed_pixels"] = count(removed)
        if max_gap > 0:
            out, filled = _fill(out, V, h, w, max_gap, rel_jump, depth_min, depth_max, True)
            counts["filled_pixels"] = count(filled)
        elif out is depths:
            out = _remove(depths, V, h, w, 0, rel_jump, depth_min, depth_max, False)[0]
        counts["valid_out"] = count(valid(out))
        names = sorted(counts)
        values = torch.stack([counts[k] for k in names]).tolist()            # the report's one host read
    report = dict(zip(names, (int(v) for v in values)))
    report.update(stats)
    return out, report
