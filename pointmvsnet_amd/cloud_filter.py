"""Clean a fused point cloud on the GPU: voxel-grid merge, radius and statistical outlier removal.

The fusers (``fusion.py``, ``geometric.py``) emit a surface patch once per view that sees it and pass every isolated
"floater" that survives their per-pixel test.  This module states the usual remedies and runs them as HIP kernels
(csrc/cloud_filter.hip) on the sorted sparse grid of ``evaluation.py`` (csrc/pf_cloud_grid.h).  **The specification below is
this project's own**; parity with PCL or Open3D is neither claimed nor tested.

Common rules.  Inputs are float32 ``(N, 3)`` tensors on the GPU; non-finite coordinates are a ``ValueError``; there is no CPU
path.  All arithmetic is float32 as written unless float64 is stated.  ``d2(i, j) = (dx*dx + dy*dy) + dz*dz``.  The
neighbours of point ``i`` are the points ``j != i`` BY INDEX: an exact duplicate is a neighbour at distance 0.

1. ``knn_mean_distances(points, max_radius, k)``: ``R = float32(max_radius)``, ``R2 = R * R`` in float32, ``1 <= k <= 32``.
   For point ``i`` take the multiset ``{d2(i, j) : j != i, d2(i, j) < R2}``; ``c_i = min(k, its size)``; with
   ``a_1 <= a_2 <= ..`` its ``c_i`` smallest values, ``s = ((sqrtf(a_1) + sqrtf(a_2)) + ...)`` and
   ``m_i = (s + float32(k - c_i) * R) / float32(k)``: a missing neighbour counts as one at distance ``R``.  The multiset of
   the ``c_i`` smallest values is unique even among ties and the order of the sum is fixed, so ``m`` is a pure function of
   the input: a permuted cloud gives the permuted ``m`` bit for bit, and so does any search grid.  ``m_i`` is continuous
   across the radius (a neighbour just inside contributes about ``R``, as a missing one does); only ``c_i`` jumps there.
   A point with no neighbour inside the radius has ``m_i = R`` exactly (``(float32(k) * R) / float32(k)`` is ``R`` only up
   to rounding for some ``k``).  ``N == 0`` gives empty outputs; ``N == 1`` gives ``m = R`` and ``c = 0``.
2. ``statistical_outlier_mask``: ``mu`` the float64 mean of ``m``, ``sigma`` its float64 population standard deviation
   (torch ``double`` reductions), ``thr = float32(mu + std_ratio * sigma)``; a point is KEPT iff ``m_i <= thr``.
3. ``radius_outlier_mask(points, radius, min_neighbors)``: kept iff at least ``min_neighbors`` other points have
   ``d2 < R2``, ``1 <= min_neighbors <= 32`` (the kernel stops a point once it has found that many).
4. ``voxel_downsample(points, voxel)``: ``o`` the per-axis minimum of the cloud (float32), ``inv = float32(1) /
   float32(voxel)`` computed ON THE HOST, cell ``c = floorf((p - o) * inv)`` per axis -- a multiplication by a host-made
   reciprocal, so that the assignment does not rest on the device's division and a float32 NumPy statement reproduces it
   exactly.  More than 2^17 cells on an axis is a ``ValueError`` (a widened cell would change the result, unlike in the
   search grids).  One output row per occupied voxel in ascending ``(cx, cy, cz)`` order.  Position: the float64 sum of the
   members in ascending input index, divided by the count, rounded to float32.  Colour (uint8 per channel):
   ``(2 * sum + count) // (2 * count)`` in integers.  Normal: the float64 sum of the members' normals, normalised in
   float64 and rounded to float32; ``(0, 0, 0)`` when the sum's length is 0.  ``inverse`` (int64, N) is the output row of
   each input point, ``counts`` (int32) the members per row.
5. ``clean_cloud``: the voxel merge (if ``voxel`` is not None), then the radius test (if ``min_neighbors``, at ``max_radius``),
   then the statistical test (if ``std_ratio`` and ``max_radius`` are not None); each step runs on the output of the one before.

Limits: those of ``evaluation.py`` (2 * 10^9 points; a search grid of more than 2^17 cells per axis gets wider cells:
slower, same result).
"""
import numpy as np
import torch

from . import _lib
from .evaluation import MAX_CELLS, _check_points, _Grid

MAX_K = 32                   # PF_CLOUD_MAX_K of include/pointflow_hip.h
CELLS_PER_RADIUS = 2         # the search grid's cells to the radius (1: the 27 cells around a point hold the radius); the
                             # fastest of 1, 2, 3, 4 at k = 8, 16 and 32 (profiles/cloud_filter_microbench.jsonl)


def _check_cloud(points, who):
    """``evaluation._check_points`` without the device check: the arguments are judged first (a ``ValueError`` needs no
    GPU), then ``_lib.require_gpu`` refuses a CPU tensor."""
    return _check_points(points, who, gpu=False)


def _radius(value, who, what):
    try:
        ok = float(value) > 0.0 and np.isfinite(np.float32(value))
    except (TypeError, ValueError):
        ok = False
    if not ok or not float(np.float32(value)) * float(np.float32(value)) > 0.0:
        raise ValueError("%s: %s must be positive and finite" % (who, what))
    return np.float32(value)


def _count_arg(value, who, what):
    if isinstance(value, bool) or int(value) != value or not 1 <= int(value) <= MAX_K:
        raise ValueError("%s: %s must be an integer in 1 .. %d" % (who, what, MAX_K))
    return int(value)


def _search_grid(points, R, cells=CELLS_PER_RADIUS):
    """The sorted grid with ``cells`` cells to the radius: the cube of that many rings covers ``R`` with the 0.05-cell margin
    of csrc/pf_cloud_grid.h (a cloud of more than 2^17 such cells per axis gets wider ones: fewer rings, same result)."""
    return _Grid(points, float(R) / (cells - 0.05) * (1.0 + 1e-4), hashed=False)


def _knn_stats(grid, R, k, mean, count):
    _lib.call("pf_cloud_knn_stats_f32", _lib.ptr(grid.packed), _lib.ptr(grid.keys), grid.n, *(grid.cells + [
        grid.edge, k, float(R), float(R * R), _lib.ptr(mean), _lib.ptr(count), _lib.stream()]))


def knn_mean_distances(points, max_radius, k=16, return_count=False):
    """float32 (N,): per point the mean distance ``m`` to its ``k`` nearest other points inside ``max_radius``, a missing
    neighbour counted at ``max_radius`` (module docstring, 1.); with ``return_count`` also ``c``, int32 (N,)."""
    points = _check_cloud(points, "knn_mean_distances")
    R = _radius(max_radius, "knn_mean_distances", "max_radius")
    k = _count_arg(k, "knn_mean_distances", "k")
    _lib.require_gpu(points)
    n, dev = int(points.shape[0]), points.device
    with _lib.on_device(dev):
        mean = torch.empty((n,), dtype=torch.float32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        if n:
            _knn_stats(_search_grid(points, R), R, k, mean, count)
    return (mean, count) if return_count else mean


def statistical_outlier_mask(points, max_radius, k=16, std_ratio=2.0, return_distances=False):
    """bool (N,): kept iff ``m_i <= float32(mean(m) + std_ratio * std(m))`` (module docstring, 2.); with
    ``return_distances`` also ``m``."""
    if not np.isfinite(float(std_ratio)):
        raise ValueError("statistical_outlier_mask: std_ratio must be finite")
    m = knn_mean_distances(points, max_radius, k)
    if m.numel() == 0:
        keep = torch.zeros((0,), dtype=torch.bool, device=m.device)
    else:
        m64 = m.double()                                                   # plumbing: the two reductions
        mu, sigma = float(m64.mean()), float(m64.std(unbiased=False))
        keep = m <= float(np.float32(mu + float(std_ratio) * sigma))
    return (keep, m) if return_distances else keep


def radius_outlier_mask(points, radius, min_neighbors):
    """bool (N,): kept iff at least ``min_neighbors`` other points lie inside ``radius`` (module docstring, 3.)."""
    points = _check_cloud(points, "radius_outlier_mask")
    R = _radius(radius, "radius_outlier_mask", "radius")
    limit = _count_arg(min_neighbors, "radius_outlier_mask", "min_neighbors")
    _lib.require_gpu(points)
    n, dev = int(points.shape[0]), points.device
    with _lib.on_device(dev):
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        if n:
            grid = _search_grid(points, R)
            _lib.call("pf_cloud_radius_count_f32", _lib.ptr(grid.packed), _lib.ptr(grid.keys), n, *(grid.cells + [
                grid.edge, limit, float(R), float(R * R), _lib.ptr(count), _lib.stream()]))
    return count >= limit


def _check_attribute(t, n, dev, dtype, who, what):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a torch tensor" % (who, what))
    if t.dim() != 2 or tuple(t.shape) != (n, 3) or t.dtype != dtype or t.device != dev:
        raise ValueError("%s: %s must be (%d, 3) %s on the points' device" % (who, what, n, str(dtype).replace("torch.", "")))
    return t.contiguous()


def voxel_downsample(points, voxel, colors=None, normals=None, return_inverse=False, return_counts=False):
    """One point per occupied voxel of edge ``voxel`` (module docstring, 4.): ``(points (M, 3) float32, colors (M, 3) uint8 or
    None, normals (M, 3) float32 or None)``, followed by ``inverse`` (N,) int64 with ``return_inverse`` and ``counts`` (M,)
    int32 with ``return_counts``."""
    who = "voxel_downsample"
    points = _check_cloud(points, who)
    n, dev = int(points.shape[0]), points.device
    colors = _check_attribute(colors, n, dev, torch.uint8, who, "colors")
    normals = _check_attribute(normals, n, dev, torch.float32, who, "normals")
    inv = _voxel_inverse(voxel, who, "voxel")
    if n:
        lo, cells = _voxel_cells(points, inv, who)
    _lib.require_gpu(points)
    with _lib.on_device(dev):
        if n == 0:
            out = (points, colors, normals)
            inverse = torch.zeros((0,), dtype=torch.int64, device=dev)
            counts = torch.zeros((0,), dtype=torch.int32, device=dev)
        else:
            out_points, out_colors, out_normals, counts, inverse, _ = _voxel_reduce(points, lo, inv, cells, colors, normals,
                                                                                    return_inverse)
            out = (out_points, out_colors, out_normals)
    return out + ((inverse,) if return_inverse else ()) + ((counts,) if return_counts else ())


def _voxel_inverse(voxel, who, what):
    """``float32(1) / float32(voxel)``, made on the host (module docstring, 4.)."""
    inv = np.float32(1.0) / _radius(voxel, who, what)
    if not (np.isfinite(inv) and inv > 0.0):
        raise ValueError("%s: %s is too small" % (who, what))
    return inv


def _voxel_cells(points, inv, who, origin=None):
    """``(o, cells per axis)`` of a non-empty cloud: ``o`` its per-axis float32 minimum, or ``origin`` (float32 (3,), which must
    be ``<=`` that minimum on every axis); more than 2^17 cells on an axis is a ``ValueError``.  Two host reads."""
    lo = points.amin(dim=0).cpu().numpy()                                  # plumbing: the bounding box, float32
    hi = points.amax(dim=0).cpu().numpy()
    if origin is not None:
        if not (origin <= lo).all():
            raise ValueError("%s: origin must be <= the smallest coordinate on every axis" % who)
        lo = origin
    top = np.floor((hi - lo) * inv)                                        # float32, monotone in p: the largest cell
    if not np.isfinite(top).all() or float(top.max()) >= MAX_CELLS:
        raise ValueError("%s: more than %d voxels on an axis" % (who, MAX_CELLS))
    return lo, [int(t) + 1 for t in top]


def _voxel_reduce(points, lo, inv, cells, colors, normals, want_inverse):
    """The two kernels of the voxel merge on a non-empty cloud, on the current device: ``(points (M, 3), colors, normals,
    counts (M,) int32, inverse (N,) int64 or None, (sorted keys (N,), segment starts (M + 1,)))``; rows come in ascending key.
    ``mesh_simplify`` clusters a mesh's vertices with it."""
    n, dev = int(points.shape[0]), points.device
    keys = torch.empty((n,), dtype=torch.int64, device=dev)
    _lib.call("pf_cloud_voxel_keys_f32", _lib.ptr(points), n, *([float(v) for v in lo] + [float(inv)] + cells + [
        _lib.ptr(keys), _lib.stream()]))
    keys, order = torch.sort(keys, stable=True)                            # plumbing; stable: ascending index inside a voxel
    first = torch.ones((n,), dtype=torch.bool, device=dev)
    first[1:] = keys[1:] != keys[:-1]
    starts = torch.nonzero(first).view(-1)                                 # plumbing: the segment starts
    m = int(starts.numel())
    starts = torch.cat([starts, torch.full((1,), n, dtype=torch.int64, device=dev)])
    out_points = torch.empty((m, 3), dtype=torch.float32, device=dev)
    out_colors = None if colors is None else torch.empty((m, 3), dtype=torch.uint8, device=dev)
    out_normals = None if normals is None else torch.empty((m, 3), dtype=torch.float32, device=dev)
    counts = torch.empty((m,), dtype=torch.int32, device=dev)
    inverse = torch.empty((n,), dtype=torch.int64, device=dev) if want_inverse else None
    _lib.call("pf_cloud_voxel_reduce_f32", _lib.ptr(points), _lib.ptr(colors), _lib.ptr(normals), _lib.ptr(order),
              _lib.ptr(starts), n, m, _lib.ptr(out_points), _lib.ptr(out_colors), _lib.ptr(out_normals),
              _lib.ptr(counts), _lib.ptr(inverse), _lib.stream())
    return out_points, out_colors, out_normals, counts, inverse, (keys, starts)


def _select(keep, points, colors, normals):
    idx = torch.nonzero(keep).view(-1)
    return points[idx], None if colors is None else colors[idx], None if normals is None else normals[idx]


def clean_cloud(points, colors=None, normals=None, voxel=None, max_radius=None, k=16, std_ratio=2.0, min_neighbors=None):
    """``(points, colors, normals, report)`` after the voxel merge (if ``voxel`` is not None), the radius test (if ``min_neighbors``, at
    ``max_radius``) and the statistical test (if ``std_ratio`` and ``max_radius`` are not None), each on the output of the one
    before (module docstring, 5.).  ``report``: the point counts ``input``, after each step that ran (``voxel``, ``radius``,
    ``statistical``) and ``output``."""
    who = "clean_cloud"
    points = _check_cloud(points, who)
    n, dev = int(points.shape[0]), points.device
    colors = _check_attribute(colors, n, dev, torch.uint8, who, "colors")
    normals = _check_attribute(normals, n, dev, torch.float32, who, "normals")
    if min_neighbors is not None and max_radius is None:
        raise ValueError("%s: min_neighbors needs max_radius" % who)
    if voxel is not None:
        _radius(voxel, who, "voxel")
    if max_radius is not None:
        _radius(max_radius, who, "max_radius")
        _count_arg(k, who, "k")
    if min_neighbors is not None:
        _count_arg(min_neighbors, who, "min_neighbors")
    _lib.require_gpu(points)
    report = {"input": n}
    if voxel is not None:
        points, colors, normals = voxel_downsample(points, voxel, colors, normals)
        report["voxel"] = int(points.shape[0])
    if min_neighbors is not None:
        points, colors, normals = _select(radius_outlier_mask(points, max_radius, min_neighbors), points, colors, normals)
        report["radius"] = int(points.shape[0])
    if std_ratio is not None and max_radius is not None:
        points, colors, normals = _select(statistical_outlier_mask(points, max_radius, k, std_ratio), points, colors, normals)
        report["statistical"] = int(points.shape[0])
    report["output"] = int(points.shape[0])
    return points, colors, normals, report
