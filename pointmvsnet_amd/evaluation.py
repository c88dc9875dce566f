"""Score a reconstructed point cloud against a scan's ground-truth cloud on the GPU: DTU accuracy and completeness.

The reference has no such step: DTU's evaluation is a separate MATLAB program (``PointCompareMain.m`` / ``ComputeStat.m``).
This module states the step itself and runs it as HIP kernels (csrc/cloud_eval.hip).  **The specification below is this
project's own**: it is modelled on that program and uses its parameters and defaults (``min_dist = 0.2``, ``max_dist = 20``,
observability mask, ground plane); bit parity with the MATLAB program is neither claimed nor tested.  Departures:

* the thinning walks the points in a STATED pseudo-random order (``prio`` below) where MATLAB draws a random permutation, so
  the result is a pure function of the input;
* all arithmetic is float32 as written below (MATLAB works in double); sums of distances are float64;
* the median is ``torch.median``'s: the LOWER middle value of an even count;
* a distance equal to ``max_dist`` counts as "no neighbour" and is left out of the scores.

Inputs are float32 ``(N, 3)`` tensors on the GPU; non-finite coordinates are a ``ValueError``; there is no CPU path.

1. ``thin_points``: ``prio(i)``, with ``x = uint32(i)``: ``x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
   x ^= x >> 16`` (a bijection on 32 bits); ``key(i) = (prio(i) << 32) | i``, the lower key goes first.  ``near(i, j)`` iff
   ``dx*dx + dy*dy + dz*dz < t`` in float32, summed in that order, ``t = float32(min_dist) * float32(min_dist)``.  Point ``i``
   is KEPT iff no kept ``j`` with ``key(j) < key(i)`` has ``near(i, j)`` -- the sequential greedy walk in key order.  The kept
   points are returned in input order.  (The kernels run the parallel form: per round an undecided point is removed if a
   lower-key near neighbour is kept, kept if all of them are removed.  ``last_thinning_rounds()`` tells how many rounds.)
2. ``nearest_distances``: ``d = min(sqrt(min_j (dx*dx + dy*dy + dz*dz)), float32(max_dist))`` per query; ``max_dist`` for
   a query with no target that near or an empty target.  The index is that of A target point attaining the distance,
   ``-1`` where ``d == max_dist``.
3. ``in_obs_mask``: ``idx = floor((p - bb_min) / res + 0.5)`` per axis in float32; inside iff ``idx`` lies in the ``(X, Y, Z)``
   grid and ``mask[idx]`` is set.  ``above_plane``: ``((a x + b y) + c z) + d > 0``.
4. ``evaluate_point_cloud``: see its docstring.

Limits: at most 2 * 10^9 points per cloud (the specification allows 2^32); the search grids have at most 2^17 cells per axis
-- a cloud whose extent is larger gets wider cells (slower, same result).
"""
import numpy as np
import torch

from . import _lib

MAX_CELLS = 1 << 17          # PF_CLOUD_MAX_CELLS of include/pointflow_hip.h
MAX_POINTS = 2000000000      # PF_CLOUD_MAX_POINTS
MARGIN = 1.05                # cell edge / search radius: covers the float32 rounding of the cell coordinates (pf_cloud_grid.h)
FINE_CELLS_PER_MAX_DIST = 40  # the fine search grid: max_dist / 40 = 0.5 at DTU's 20
FINE_RINGS = 3               # the first pass walks the cubes of radius 1 and 3 cells

_last_rounds = 0
_last_unfinished = 0


def last_thinning_rounds():
    """Rounds the last ``thin_points`` call took (tools/microbench_evaluation.py reports it)."""
    return _last_rounds


def last_unfinished_queries():
    """Queries the last ``nearest_distances`` call handed to the one-wave-per-query pass."""
    return _last_unfinished


def _check_points(points, what, gpu=True):
    """The rules for a cloud.  ``gpu=False`` leaves the device check to the caller (cloud_filter.py judges its other
    arguments first, so that their ``ValueError`` needs no GPU)."""
    if not isinstance(points, torch.Tensor):
        raise TypeError("%s: expected a torch tensor" % what)
    if gpu:
        _lib.require_gpu(points)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("%s: points must be (N, 3) float32" % what)
    if points.shape[0] > MAX_POINTS:
        raise ValueError("%s: more than %d points" % (what, MAX_POINTS))
    points = points.contiguous()
    if points.numel() and not bool(torch.isfinite(points).all()):
        raise ValueError("%s: non-finite coordinates" % what)
    return points


def _grid_frame(lo, hi, edge):
    """``(edge, origin, cells)`` of the search grid over the float64 box ``lo .. hi`` with the cell edge wanted: the edge is
    widened until the box fits into ``MAX_CELLS - 4`` cells and rounded to float32, the origin is the box's float32 corner and
    every axis gets ``floor(extent / edge) + 2`` cells (the upper corner's own cell and one of slack)."""
    edge = float(np.float32(max(float(edge), float((hi - lo).max()) / (MAX_CELLS - 4))))
    return edge, [float(v) for v in lo.astype(np.float32)], [int(np.floor(e / edge)) + 2 for e in (hi - lo)]


class _Grid(object):
    """A cloud sorted into a sparse grid of cell edge >= ``edge``: ``keys`` (sorted), ``packed`` (N, 4) records, ``order``."""

    def __init__(self, points, edge, hashed):
        n = int(points.shape[0])
        dev = points.device
        lo = points.amin(dim=0).cpu().numpy().astype(np.float64)       # plumbing: the bounding box
        hi = points.amax(dim=0).cpu().numpy().astype(np.float64)
        self.edge, self.origin, self.cells = _grid_frame(lo, hi, edge)
        self.n = n
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        _lib.call("pf_cloud_cell_keys_f32", _lib.ptr(points), n, *(self.origin + [self.edge] + self.cells +
                                                                   [_lib.ptr(keys), _lib.stream()]))
        self.keys, self.order = torch.sort(keys, stable=True)          # plumbing
        self.packed = torch.empty((n, 4), dtype=torch.int32, device=dev)
        _lib.call("pf_cloud_pack_f32", _lib.ptr(points), _lib.ptr(self.order), n, 1 if hashed else 0, _lib.ptr(self.packed),
                  _lib.stream())

    def args(self):
        return self.origin + [self.edge] + self.cells


def thin_points(points, min_dist=0.2, return_index=False):
    """The points of ``points`` (N, 3) kept by the greedy minimum-distance thinning (module docstring, 1.), in input order;
    with ``return_index`` also their int64 indices."""
    global _last_rounds
    points = _check_points(points, "thin_points")
    if not float(min_dist) > 0.0:
        raise ValueError("thin_points: min_dist must be positive")
    n = int(points.shape[0])
    dev = points.device
    _last_rounds = 0
    if n == 0:
        idx = torch.zeros((0,), dtype=torch.int64, device=dev)
        return (points, idx) if return_index else points
    with _lib.on_device(dev):
        md = np.float32(min_dist)
        t = float(md * md)                                             # float32 product
        grid = _Grid(points, float(md) * MARGIN, hashed=True)
        state = torch.zeros((n,), dtype=torch.uint8, device=dev)
        other = torch.empty_like(state)
        pending = torch.zeros((1,), dtype=torch.int32, device=dev)
        while True:
            pending.zero_()
            _lib.call("pf_cloud_thin_round", _lib.ptr(grid.packed), _lib.ptr(grid.keys), n, *(grid.cells + [
                t, _lib.ptr(state), _lib.ptr(other), _lib.ptr(pending), _lib.stream()]))
            state, other = other, state
            _last_rounds += 1
            if int(pending.item()) == 0:
                break
            if _last_rounds > n:
                raise RuntimeError("thin_points: the rounds do not settle")
        keep = torch.empty((n,), dtype=torch.bool, device=dev)
        keep[grid.order] = state == 1                                  # back to input order (plumbing)
        idx = torch.nonzero(keep).view(-1)
        kept = points[idx]
    return (kept, idx) if return_index else kept


def _two_pass_search(query, cap, make_grid, first_pass, second_pass, dist, index):
    """The search of ``nearest_distances`` and ``mesh_distance.point_mesh_distances`` into ``dist`` / ``index``:
    ``make_grid(edge)`` sorts the target into a grid; ``first_pass`` (a thread per query on the fine grid, edge ``cap / 40``)
    marks in ``done`` what it finishes; the rest goes to ``second_pass`` (a wave per query) on the coarse grid of edge
    ``1.05 cap``, built only when needed.  Returns ``(fine, coarse or None, number of second-pass queries)``."""
    fine = make_grid(cap / FINE_CELLS_PER_MAX_DIST)
    coarse, unfinished = None, 0
    if fine.keys.numel():                                              # no record (no face has a surface): nothing to find
        done = torch.empty((int(query.shape[0]),), dtype=torch.uint8, device=query.device)
        first_pass(query, fine, cap, dist, index, done)
        todo = torch.nonzero(done == 0).view(-1)                       # plumbing: the list of unfinished queries
        unfinished = int(todo.numel())
        if unfinished:
            coarse = make_grid(cap * MARGIN)
            second_pass(query, todo, coarse, cap, dist, index)
    return fine, coarse, unfinished


def _first_pass(query, grid, cap, dist, index, done):
    _lib.call("pf_cloud_nn_cells_f32", _lib.ptr(query), int(query.shape[0]), _lib.ptr(grid.packed), _lib.ptr(grid.keys), grid.n,
              *(grid.args() + [FINE_RINGS, cap, _lib.ptr(dist), _lib.ptr(index), _lib.ptr(done), _lib.stream()]))


def _second_pass(query, todo, grid, cap, dist, index):
    _lib.call("pf_cloud_nn_wave_f32", _lib.ptr(query), _lib.ptr(todo), int(todo.numel()), int(query.shape[0]),
              _lib.ptr(grid.packed), _lib.ptr(grid.keys), grid.n,
              *(grid.args() + [cap, _lib.ptr(dist), _lib.ptr(index), _lib.stream()]))


def nearest_distances(query, target, max_dist=20.0, return_index=False):
    """Per point of ``query`` (Nq, 3) its distance to the nearest point of ``target`` (Nt, 3), capped at ``max_dist`` (module
    docstring, 2.): float32 (Nq,); with ``return_index`` also the int64 index of that target point (-1 at the cap)."""
    global _last_unfinished
    query = _check_points(query, "nearest_distances")
    target = _check_points(target, "nearest_distances")
    if query.device != target.device:
        raise ValueError("nearest_distances: the clouds are on different devices")
    if not float(max_dist) > 0.0:
        raise ValueError("nearest_distances: max_dist must be positive")
    nq, nt = int(query.shape[0]), int(target.shape[0])
    dev = query.device
    cap = float(np.float32(max_dist))
    _last_unfinished = 0
    with _lib.on_device(dev):
        dist = torch.full((nq,), cap, dtype=torch.float32, device=dev)
        index = torch.full((nq,), -1, dtype=torch.int32, device=dev)
        if nq and nt:
            _last_unfinished = _two_pass_search(query, cap, lambda edge: _Grid(target, edge, hashed=False), _first_pass,
                                                _second_pass, dist, index)[2]
    return (dist, index.long()) if return_index else dist


def in_obs_mask(points, mask, bb_min, res):
    """bool (N,): the point's voxel ``floor((p - bb_min) / res + 0.5)`` lies in the bool ``(X, Y, Z)`` grid ``mask`` and is set."""
    points = _check_points(points, "in_obs_mask")
    dev = points.device
    mask = torch.as_tensor(mask)
    if mask.dim() != 3 or min(mask.shape) < 1:
        raise ValueError("in_obs_mask: mask must be a non-empty (X, Y, Z) grid")
    bb = [float(np.float32(v)) for v in np.asarray(torch.as_tensor(bb_min).cpu(), dtype=np.float64).reshape(-1)]
    if len(bb) != 3 or not float(res) > 0.0:
        raise ValueError("in_obs_mask: bb_min must have three values and res must be positive")
    with _lib.on_device(dev):
        grid = (mask != 0).to(device=dev, dtype=torch.uint8).contiguous()
        out = torch.empty((points.shape[0],), dtype=torch.uint8, device=dev)
        _lib.call("pf_cloud_obs_mask_f32", _lib.ptr(points), int(points.shape[0]), _lib.ptr(grid),
                  *([int(s) for s in grid.shape] + bb + [float(np.float32(res)), _lib.ptr(out), _lib.stream()]))
    return out.bool()


def above_plane(points, plane):
    """bool (N,): ``plane . (x, y, z, 1) > 0`` for the four floats of ``plane``."""
    points = _check_points(points, "above_plane")
    p = [float(np.float32(v)) for v in np.asarray(torch.as_tensor(plane).cpu(), dtype=np.float64).reshape(-1)]
    if len(p) != 4:
        raise ValueError("above_plane: plane must have four values")
    with _lib.on_device(points.device):
        out = torch.empty((points.shape[0],), dtype=torch.uint8, device=points.device)
        _lib.call("pf_cloud_above_plane_f32", _lib.ptr(points), int(points.shape[0]), *(p + [_lib.ptr(out), _lib.stream()]))
    return out.bool()


def _mean_median(d):
    if d.numel() == 0:
        return float("nan"), float("nan")
    return float(d.double().sum() / d.numel()), float(torch.median(d))


def _scores(d_acc, acc_points, d_comp, comp_points, cap, counts, tensors, obs_mask, bb_min, res, plane):
    """The scoring tail of every ``evaluate_*`` route, here and in mesh_distance.py.  ``d_acc`` (measured from ``acc_points``)
    is used below the cap and inside ``obs_mask``, ``d_comp`` (from ``comp_points``) below the cap and above ``plane``.  The
    dict holds the five scores, ``counts`` and the two used counts; with ``tensors`` (for ``return_distances``, else None)
    also those, the two distance tensors and the two masks."""
    acc_used = d_acc < cap
    if obs_mask is not None:
        acc_used &= in_obs_mask(acc_points, obs_mask, bb_min, res)
    comp_used = d_comp < cap
    if plane is not None:
        comp_used &= above_plane(comp_points, plane)
    acc_mean, acc_median = _mean_median(d_acc[acc_used])
    comp_mean, comp_median = _mean_median(d_comp[comp_used])
    out = {"accuracy_mean": acc_mean, "accuracy_median": acc_median, "completeness_mean": comp_mean,
           "completeness_median": comp_median, "overall": (acc_mean + comp_mean) / 2.0}
    out.update(counts)
    out.update(n_data_used=int(acc_used.sum()), n_gt_used=int(comp_used.sum()))
    if tensors is not None:
        out.update(tensors, d_acc=d_acc, d_comp=d_comp, acc_used=acc_used, comp_used=comp_used)
    return out


def _dtu_filters(obs_mask_mat, plane_mat):
    """DTU's ``ObsMask<scan>_10.mat`` / ``Plane<scan>.mat`` as the filter arguments of the ``evaluate_*`` functions."""
    from .utils import io as IO
    kw = {}
    if obs_mask_mat is not None:
        mask, bb_min, res = IO.load_dtu_obs_mask(obs_mask_mat)
        kw.update(obs_mask=mask, bb_min=bb_min, res=res)
    if plane_mat is not None:
        kw.update(plane=IO.load_dtu_plane(plane_mat))
    return kw


def evaluate_point_cloud(data, gt, min_dist=0.2, max_dist=20.0, obs_mask=None, bb_min=None, res=None, plane=None, thin=True,
                         return_distances=False):
    """DTU's scores of the reconstructed cloud ``data`` against the ground-truth cloud ``gt`` as a dict of Python numbers.

    ``data' = thin_points(data, min_dist)`` when ``thin``.  ``d_acc = nearest_distances(data', gt, max_dist)`` is used where
    ``in_obs_mask(data', obs_mask, bb_min, res)`` (everywhere without a mask) and ``d_acc < max_dist``;
    ``d_comp = nearest_distances(gt, data', max_dist)`` where ``above_plane(gt, plane)`` (everywhere without a plane) and
    ``d_comp < max_dist``.  ``accuracy_mean``, ``accuracy_median``, ``completeness_mean``, ``completeness_median`` over the
    used distances (float64 sums, the lower median), ``overall = (accuracy_mean + completeness_mean) / 2`` and the counts
    ``n_data``, ``n_data_thinned``, ``n_data_used``, ``n_gt``, ``n_gt_used``.  A score over an empty set is ``nan``.
    With ``return_distances`` the dict also holds the tensors ``data_thinned``, ``d_acc``, ``d_comp``, ``acc_used``, ``comp_used``."""
    data = _check_points(data, "evaluate_point_cloud")
    gt = _check_points(gt, "evaluate_point_cloud")
    if obs_mask is not None and (bb_min is None or res is None):
        raise ValueError("evaluate_point_cloud: obs_mask needs bb_min and res")
    cap = float(np.float32(max_dist))
    thinned = thin_points(data, min_dist) if thin else data
    d_acc = nearest_distances(thinned, gt, max_dist)
    d_comp = nearest_distances(gt, thinned, max_dist)
    return _scores(d_acc, thinned, d_comp, gt, cap,
                   {"n_data": int(data.shape[0]), "n_data_thinned": int(thinned.shape[0]), "n_gt": int(gt.shape[0])},
                   {"data_thinned": thinned} if return_distances else None, obs_mask, bb_min, res, plane)


def evaluate_ply(data_ply, gt_ply, obs_mask_mat=None, plane_mat=None, min_dist=0.2, max_dist=20.0, thin=True, device=None,
                 return_distances=False):
    """``evaluate_point_cloud`` on the vertices of two PLY files (``utils.io.load_ply_points``), with DTU's
    ``ObsMask<scan>_10.mat`` / ``Plane<scan>.mat`` when given (``utils.io.load_dtu_obs_mask`` / ``load_dtu_plane``)."""
    from .utils import io as IO
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    data = torch.from_numpy(IO.load_ply_points(data_ply)).to(dev)
    gt = torch.from_numpy(IO.load_ply_points(gt_ply)).to(dev)
    return evaluate_point_cloud(data, gt, min_dist=min_dist, max_dist=max_dist, thin=thin,
                                return_distances=return_distances, **_dtu_filters(obs_mask_mat, plane_mat))
