"""Exact point-to-triangle-mesh distances on the GPU, and the scores that use them.

``mesh_ops.sample_surface`` followed by ``evaluation.nearest_distances`` measures the distance to a *sample* of a surface: a
point that lies exactly on the mesh is still about half a pitch from the nearest sample, and at DTU's 0.2 that bias is a
large share of a 0.3 - 0.5 mm mean.  This module measures the distance to the surface itself, as five HIP kernels
(csrc/mesh_distance.hip).  **The specification below is this project's own**; parity with Open3D's ``RaycastingScene``,
trimesh, libigl or CGAL is neither claimed nor tested.  The library is built with ``-ffp-contract=off``, so the float64
arithmetic is meant as written.

``point_mesh_distances(points, vertices, faces, max_dist=20.0, return_face=False) -> dist (N,) float32 [, face (N,) int64]``

Inputs
------
``points`` (N, 3) float32 on the GPU; non-finite coordinates are a ValueError (``evaluation._check_points``).  ``vertices``
(Nv, 3) float32 and ``faces`` (Nf, 3) int32 or int64 by the rules of ``mesh_ops`` (``_check_mesh``, ``_faces32``: one range check
with torch min / max, an index outside ``[0, Nv)`` is a ValueError), ``Nf <= 2^27 - 2^13``.  All arguments are checked before a
GPU is needed.  There is no CPU path.  ``N == 0``, ``Nf == 0`` and ``Nv == 0`` work; an empty mesh gives ``max_dist`` and ``-1``
everywhere.  A face that names a non-finite vertex has no surface and is skipped.  A face may name a vertex twice, may have
no area, and may be duplicated.

The distance
------------
Per pair (query ``p``, face ``(a, b, c)``), every float32 coordinate is converted to **float64** and everything below is
float64.  Dot products are ``(x x' + y y') + z z'``.  Cross products are a product, a product and a difference per component.

* ``seg(p, u, v)``: ``e = v - u``, ``w = p - u``, ``ee = e.e``; ``t = clamp((w.e) / ee, 0, 1)`` if ``ee > 0``, else ``0``;
  ``r = w - t e``; the result is ``r.r``.
* ``d2_edges = min(seg(p, a, b), seg(p, b, c), seg(p, c, a))``.
* ``n = cross(b - a, c - a)`` and ``nn = n.n``.
* The pair is *inside* iff all four hold: ``nn > 0``; ``cross(b - a, p - a).n >= 0``; ``cross(c - b, p - b).n >= 0``;
  ``cross(a - c, p - c).n >= 0``.
* When inside, ``d2_plane = ((p - a).n)^2 / nn`` and ``d2 = min(d2_plane, d2_edges)``.  Otherwise ``d2 = d2_edges``.

So a face without area acts as its edges and a point is the face's own segment of length 0; slivers cost no accuracy, because
the differences of nearby float32 values are exact in float64.

Per query ``(d2*, f*)`` is the **lexicographic minimum of (d2, face index)** over all faces that are not skipped, and
``d = float32(sqrt(d2*))``.  If ``d >= float32(max_dist)``, or there is no face, then ``dist = float32(max_dist)`` and
``face = -1``; otherwise ``dist = d`` and ``face = f*`` (``nearest_distances``' cap rule).  The lexicographic minimum does not
depend on the order or multiplicity in which candidates are visited: the result is a pure function of the input, and two
runs give identical bytes.

Float64 is the design decision: a float32 statement would need a per-face conditioning term (``1 / sin`` of the smallest
angle) in every tolerance, and marching tetrahedra produce slivers by construction.  tools/microbench_mesh_distance.py
reports what it costs.

The search
----------
Correctness does not depend on it.  A sorted sparse grid of **(cell, face) pairs** with ``pf_cloud_grid.h``'s keys (the
structure of ``evaluation._Grid``): a face is listed in every cell of its bounding box grown by ``0.02`` cell edges in float32
(``PF_MESH_DIST_BOX_MARGIN``; csrc/mesh_distance.hip proves that a search of radius ``r`` cells meets every face nearer than
``(r - 0.05)`` edges).  The list is built by a count kernel per face, ``torch.cumsum``, an emit kernel per pair and a stable
torch sort of the keys (plumbing); a pack kernel then gathers 48-byte face records in sorted order, so that the inner loops
have no dependent index load.  The grid's box is that of the finite vertices.

* First pass: one thread per query walks the cubes of radius 1 and 3 cells (``FINE_RINGS``) around its own cell on a fine
  grid of edge ``max_dist / 40``, and stops when its best distance lies inside the cube already visited or the cube covers
  ``max_dist``.
* Second pass: the queries that did not finish are collected and handled one wave per query on a coarse grid of edge
  ``1.05 max_dist`` (27 cells), exactly as ``nearest_distances`` does; the wave-wide ``(d2, face)`` minimum goes through
  shuffles.  The coarse grid is built only when there are such queries.
* Large faces: the host reads each grid's pair total (one synchronisation, needed anyway to allocate).  While the total
  exceeds the **budget of ``16 Nf + 2^16`` pairs** the cell edge is doubled and the faces are counted again; a grid of two
  cells per axis has at most 8 pairs per face, so this ends.  Such meshes -- two triangles over the whole scene -- are
  correct and slower.
* ``last_grid_report()`` tells the edges, the pair counts and the number of second-pass queries of the latest call.

Scores
------
``evaluate_mesh`` scores a reconstructed mesh against a ground-truth cloud, ``evaluate_point_cloud_on_mesh`` a cloud against a
ground-truth surface; see their docstrings.  The side that measures *to* the mesh is exact; the other side samples the mesh,
because a distance from a surface to a cloud is an integral and not a minimum.  ``evaluate_mesh_ply`` and
``evaluate_ply_on_mesh`` are the same on PLY files.

Out of scope
------------
Closest points and barycentrics of the foot point; signed distances; mesh-to-mesh Hausdorff distances; a BVH.
"""
import numpy as np
import torch

from . import _lib, evaluation, mesh_ops
from .evaluation import FINE_CELLS_PER_MAX_DIST, FINE_RINGS, MARGIN  # the search's grid parameters are nearest_distances'

MAX_FACES = 2 ** 27 - 2 ** 13                  # PF_MESH_DIST_MAX_FACES: the budget below then stays under 2^31 pairs
BUDGET_PER_FACE = 16
BUDGET_BASE = 1 << 16

_last_report = {}


def pair_budget(num_faces):
    """The most (cell, face) pairs a grid may hold: ``16 Nf + 2^16``."""
    return BUDGET_PER_FACE * int(num_faces) + BUDGET_BASE


def last_grid_report():
    """What the latest ``point_mesh_distances`` call did, as a dict: ``queries``, ``faces``, ``budget``; for the fine grid
    ``fine_edge_first`` / ``fine_pairs_first`` (the first edge tried and its pair count, clamped per face to ``budget + 1``),
    ``fine_edge`` / ``fine_pairs`` (the grid used) and ``fine_widenings``; ``second_pass_queries``; and, when there were any,
    the same five ``coarse_`` entries.  Empty after a call that needed no search."""
    return dict(_last_report)


class _FaceGrid(object):
    """The (cell, face) pairs of a mesh on a grid of cell edge >= ``edge``, sorted by cell: ``keys`` and 48-byte ``records``."""

    def __init__(self, vertices, faces32, lo, hi, edge):
        Nv, Nf = int(vertices.shape[0]), int(faces32.shape[0])
        dev = vertices.device
        budget = pair_budget(Nf)
        self.widenings = 0
        count = torch.empty((Nf,), dtype=torch.int64, device=dev)
        while True:
            self.edge, self.origin, self.cells = evaluation._grid_frame(lo, hi, edge)
            _lib.call("pf_mesh_dist_count_f32", _lib.ptr(vertices), Nv, _lib.ptr(faces32), Nf,
                      *(self.args() + [budget + 1, _lib.ptr(count), _lib.stream()]), algo_bytes=Nf * (12 + 36 + 8))
            incl = torch.cumsum(count, dim=0)                              # plumbing
            total = int(incl[-1])                                          # the grid's one host read
            if self.widenings == 0:
                self.edge_first, self.pairs_first = self.edge, total
            if total <= budget:
                break
            if max(self.cells) <= 2:                                       # at most 8 pairs per face: cannot happen
                raise RuntimeError("point_mesh_distances: %d pairs on a grid of %s cells" % (total, self.cells))
            edge = 2.0 * self.edge                                         # exact in float32: the frame keeps it as it is
            self.widenings += 1
        self.pairs = total
        self.keys = torch.empty((0,), dtype=torch.int64, device=dev)
        self.records = torch.empty((0, 12), dtype=torch.int32, device=dev)
        if total:
            keys = torch.empty((total,), dtype=torch.int64, device=dev)
            pair_face = torch.empty((total,), dtype=torch.int32, device=dev)
            # per pair ~log2(Nf) sums of the search, its face's indices and vertices in, 12 bytes out
            _lib.call("pf_mesh_dist_emit_f32", _lib.ptr(vertices), Nv, _lib.ptr(faces32), Nf,
                      *(self.args() + [_lib.ptr(incl), total, _lib.ptr(keys), _lib.ptr(pair_face), _lib.stream()]),
                      algo_bytes=total * (8 * max(1, Nf.bit_length()) + 48 + 12))
            self.keys, order = torch.sort(keys, stable=True)              # plumbing
            self.records = torch.empty((total, 12), dtype=torch.int32, device=dev)
            _lib.call("pf_mesh_dist_pack_f32", _lib.ptr(vertices), Nv, _lib.ptr(faces32), Nf, _lib.ptr(pair_face),
                      _lib.ptr(order), total, _lib.ptr(self.records), _lib.stream(), algo_bytes=total * (12 + 12 + 36 + 48))

    def args(self):
        return self.origin + [self.edge] + self.cells

    def report(self, prefix):
        return {prefix + "edge_first": self.edge_first, prefix + "pairs_first": self.pairs_first, prefix + "edge": self.edge,
                prefix + "pairs": self.pairs, prefix + "widenings": self.widenings}


def _mesh_box(vertices):
    """``(lo, hi)`` float64 (3,) over the finite vertices, or None when there is none (plumbing, one host read)."""
    finite = torch.isfinite(vertices).all(dim=1)
    big = torch.finfo(torch.float32).max
    lo = torch.where(finite[:, None], vertices, vertices.new_full((), big)).amin(dim=0)
    hi = torch.where(finite[:, None], vertices, vertices.new_full((), -big)).amax(dim=0)
    box = torch.stack([lo, hi]).cpu().numpy().astype(np.float64)
    if not bool(finite.any()):
        return None
    return box[0], box[1]


def _first_pass(points, grid, cap, dist, face, done):
    nq = int(points.shape[0])
    _lib.call("pf_mesh_dist_cells_f64", _lib.ptr(points), nq, _lib.ptr(grid.records), _lib.ptr(grid.keys), grid.pairs,
              *(grid.args() + [FINE_RINGS, cap, _lib.ptr(dist), _lib.ptr(face), _lib.ptr(done), _lib.stream()]))


def _second_pass(points, todo, grid, cap, dist, face):
    _lib.call("pf_mesh_dist_wave_f64", _lib.ptr(points), _lib.ptr(todo), int(todo.numel()), int(points.shape[0]),
              _lib.ptr(grid.records), _lib.ptr(grid.keys), grid.pairs,
              *(grid.args() + [cap, _lib.ptr(dist), _lib.ptr(face), _lib.stream()]))


def _check_max_dist(who, max_dist):
    try:
        cap = float(np.float32(max_dist))
    except (TypeError, ValueError):
        raise ValueError("%s: max_dist must be a positive length" % who)
    if not (cap > 0.0 and np.isfinite(cap)):
        raise ValueError("%s: max_dist must be a positive length" % who)
    return cap


def _check_values(who, points, vertices, faces, max_dist, obs_mask=None, bb_min=None, res=None):
    """``(points, Nv, Nf, cap)`` from the checks that need no device."""
    points = evaluation._check_points(points, who, gpu=False)
    Nv, Nf = mesh_ops._check_mesh(who, vertices, faces)
    if Nf > MAX_FACES:
        raise ValueError("%s: more than 2^27 - 2^13 faces" % who)
    cap = _check_max_dist(who, max_dist)
    if obs_mask is not None and (bb_min is None or res is None):
        raise ValueError("%s: obs_mask needs bb_min and res" % who)
    return points, Nv, Nf, cap


def _check_devices(who, points, vertices, faces):
    _lib.require_gpu(points, vertices, faces)
    if points.device != vertices.device:
        raise ValueError("%s: points and mesh must be on one device" % who)


def point_mesh_distances(points, vertices, faces, max_dist=20.0, return_face=False):
    """Per point of ``points`` (N, 3) its distance to the surface of the mesh, capped at ``max_dist``, by the module
    docstring: float32 (N,); with ``return_face`` also the int64 index of the face that attains it (the smallest such index;
    -1 at the cap).  Synchronises with the host for the index check, the mesh's box and once per grid built."""
    global _last_report
    who = "point_mesh_distances"
    points, Nv, Nf, cap = _check_values(who, points, vertices, faces, max_dist)
    _check_devices(who, points, vertices, faces)
    faces32 = mesh_ops._faces32(who, faces, Nv, vertices)
    nq = int(points.shape[0])
    dev = points.device
    _last_report = {}
    with _lib.on_device(dev):
        vertices = vertices.contiguous()
        dist = torch.full((nq,), cap, dtype=torch.float32, device=dev)
        face = torch.full((nq,), -1, dtype=torch.int32, device=dev)
        box = _mesh_box(vertices) if nq and Nf and Nv else None
        if box is not None:
            fine, coarse, unfinished = evaluation._two_pass_search(
                points, cap, lambda edge: _FaceGrid(vertices, faces32, box[0], box[1], edge), _first_pass, _second_pass,
                dist, face)
            report = {"queries": nq, "faces": Nf, "budget": pair_budget(Nf), "second_pass_queries": unfinished}
            report.update(fine.report("fine_"))
            if coarse is not None:
                report.update(coarse.report("coarse_"))
            _last_report = report
    return (dist, face.long()) if return_face else dist


def _sample(vertices, faces, pitch, seed):
    if int(faces.shape[0]) == 0 or int(vertices.shape[0]) == 0:
        mesh_ops._check_sampling("sample_surface", pitch, seed)
        return torch.zeros((0, 3), dtype=torch.float32, device=vertices.device)
    return mesh_ops.sample_surface(vertices, faces, pitch, seed)[0]


def evaluate_mesh(vertices, faces, gt, pitch=0.2, max_dist=20.0, obs_mask=None, bb_min=None, res=None, plane=None, seed=0,
                  return_distances=False):
    """DTU's scores of a reconstructed mesh against the ground-truth cloud ``gt`` as a dict of Python numbers.

    ``samples = sample_surface(vertices, faces, pitch, seed)[0]``.  ``d_acc = nearest_distances(samples, gt, max_dist)`` is
    used where ``in_obs_mask(samples, obs_mask, bb_min, res)`` (everywhere without a mask) and ``d_acc < max_dist``; there is no
    thinning, because the samples are already uniform.  ``d_comp = point_mesh_distances(gt, vertices, faces, max_dist)`` --
    **exact** -- is used where ``above_plane(gt, plane)`` (everywhere without a plane) and ``d_comp < max_dist``.  The keys are
    ``evaluate_point_cloud``'s (float64 sums, the lower median, ``nan`` over an empty set), with ``n_data = n_data_thinned =
    n_samples`` the number of samples.  With ``return_distances`` the dict also holds the tensors ``samples``, ``d_acc``,
    ``d_comp``, ``acc_used``, ``comp_used``."""
    who = "evaluate_mesh"
    gt, _, _, cap = _check_values(who, gt, vertices, faces, max_dist, obs_mask, bb_min, res)
    _check_devices(who, gt, vertices, faces)
    samples = _sample(vertices, faces, pitch, seed)
    d_acc = evaluation.nearest_distances(samples, gt, max_dist)
    d_comp = point_mesh_distances(gt, vertices, faces, max_dist)
    n = int(samples.shape[0])
    return evaluation._scores(d_acc, samples, d_comp, gt, cap,
                              {"n_data": n, "n_data_thinned": n, "n_gt": int(gt.shape[0]), "n_samples": n},
                              {"samples": samples} if return_distances else None, obs_mask, bb_min, res, plane)


def evaluate_point_cloud_on_mesh(data, gt_vertices, gt_faces, gt_pitch=0.2, min_dist=0.2, max_dist=20.0, obs_mask=None,
                                 bb_min=None, res=None, plane=None, thin=True, seed=0, return_distances=False):
    """DTU's scores of the reconstructed cloud ``data`` against a ground-truth *surface* as a dict of Python numbers.

    ``data' = thin_points(data, min_dist)`` when ``thin``.  ``d_acc = point_mesh_distances(data', gt_vertices, gt_faces,
    max_dist)`` -- **exact** -- is used where ``in_obs_mask(data', obs_mask, bb_min, res)`` (everywhere without a mask) and
    ``d_acc < max_dist``.  ``samples = sample_surface(gt_vertices, gt_faces, gt_pitch, seed)[0]`` stand for the surface in the
    other direction: ``d_comp = nearest_distances(samples, data', max_dist)`` is used where ``above_plane(samples, plane)``
    (everywhere without a plane) and ``d_comp < max_dist``.  The keys are ``evaluate_point_cloud``'s, with ``n_gt = n_samples``
    the number of samples.  With ``return_distances`` the dict also holds the tensors ``data_thinned``, ``samples``, ``d_acc``,
    ``d_comp``, ``acc_used``, ``comp_used``."""
    who = "evaluate_point_cloud_on_mesh"
    data, _, _, cap = _check_values(who, data, gt_vertices, gt_faces, max_dist, obs_mask, bb_min, res)
    _check_devices(who, data, gt_vertices, gt_faces)
    thinned = evaluation.thin_points(data, min_dist) if thin else data
    samples = _sample(gt_vertices, gt_faces, gt_pitch, seed)
    d_acc = point_mesh_distances(thinned, gt_vertices, gt_faces, max_dist)
    d_comp = evaluation.nearest_distances(samples, thinned, max_dist)
    n = int(samples.shape[0])
    counts = {"n_data": int(data.shape[0]), "n_data_thinned": int(thinned.shape[0]), "n_gt": n, "n_samples": n}
    return evaluation._scores(d_acc, thinned, d_comp, samples, cap, counts,
                              {"data_thinned": thinned, "samples": samples} if return_distances else None,
                              obs_mask, bb_min, res, plane)


def load_ply_surface(path, dev):
    from .utils import io as IO
    vertices, _, _, faces = IO.load_ply_mesh(path)
    if faces is None or not len(faces):
        raise ValueError("%s has no faces" % path)
    return (torch.from_numpy(np.ascontiguousarray(vertices, dtype=np.float32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(faces).astype(np.int64)).to(dev))


def evaluate_mesh_ply(data_ply, gt_ply, obs_mask_mat=None, plane_mat=None, pitch=0.2, max_dist=20.0, seed=0, device=None,
                      return_distances=False):
    """``evaluate_mesh`` of a PLY with faces (``utils.io.load_ply_mesh``) against the vertices of a ground-truth PLY, with
    DTU's ``ObsMask<scan>_10.mat`` / ``Plane<scan>.mat`` when given, as ``evaluation.evaluate_ply``."""
    from .utils import io as IO
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    vertices, faces = load_ply_surface(data_ply, dev)
    gt = torch.from_numpy(IO.load_ply_points(gt_ply)).to(dev)
    return evaluate_mesh(vertices, faces, gt, pitch=pitch, max_dist=max_dist, seed=seed, return_distances=return_distances,
                         **evaluation._dtu_filters(obs_mask_mat, plane_mat))


def evaluate_ply_on_mesh(data_ply, gt_mesh_ply, obs_mask_mat=None, plane_mat=None, gt_pitch=0.2, min_dist=0.2, max_dist=20.0,
                         thin=True, seed=0, device=None, return_distances=False):
    """``evaluate_point_cloud_on_mesh`` of the vertices of a PLY against a ground-truth PLY with faces."""
    from .utils import io as IO
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    data = torch.from_numpy(IO.load_ply_points(data_ply)).to(dev)
    gt_vertices, gt_faces = load_ply_surface(gt_mesh_ply, dev)
    return evaluate_point_cloud_on_mesh(data, gt_vertices, gt_faces, gt_pitch=gt_pitch, min_dist=min_dist, max_dist=max_dist,
                                        thin=thin, seed=seed, return_distances=return_distances,
                                        **evaluation._dtu_filters(obs_mask_mat, plane_mat))
