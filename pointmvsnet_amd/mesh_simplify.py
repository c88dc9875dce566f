"""Simplify a triangle mesh on the GPU: vertex clustering with quadric placement.

``tsdf.extract_mesh`` makes a mesh whose density is the voxel's whatever the surface looks like, with the slivers and
zero-area faces that marching tetrahedra make by construction.  This module merges all vertices of a grid cell into one
(Rossignac-Borrel clusters) and puts that one where the planes of the cluster's faces meet best (Lindstrom's quadrics,
weighted by squared area).  There is no priority queue and no sequential edge collapse: it is the sorted-cell idiom of
``cloud_filter.voxel_downsample`` -- whose two kernels do the clustering here -- plus four HIP kernels
(csrc/mesh_simplify.hip), and the result is a pure function of the input.  **The specification below is this project's
own**; parity with Open3D (``simplify_vertex_clustering``), MeshLab or any paper's code is neither claimed nor tested.  The
library is built with ``-ffp-contract=off``, so "float64 in this order" is meant literally.

``simplify_mesh(vertices, faces, cell, colours=None, placement="quadric", regularisation=1e-3, origin=None)``

Inputs
------
``mesh_ops``' contract: ``vertices`` (Nv, 3) float32 and ``faces`` (Nf, 3) int32 or int64 on one GPU, the index range checked
once.  A face may name a vertex twice, faces may be duplicated or have no area, ``Nv == 0`` or ``Nf == 0`` work.  A non-finite
vertex coordinate is a ``ValueError`` (the cell rule is not defined for it).  ``colours`` (Nv, 3) uint8 or None.  Arguments are
checked before a GPU is needed.  There is no CPU path.

1. Clusters.  Exactly ``voxel_downsample``'s rule (cloud_filter.py, 4.): ``inv = float32(1) / float32(cell)`` made on the
   host, cell ``floorf((p - o) * inv)`` per axis in float32, ``o`` the per-axis float32 minimum of the vertices or the given
   ``origin`` (float32; not ``<=`` that minimum on every axis: ``ValueError``); more than 2^17 cells on an axis is a
   ``ValueError``.  Clusters are numbered in ascending ``(cx, cy, cz)`` order; ``C(v)`` is the cluster of vertex ``v``.  Per
   cluster, ``m`` is the float32-rounded float64 mean of its members summed in ascending vertex index, and its colour is
   ``(2 * sum + count) // (2 * count)`` per channel.  Every vertex is clustered, whether a face names it or not.
2. Faces.  Face ``(a, b, c)`` becomes ``(C(a), C(b), C(c))``, rotation and winding untouched.  It is *collapsed*, and dropped,
   if two of the three clusters are equal.  Among the others, two with the same unordered cluster triple are *duplicates*:
   the one with the lowest input face index is kept, with its own winding (a mirrored twin goes as well).  Output faces come
   in ascending input face index (``face_source``).  Integers only; the sort by triple and the compaction are torch plumbing.
3. Vertices.  The output vertices are the clusters that a kept face names, in cluster order; a cluster none of whose faces
   was kept is *unreferenced* and not output.  ``vertex_map[v]`` is the output row of ``C(v)``, -1 for an unreferenced one.
   Colours are those of the cluster.
4. Placement, per cluster.  ``"mean"`` gives ``m``.  ``"quadric"`` works in float64 in coordinates relative to ``m``: every
   float32 coordinate is converted exactly and ``p' = p - m`` per coordinate.  The cluster owns the corners ``3 f + j`` with
   ``C(faces[f, j])`` equal to it, in ascending order (``mesh_ops.vertex_corner_table``'s idiom: a stable torch sort); a face
   with two corners in the cluster counts twice.  Per corner, with the face's ``(a, b, c)`` in its own order:
   ``e1 = p_b' - p_a'``, ``e2 = p_c' - p_a'``, ``n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x)`` (a product, a
   product and a difference each), the corner skipped if a component is not finite; ``d = -((nx ax' + ny ay') + nz az')``;
   ``A += n n^T`` (six sums ``nx nx, nx ny, nx nz, ny ny, ny nz, nz nz``) and ``b += d n`` (three sums ``d nx, d ny, d nz``).
   ``n`` is not normalised: a face weighs 4 area^2 and there is no square root.

   Order of the nine sums: a cluster with fewer than ``WAVE_MIN_CORNERS`` corners adds them in ascending corner order (one
   thread).  A longer list is shared by a wave of 64 lanes: lane ``l`` adds list entries ``l, l + 64, ..`` in that order,
   then the lanes are combined pairwise, ``s_l += s_(l xor 32)``, then ``xor 16, 8, 4, 2, 1``.  The path depends on the length
   of the list alone and there are no float atomics: two runs give identical bytes.

   ``t = (A00 + A11) + A22``.  Unless ``t`` is finite and positive the position is ``m``.  Otherwise
   ``lam = (regularisation * t) / 3`` and ``(A + lam I) x = -b`` -- the minimiser of the quadric plus ``lam |x|^2``, a pull
   towards ``m``; the matrix is symmetric positive definite with condition number at most ``3 / regularisation + 1``, which
   is the point of the term -- is solved by the root-free Cholesky factorisation ``L D L^T`` in this order:
   ``m00 = A00 + lam`` (``m11``, ``m22`` alike); ``l10 = A01 / m00``; ``l20 = A02 / m00``; ``d1 = m11 - l10 A01``;
   ``u21 = A12 - l20 A01``; ``l21 = u21 / d1``; ``d2 = m22 - (l20 A02 + l21 u21)``; ``y0 = -b0``; ``y1 = -b1 - l10 y0``;
   ``y2 = -b2 - (l20 y0 + l21 y1)``; ``x2 = y2 / d2``; ``x1 = y1 / d1 - l21 x2``; ``x0 = y0 / m00 - (l10 x1 + l20 x2)``.
   If ``|x_k| <= float32(cell)`` fails for some ``k`` the position is ``m``: a *fallback*, counted in the report for the
   clusters that are output.  Otherwise it is ``float32(m + x)`` per coordinate.  ``regularisation`` is finite and in
   ``[1e-6, 1]``.
5. ``report``: plain integers ``vertices_in``, ``faces_in``, ``vertices_out``, ``faces_out``, ``clusters``, ``collapsed``,
   ``duplicates``, ``fallback``, ``unreferenced_clusters``.

A closed form: an output vertex lies within ``cell`` per axis of its cluster's mean, and the mean lies in the cluster's cell
(up to float32 rounding), which holds every member.  So an input vertex with ``vertex_map >= 0`` is at most
``2 sqrt(3) cell`` from the simplified surface.

``mesh_edge_counts(faces)`` (plain torch, CPU tensors work): the undirected edges ``{a, b}``, ``a != b``, of the faces, each
counted once per face side that has it: ``boundary`` edges occur once, ``manifold`` edges twice, ``nonmanifold`` edges more
often.  Clustering can make non-manifold edges; they are counted, not repaired.

Out of scope
------------
Smoothing; edge-collapse decimation to a target face count; feature-sensitive or adaptive cell sizes; repair of
non-manifold edges; normals carried through clustering (``mesh_ops.vertex_normals`` recomputes them on the result).
"""
import math

import numpy as np
import torch

from . import _lib, cloud_filter, mesh_ops

PLACEMENTS = ("quadric", "mean")
MIN_REGULARISATION = 1e-6                      # PF_MESH_SIMPLIFY_MIN_REG of include/pointflow_hip.h
WAVE_MIN_CORNERS = 16                          # a cluster with this many corners or more gets a wave, a shorter list a thread:
                                               # the best of 0, 4, 8, 16, 32, .. 1024 and "never" over cells of 0.5 to 8 voxels
                                               # (profiles/mesh_simplify_microbench.jsonl)


def _check_arguments(who, cell, placement, regularisation, origin):
    """``(inv, float32 cell, regularisation, origin as float32 (3,) or None)`` from the checks that need no tensor."""
    inv = cloud_filter._voxel_inverse(cell, who, "cell")
    if placement not in PLACEMENTS:
        raise ValueError("%s: placement must be one of %s" % (who, ", ".join(PLACEMENTS)))
    try:
        reg = float(regularisation)
    except (TypeError, ValueError):
        raise ValueError("%s: regularisation must be a number in [1e-6, 1]" % who)
    if isinstance(regularisation, bool) or not (math.isfinite(reg) and MIN_REGULARISATION <= reg <= 1.0):
        raise ValueError("%s: regularisation must be a number in [1e-6, 1]" % who)
    if origin is not None:
        try:
            origin = np.asarray(origin.cpu() if isinstance(origin, torch.Tensor) else origin, dtype=np.float32).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("%s: origin must be three finite numbers" % who)
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError("%s: origin must be three finite numbers" % who)
    return inv, np.float32(cell), reg, origin


def check_simplify_arguments(who, cell, placement="quadric", regularisation=1e-3, origin=None):
    """The argument checks of ``simplify_mesh`` that need no mesh (``ScanAccumulator.mesh`` judges its own with them)."""
    _check_arguments(who, cell, placement, regularisation, origin)


def _classify_faces(faces32, Nv, cluster, M):
    """``(triple (Nf, 3) int32, ascending (Nf, 3) int32, collapsed (Nf,) uint8)`` of section 2."""
    Nf, dev = int(faces32.shape[0]), faces32.device
    triple = torch.empty((Nf, 3), dtype=torch.int32, device=dev)
    ascending = torch.empty((Nf, 3), dtype=torch.int32, device=dev)
    collapsed = torch.empty((Nf,), dtype=torch.uint8, device=dev)
    if Nf:
        # per face its three indices, three cluster entries, two triples and a flag out
        _lib.call("pf_mesh_simplify_faces", _lib.ptr(faces32), Nf, Nv, _lib.ptr(cluster), M, _lib.ptr(triple),
                  _lib.ptr(ascending), _lib.ptr(collapsed), _lib.stream(), algo_bytes=Nf * (12 + 24 + 24 + 1))
    return triple, ascending, collapsed


def _sort_by_triple(ascending, survivors, M):
    """The surviving faces ordered by their ascending triple, ascending face index inside a run (plumbing: two stable
    sorts, the last entry first, then ``lo * M + mid``, which is below 2^62)."""
    asc = ascending[survivors].long()
    first = torch.sort(asc[:, 2], stable=True)[1]
    second = torch.sort((asc[:, 0] * max(M, 1) + asc[:, 1])[first], stable=True)[1]
    return survivors[first[second]]


def _keep_first(ascending, sorted_faces):
    """``keep (Nf,) uint8``: 1 for the first face of every run of equal triples in ``sorted_faces``, else 0."""
    Nf, K = int(ascending.shape[0]), int(sorted_faces.shape[0])
    keep = torch.zeros((Nf,), dtype=torch.uint8, device=ascending.device)
    if K:
        _lib.call("pf_mesh_simplify_keep_first", _lib.ptr(ascending), Nf, _lib.ptr(sorted_faces), K, _lib.ptr(keep),
                  _lib.stream(), algo_bytes=K * (16 + 24 + 1))
    return keep


def _cluster_corner_table(triple, M):
    """``mesh_ops.vertex_corner_table`` with the cluster in place of the vertex: ``(offsets (M + 1,) int64, corners (3 Nf,)
    int64)``, cluster ``s`` owning ``corners[offsets[s]:offsets[s + 1]]`` in ascending order (plumbing: a stable sort of the
    int32 cluster numbers, then a binary search for every cluster's first slot)."""
    ids, corners = torch.sort(triple.reshape(-1), stable=True)
    offsets = torch.searchsorted(ids, torch.arange(M + 1, dtype=torch.int32, device=triple.device))
    return offsets, corners


def _corner_lengths(offsets):
    return offsets[1:] - offsets[:-1]


def _quadric_positions(vertices, faces32, offsets, corners, means, cell32, reg, threshold=WAVE_MIN_CORNERS):
    """``(positions (M, 3) float32, fallback (M,) uint8)`` of section 4: clusters with fewer than ``threshold`` corners by the
    thread kernel, the others by the wave kernel (the microbenchmark varies ``threshold``)."""
    Nv, Nf, M, dev = int(vertices.shape[0]), int(faces32.shape[0]), int(means.shape[0]), vertices.device
    positions = torch.zeros((M, 3), dtype=torch.float32, device=dev)
    fallback = torch.zeros((M,), dtype=torch.uint8, device=dev)
    if M == 0:
        return positions, fallback
    lengths = _corner_lengths(offsets)
    todo = torch.nonzero(lengths >= threshold).view(-1)                 # plumbing: the long lists (one host read)
    ntodo = int(todo.numel())
    long_corners = int(lengths[todo].sum()) if ntodo and _lib.timing() else 0       # a host read that only algo_bytes needs
    # per corner its list entry, the face's indices and three vertices; per cluster two offsets, the mean and 13 bytes out
    per_corner, per_cluster = 8 + 12 + 36, 16 + 12 + 13
    if ntodo < M:
        _lib.call("pf_mesh_quadric_thread_f64", _lib.ptr(vertices), Nv, _lib.ptr(faces32), Nf, _lib.ptr(offsets),
                  _lib.ptr(corners), _lib.ptr(means), M, float(cell32), reg, int(threshold), _lib.ptr(positions),
                  _lib.ptr(fallback), _lib.stream(), algo_bytes=(3 * Nf - long_corners) * per_corner + M * per_cluster)
    if ntodo:
        _lib.call("pf_mesh_quadric_wave_f64", _lib.ptr(vertices), Nv, _lib.ptr(faces32), Nf, _lib.ptr(offsets),
                  _lib.ptr(corners), _lib.ptr(means), M, float(cell32), reg, _lib.ptr(todo), ntodo, _lib.ptr(positions),
                  _lib.ptr(fallback), _lib.stream(), algo_bytes=long_corners * per_corner + ntodo * (per_cluster + 8))
    return positions, fallback


def simplify_mesh(vertices, faces, cell, colours=None, placement="quadric", regularisation=1e-3, origin=None,
                  return_maps=False):
    """Cluster the mesh's vertices on a grid of edge ``cell`` and place one vertex per cluster (module docstring).  Returns
    ``(vertices (Mv, 3) float32, faces (Mf, 3) in the dtype given, colours (Mv, 3) uint8 or None, report)`` and with
    ``return_maps`` also ``vertex_map`` (Nv,) int64 (old to new, -1 if dropped) and ``face_source`` (Mf,) int64 (the input
    face of each output face).  Synchronises with the host a few times (the checks and the counts).  There is no CPU path."""
    who = "simplify_mesh"
    Nv, Nf = mesh_ops._check_mesh(who, vertices, faces)
    inv, cell32, reg, origin = _check_arguments(who, cell, placement, regularisation, origin)
    if colours is not None and not isinstance(colours, torch.Tensor):
        raise ValueError("%s: colours must be an (Nv, 3) uint8 tensor" % who)
    colours = cloud_filter._check_attribute(colours, Nv, vertices.device, torch.uint8, who, "colours")
    vertices = vertices.contiguous()
    if Nv:
        if not bool(torch.isfinite(vertices).all()):
            raise ValueError("%s: non-finite vertex coordinates" % who)
        lo, cells = cloud_filter._voxel_cells(vertices, inv, who, origin)
    faces32 = mesh_ops._faces32(who, faces, Nv, vertices)
    dev = vertices.device
    with _lib.on_device(dev):
        M, fallen = 0, 0
        if Nv:
            means, cluster_colours, _, _, cluster, _ = cloud_filter._voxel_reduce(vertices, lo, inv, cells, colours, None, True)
            M = int(means.shape[0])
        else:
            means, cluster_colours = vertices, colours
            cluster = torch.zeros((0,), dtype=torch.int64, device=dev)
        triple, ascending, collapsed = _classify_faces(faces32, Nv, cluster, M)
        survivors = torch.nonzero(collapsed == 0).view(-1)                 # plumbing: ascending face index
        keep = _keep_first(ascending, _sort_by_triple(ascending, survivors, M))
        face_source = torch.nonzero(keep).view(-1)
        kept = triple[face_source].long()
        used = torch.zeros((M,), dtype=torch.bool, device=dev)
        used[kept.reshape(-1)] = True
        cluster_map = torch.where(used, torch.cumsum(used, dim=0, dtype=torch.int64) - 1,
                                  torch.full((M,), -1, dtype=torch.int64, device=dev))
        if placement == "quadric" and M:
            offsets, corners = _cluster_corner_table(triple, M)
            positions, fallback = _quadric_positions(vertices, faces32, offsets, corners, means, cell32, reg)
            fallen = int((fallback.bool() & used).sum())
        else:
            positions = means
        out_vertices = positions[used]
        out_faces = cluster_map[kept].to(faces.dtype)
        out_colours = None if cluster_colours is None else cluster_colours[used]
        vertex_map = cluster_map[cluster]
    Mv, Mf, K = int(out_vertices.shape[0]), int(out_faces.shape[0]), int(survivors.numel())
    report = {"vertices_in": Nv, "faces_in": Nf, "vertices_out": Mv, "faces_out": Mf, "clusters": M, "collapsed": Nf - K,
              "duplicates": K - Mf, "fallback": fallen, "unreferenced_clusters": M - Mv}
    return (out_vertices, out_faces, out_colours, report) + ((vertex_map, face_source) if return_maps else ())


def mesh_edge_counts(faces):
    """``{"boundary", "manifold", "nonmanifold"}``: the undirected edges of ``faces`` (Nf, 3) integer that one, two and more
    than two face sides share (module docstring; plain torch on the device of ``faces``)."""
    if (not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point
            or faces.dtype == torch.bool):
        raise ValueError("mesh_edge_counts: faces must be an (Nf, 3) integer tensor")
    f = faces.long()
    if f.numel() and int(f.min()) < 0:
        raise ValueError("mesh_edge_counts: negative face index")
    edges = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    edges = edges[edges[:, 0] != edges[:, 1]]
    out = {"boundary": 0, "manifold": 0, "nonmanifold": 0}
    if edges.shape[0]:
        lo, hi = edges.min(dim=1)[0], edges.max(dim=1)[0]
        counts = torch.unique(lo * (int(hi.max()) + 1) + hi, return_counts=True)[1]
        out = {"boundary": int((counts == 1).sum()), "manifold": int((counts == 2).sum()),
               "nonmanifold": int((counts > 2).sum())}
    return out
