"""Mesh clean-up and scoring on the GPU: connected components, removal of small pieces, vertex normals and surface sampling.

``tsdf.extract_mesh`` ends the pipeline in a triangle mesh that nobody would use as it is: a TSDF of noisy depth maps grows
detached fragments wherever ``min_weight`` views agree on a floater, the mesh has no normals, and it can only be scored by
its vertices, whose density is the voxel's.  The three remedies all need the mesh's connectivity on the GPU, and all three
are pure functions of their input here, as everything else in this pipeline.  They run as six HIP kernels
(csrc/mesh_ops.hip).  **The specification below is this project's own**; parity with Open3D
(``cluster_connected_triangles``, ``compute_vertex_normals``, ``sample_points_uniformly``), MeshLab or PCL is neither
claimed nor tested.  The library is built with ``-ffp-contract=off``, so "float32 in this order" is meant literally.

Inputs
------
``vertices`` (Nv, 3) float32 and ``faces`` (Nf, 3) int32 or int64 on one GPU, ``Nv, Nf < 2^31``.  The face indices are
checked once with torch min / max (one host synchronisation); an index outside ``[0, Nv)`` is a ValueError.  The kernels
skip any face with such an index all the same: no input faults.  A face may name a vertex twice, faces may be duplicated
or have no area (``extract_mesh`` keeps those), vertices may be non-finite, and ``Nf == 0`` or ``Nv == 0`` work.  Arguments
are checked before a GPU is needed.  There is no CPU path.

Connected components
--------------------
``mesh_components(faces, num_vertices)``.  Two vertices are connected when a face names both.  ``vertex_label[v]`` is the
**smallest vertex index of v's component** (a vertex that no face names is its own component), ``face_label[f]`` the label
of the face's first vertex.  That answer is unique: two runs give identical bytes, and a permutation of the faces gives the
same vertex labels.

The route is hook-and-compress (Shiloach-Vishkin style) on one ``label`` array with ``label[v] = v`` at first.  A *round*
is one hook launch over the faces (the larger root of every face edge is linked to the smaller by a device-scope integer
``atomicMin``; a thread whose hook met a vertex that another thread had hooked meanwhile goes on with that vertex's parent,
never waiting for anybody) and one compress launch (every vertex walks to its root).  The host reads one changed-flag per
round; a round whose hook found no edge with two different roots ends the loop.  Every store to ``label`` is an ``atomicMin``
with a vertex of the same component, so ``label[x] <= x`` holds at all times and a stale load -- the chip's L2s are not
coherent with each other -- is an earlier valid value; the argument is written out at the kernel.  The number of rounds
does not grow with the mesh's width (plain label propagation needs as many rounds as the mesh is wide).

Removing small pieces
---------------------
``remove_small_components(vertices, faces, min_faces=None, keep_largest=None, colours=None, normals=None)``.  A component's
size is its number of faces (``component_sizes(face_label)``: labels ascending, their face counts).  A component is kept if
its size is ``>= min_faces`` and, with ``keep_largest=k``, if it is among the ``k`` largest, ties going to the smaller label.
Kept faces stay in their order; kept vertices are those a kept face names, in their order (unreferenced vertices go);
faces are re-indexed; colours and normals are carried.  ``vertex_map`` (old to new, -1 for removed) and ``face_keep`` come
with ``return_maps``.  With both arguments ``None`` the mesh comes back minus its unreferenced vertices.  Integers only:
torch's ``unique``, ``sort`` and ``cumsum`` are the plumbing.

Vertex normals
--------------
``vertex_normals(vertices, faces)``: (Nv, 3) float32, unit or ``(0, 0, 0)``; area-weighted, in a fixed order.  Vertex ``v``
owns its corners ``c = 3 f + j`` with ``faces[f, j] == v``, in ascending ``c`` (``vertex_corner_table``: a stable torch sort of
``faces.view(-1)``).  Per corner's face ``(a, b, c)``, in float32: ``e1 = p_b - p_a``, ``e2 = p_c - p_a`` per coordinate,
``n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x)``, each a product, a product and a difference.  The face is
skipped if a component of ``n`` is not finite, otherwise ``n`` is added to a **float64** sum, in that corner order; a face
that names ``v`` twice counts twice.  Then ``len = sqrt((sx sx + sy sy) + sz sz)`` in float64 and the result is
``float32(s / len)`` if ``len`` is finite and positive, else zeros.  A TSDF mesh's winding makes these point towards the
cameras.  One thread per vertex walks its list, no atomics.  Valence in marching-tetrahedra meshes is a few dozen at most;
a hub vertex (the apex of a fan of 10^5 faces) is correct and slow: sharing its list across a wave would change the order
of summation.

Surface sampling
----------------
``sample_surface(vertices, faces, pitch, seed=0)``: ``points`` (N, 3) float32, ``face_index`` (N,) int32, ``bary`` (N, 3)
float32, about one sample per ``pitch^2`` of area.  ``H`` is the 32-bit hash of csrc/pf_hash.h (``x ^= x >> 16; x *=
0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16``), all sums mod 2^32, ``seed`` a 32-bit unsigned integer.

Counts.  ``inv = float32(1) / (float32(pitch) * float32(pitch))`` on the host.  Per face, in float32: ``n`` as above,
``q = (nx nx + ny ny) + nz nz``, ``area = 0.5f * sqrtf(q)``, ``x = area * inv``, ``count_f = floorf(x + u_f)`` with
``u_f = (H(H(f ^ seed)) >> 8) * 2^-24``; 0 unless ``x`` is finite; clamped to ``2^31 - 1``, so that an absurd request
overflows the total rather than the count.  This is stochastic rounding: a face far smaller than ``pitch^2`` is still
sampled in proportion to its area.  The inclusive sums are a ``torch.cumsum`` in int64; ``N > 2^31 - 1`` is a ValueError,
raised before the emit launch (one host synchronisation).

Samples.  One thread per *sample* finds its face by binary search in the inclusive sums.  Sample ``j`` of face ``f`` has
``r1 = (H(H(f ^ seed) + 2j + 1) >> 8) * 2^-24`` and ``r2`` likewise with ``2j + 2``.  If ``r1 + r2 > 1`` both become ``1 - r``;
all are multiples of ``2^-24``, so this is exact (the kernel decides it on the integers).  ``bary = (1 - r1 - r2, r1, r2)``,
exact, never negative, summing to 1 exactly.  ``point = p_a + (r1 e1 + r2 e2)`` per coordinate in float32, in that order.
(The reflection makes the fold uniform; no square root is needed, and none is used.)  Samples come in ascending face, then
``j``.  Attributes are interpolated by ``render.interpolate_vertex_attributes(face_index.view(1, 1, -1),
bary.view(1, 1, -1, 3), faces, attributes)``.

Out of scope
------------
Smoothing; edge-collapse decimation; hole filling; non-manifold repair; edge-connectivity (as opposed to
vertex-connectivity) components; area thresholds for components; a wave-shared path for hub vertices.  (Point-to-triangle
distances are pointmvsnet_amd/mesh_distance.py; simplification by vertex clustering is pointmvsnet_amd/mesh_simplify.py.)
"""
import math

import numpy as np
import torch

from . import _lib

MAX_COUNT = 2 ** 31 - 1                        # PF_MESH_OPS_MAX of include/pointflow_hip.h
_FLAGS = 32                                    # changed-flags per allocation: one per round, re-zeroed when used up

_last_rounds = 0


def last_component_rounds():
    """The rounds (hook launch, compress launch, one flag read) of the latest ``mesh_components`` call."""
    return _last_rounds


def _check_faces(who, faces, num_vertices):
    """``(Nv, Nf)`` from the checks that need no device."""
    if (not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3
            or faces.dtype not in (torch.int32, torch.int64)):
        raise ValueError("%s: faces must be an (Nf, 3) int32 or int64 tensor" % who)
    if isinstance(num_vertices, bool) or not isinstance(num_vertices, (int, np.integer)) or num_vertices < 0:
        raise ValueError("%s: num_vertices must be a non-negative integer" % who)
    Nv, Nf = int(num_vertices), int(faces.shape[0])
    if Nv > MAX_COUNT or Nf > MAX_COUNT:
        raise ValueError("%s: a mesh has fewer than 2^31 vertices and fewer than 2^31 faces" % who)
    return Nv, Nf


def _check_mesh(who, vertices, faces):
    if (not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3
            or vertices.dtype != torch.float32):
        raise ValueError("%s: vertices must be an (Nv, 3) float32 tensor" % who)
    return _check_faces(who, faces, int(vertices.shape[0]))


def _check_range(who, faces, Nv):
    """The one look at the face indices: torch min / max, one host synchronisation."""
    if faces.shape[0] == 0:
        return
    lo, hi = (int(x) for x in torch.stack(torch.aminmax(faces)).tolist())
    if lo < 0 or hi >= Nv:
        raise ValueError("%s: face indices run from %d to %d, the mesh has %d vertices" % (who, lo, hi, Nv))


def _faces32(who, faces, Nv, vertices=None):
    """``faces`` range-checked, contiguous and int32, on its GPU (which must be that of ``vertices``)."""
    _lib.require_gpu(faces, vertices)
    if vertices is not None and vertices.device != faces.device:
        raise ValueError("%s: vertices and faces must be on one device" % who)
    _check_range(who, faces, Nv)
    return faces.to(torch.int32).contiguous()


def _cc_hook(faces32, Nv, label, flag):
    Nf = int(faces32.shape[0])
    # per face its three indices and, on a compressed forest, two label loads per corner
    _lib.call("pf_mesh_cc_hook", _lib.ptr(faces32), Nf, Nv, _lib.ptr(label), _lib.ptr(flag), _lib.stream(),
              algo_bytes=Nf * (12 + 24))


def _cc_compress(label):
    Nv = int(label.shape[0])
    _lib.call("pf_mesh_cc_compress", _lib.ptr(label), Nv, _lib.stream(), algo_bytes=Nv * 12)


def _components(faces32, Nv):
    """``(label (Nv,) int32, rounds)`` of range-checked int32 faces on the current device."""
    global _last_rounds
    dev = faces32.device
    label = torch.arange(Nv, dtype=torch.int32, device=dev)
    rounds = 0
    if Nv and faces32.shape[0]:
        flags = None
        while True:
            if rounds % _FLAGS == 0:
                flags = torch.zeros((_FLAGS,), dtype=torch.int32, device=dev)
            flag = flags[rounds % _FLAGS:]
            _cc_hook(faces32, Nv, label, flag)
            _cc_compress(label)
            rounds += 1
            if not int(flag[0]):                                   # the round's one host read
                break
            if rounds > Nv + 1:                                    # every changed round joins two trees: Nv - 1 at most
                raise RuntimeError("mesh_components: %d rounds on %d vertices" % (rounds, Nv))
    _last_rounds = rounds
    return label, rounds


def _face_labels(faces32, Nv, label):
    Nf = int(faces32.shape[0])
    face_label = torch.empty((Nf,), dtype=torch.int32, device=faces32.device)
    if Nf:
        _lib.call("pf_mesh_face_labels", _lib.ptr(faces32), Nf, Nv, _lib.ptr(label), _lib.ptr(face_label), _lib.stream(),
                  algo_bytes=Nf * 20)
    return face_label


def mesh_components(faces, num_vertices, return_rounds=False):
    """The connected components of the module docstring: ``(vertex_label (Nv,) int32, face_label (Nf,) int32)`` on the
    device of ``faces`` (Nf, 3) int32 or int64, and with ``return_rounds`` the number of rounds.  Synchronises with the
    host once for the index check and once per round.  There is no CPU path."""
    who = "mesh_components"
    Nv, _ = _check_faces(who, faces, num_vertices)
    faces32 = _faces32(who, faces, Nv)
    with _lib.on_device(faces32.device):
        label, rounds = _components(faces32, Nv)
        face_label = _face_labels(faces32, Nv, label)
    return (label, face_label) + ((rounds,) if return_rounds else ())


def component_sizes(face_label):
    """``(labels, face_counts)``, both int64 and sorted by label, of a ``face_label`` (Nf,) integer tensor (plain torch)."""
    if not isinstance(face_label, torch.Tensor) or face_label.dim() != 1 or face_label.dtype.is_floating_point:
        raise ValueError("component_sizes: face_label must be an (Nf,) integer tensor")
    labels, counts = torch.unique(face_label.long(), sorted=True, return_counts=True)
    return labels, counts


def _check_selection(who, min_faces, keep_largest):
    for name, value in (("min_faces", min_faces), ("keep_largest", keep_largest)):
        if value is not None and (isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0):
            raise ValueError("%s: %s must be a non-negative integer or None" % (who, name))


def _check_carried(who, Nv, colours, normals):
    for name, t in (("colours", colours), ("normals", normals)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 2 or int(t.shape[0]) != Nv):
            raise ValueError("%s: %s must be an (Nv, C) tensor" % (who, name))


def _select_faces(face_label, min_faces, keep_largest):
    """``(face_keep (Nf,) bool, number of components)`` by the rule of the module docstring."""
    labels, counts = component_sizes(face_label)
    keep = torch.ones_like(labels, dtype=torch.bool)
    if min_faces is not None:
        keep &= counts >= int(min_faces)
    if keep_largest is not None:
        order = torch.sort(counts, descending=True, stable=True)[1]       # labels ascend: ties go to the smaller label
        among = torch.zeros_like(keep)
        among[order[:int(keep_largest)]] = True
        keep &= among
    if labels.numel() == 0:
        return torch.zeros((0,), dtype=torch.bool, device=face_label.device), 0
    return keep[torch.searchsorted(labels, face_label.long())], int(labels.numel())


def _compact(vertices, faces, face_keep, colours, normals):
    """The kept faces in their order over the vertices they name in their order: ``(vertices, faces, colours, normals,
    vertex_map)``."""
    Nv = int(vertices.shape[0])
    kept = faces[face_keep]
    used = torch.zeros((Nv,), dtype=torch.bool, device=faces.device)
    used[kept.reshape(-1).long()] = True
    vertex_map = torch.where(used, torch.cumsum(used, dim=0, dtype=torch.int64) - 1, torch.full((Nv,), -1, dtype=torch.int64,
                                                                                                device=faces.device))
    new_faces = vertex_map[kept.long()].to(faces.dtype)
    carry = [None if t is None else t.to(faces.device)[used] for t in (colours, normals)]
    return vertices[used], new_faces, carry[0], carry[1], vertex_map


def remove_small_components(vertices, faces, min_faces=None, keep_largest=None, colours=None, normals=None,
                            return_maps=False):
    """Drop the components of the mesh that the module docstring's rule does not keep.  Returns ``(vertices, faces, colours,
    normals)`` -- ``faces`` in the dtype they came in, ``colours`` and ``normals`` (Nv, C) carried or None -- and with
    ``return_maps`` also ``vertex_map`` (Nv,) int64 (old to new, -1 for removed) and ``face_keep`` (Nf,) bool."""
    who = "remove_small_components"
    Nv, _ = _check_mesh(who, vertices, faces)
    _check_selection(who, min_faces, keep_largest)
    _check_carried(who, Nv, colours, normals)
    faces32 = _faces32(who, faces, Nv, vertices)
    with _lib.on_device(faces32.device):
        label, _ = _components(faces32, Nv)
        face_keep, _ = _select_faces(_face_labels(faces32, Nv, label), min_faces, keep_largest)
        v, f, c, n, vertex_map = _compact(vertices, faces, face_keep, colours, normals)
    return (v, f, c, n) + ((vertex_map, face_keep) if return_maps else ())


def vertex_corner_table(faces, num_vertices):
    """``(offsets (Nv + 1,) int64, corners (3 Nf,) int64)``: vertex ``v`` owns the corners ``corners[offsets[v]:offsets[v + 1]]``,
    corner ``3 f + j`` being ``faces[f, j]``, in ascending order.  Plain torch on the device of ``faces`` (CPU tensors work)."""
    who = "vertex_corner_table"
    Nv, _ = _check_faces(who, faces, num_vertices)
    _check_range(who, faces, Nv)
    return _corner_table(faces, Nv)


def _corner_table(faces, Nv):
    flat = faces.reshape(-1).long()
    corners = torch.sort(flat, stable=True)[1]
    offsets = torch.zeros((Nv + 1,), dtype=torch.int64, device=faces.device)
    if Nv:
        offsets[1:] = torch.cumsum(torch.bincount(flat, minlength=Nv), dim=0)
    return offsets, corners


def _vertex_normals(vertices, faces32):
    Nv, Nf = int(vertices.shape[0]), int(faces32.shape[0])
    normals = torch.empty((Nv, 3), dtype=torch.float32, device=vertices.device)
    if Nv:
        offsets, corners = _corner_table(faces32, Nv)
        # per corner its table entry, the face's indices and three vertices; per vertex two offsets and the normal
        _lib.call("pf_mesh_vertex_normals_f32", _lib.ptr(vertices), Nv, _lib.ptr(faces32), Nf, _lib.ptr(offsets),
                  _lib.ptr(corners), _lib.ptr(normals), _lib.stream(), algo_bytes=3 * Nf * (8 + 12 + 36) + Nv * 28)
    return normals


def vertex_normals(vertices, faces):
    """The area-weighted vertex normals of the module docstring: (Nv, 3) float32 on the device of the mesh, unit or
    ``(0, 0, 0)``.  One host synchronisation (the index check).  There is no CPU path."""
    who = "vertex_normals"
    Nv, _ = _check_mesh(who, vertices, faces)
    faces32 = _faces32(who, faces, Nv, vertices)
    with _lib.on_device(faces32.device):
        return _vertex_normals(vertices.contiguous(), faces32)


def _check_sampling(who, pitch, seed):
    """``(inv, seed)``: ``float32(1) / (float32(pitch) * float32(pitch))`` as a Python float."""
    try:
        pitch = float(pitch)
    except (TypeError, ValueError):
        raise ValueError("%s: pitch must be a positive length" % who)
    if not (pitch > 0.0 and math.isfinite(pitch)):
        raise ValueError("%s: pitch must be a positive length" % who)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 32:
        raise ValueError("%s: seed must be an integer in [0, 2^32)" % who)
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / (np.float32(pitch) * np.float32(pitch))
    if not (np.isfinite(inv) and inv > 0):
        raise ValueError("%s: pitch^2 is outside float32" % who)
    return float(inv), int(seed)


def _sample_counts(vertices, faces32, inv, seed):
    Nv, Nf = int(vertices.shape[0]), int(faces32.shape[0])
    count = torch.empty((Nf,), dtype=torch.int32, device=faces32.device)
    if Nf:
        _lib.call("pf_mesh_sample_count_f32", _lib.ptr(vertices), Nv, _lib.ptr(faces32), Nf, inv, seed, _lib.ptr(count),
                  _lib.stream(), algo_bytes=Nf * (12 + 36 + 4))
    return count


def sample_surface(vertices, faces, pitch, seed=0):
    """Sample the mesh's surface by the module docstring, about one sample per ``pitch^2`` of area: ``(points (N, 3)
    float32, face_index (N,) int32, bary (N, 3) float32)`` on the device of the mesh, in ascending face.  Synchronises with
    the host twice (the index check and ``N``).  A total above ``2^31 - 1`` is a ValueError.  There is no CPU path."""
    who = "sample_surface"
    Nv, Nf = _check_mesh(who, vertices, faces)
    inv, seed = _check_sampling(who, pitch, seed)
    faces32 = _faces32(who, faces, Nv, vertices)
    dev = faces32.device
    with _lib.on_device(dev):
        vertices = vertices.contiguous()
        N = 0
        if Nf:
            incl = torch.cumsum(_sample_counts(vertices, faces32, inv, seed), dim=0, dtype=torch.int64)
            N = int(incl[-1])
        if N > MAX_COUNT:
            raise ValueError("%s: %d samples at pitch %g are more than 2^31 - 1" % (who, N, float(pitch)))
        points = torch.empty((N, 3), dtype=torch.float32, device=dev)
        face_index = torch.empty((N,), dtype=torch.int32, device=dev)
        bary = torch.empty((N, 3), dtype=torch.float32, device=dev)
        if N:
            # per sample ~log2(Nf) sums of the search, its face and vertices in, 28 bytes out
            _lib.call("pf_mesh_sample_emit_f32", _lib.ptr(vertices), Nv, _lib.ptr(faces32), Nf, _lib.ptr(incl), N, seed,
                      _lib.ptr(points), _lib.ptr(face_index), _lib.ptr(bary), _lib.stream(),
                      algo_bytes=N * (8 * max(1, Nf.bit_length()) + 48 + 28))
    return points, face_index, bary
