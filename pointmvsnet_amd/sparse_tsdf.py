"""Sparse TSDF volumes on the GPU: the volume of ``tsdf.py`` stored only near the surface, in bricks of 8 x 8 x 8 samples.

``tsdf.TSDFVolume`` keeps 24 bytes of state for every sample of the bounding box, whether or not a surface is near it; at the
pitch DTU is scored at the box no longer fits, and below voxel 0.125 the 49-view scan has more than 2^31 samples.  This
module keeps the same sums on the same grid for the bricks near the surface only (Open3D's ``ScalableTSDFVolume`` is the
model, as for the dense class).  **The specification is ``tsdf.py``'s**, sample for sample; with the allocation rule below the
mesh is the dense mesh bit for bit, which is what tests/test_sparse_tsdf.py compares.  Six HIP kernels
(csrc/sparse_tsdf.hip); the per-view update, the tetrahedra, the edge keys and the vertex arithmetic are the dense kernels'
own device functions (csrc/pf_tsdf.h).

The virtual grid
----------------
``origin``, ``voxel`` and ``dims = (nx, ny, nz)`` are those of ``TSDFVolume``: sample ``(i, j, k)`` sits at
``o + float(i) * voxel`` per coordinate in float32.  Limits, stated on the host: ``nx ny nz < 2^60`` (the dense limit of 2^31
samples is lifted: edge keys are int64 already) and at most 2^20 samples per axis, so that ``float(i)`` is exact.

Bricks
------
Brick ``(bi, bj, bk) = (i >> 3, j >> 3, k >> 3)``; its key is ``(bk NBy + bj) NBx + bi`` as int64 with ``NB* = ceil(n* / 8)``;
there are fewer than 2^31 virtual bricks.  The allocated bricks are **one sorted array of unique keys** and a brick is found
by binary search (the idiom of csrc/pf_cloud_grid.h; this is not a hash table).  State per allocated brick, in key order:
``S`` (Nb, 512) float32, ``W`` (Nb, 512) int32 and, with colour, ``CS`` (Nb, 512, 3) and ``CW`` (Nb, 512) int32; the local
index is ``(lk * 8 + lj) * 8 + li``, x fastest.  ``Nb * 512 <= 2^31 - 1``; more is a ValueError that names the brick count.
Samples of an edge brick that lie outside ``dims`` are never integrated: they stay zero, so ``W = 0``.

Allocation
----------
A sample is a *band sample* of a set of views if some view reaches step 6 of the dense integration with
``|sdf| <= trunc`` (in the dense volume with colour: ``CW > 0``).  ``L`` is the set of bricks that hold a sample within
Chebyshev distance 1 (in samples) of a band sample.  ``allocate(depths, K, E)`` allocates a set ``A`` with ``L <= A <= U``,
where ``U`` is the brick test below evaluated in float64 with doubled slack: the box grown by two samples per side, the
pixel box padded by two pixels, the z-interval widened by ``trunc (1 + 2^-10)`` and the closeness guard at an eighth of a
pixel.

The brick test, per virtual brick and view, in float32 (``pf_sparse_tsdf_touch``; eps = 2^-24):

1. Grow the brick's box by one sample per side: ``i`` from ``8 bi - 1`` to ``8 bi + 8``, positions by the grid's own
   expression.  Project its 8 corners with the dense kernel's expressions for ``qx, qy, z``; ``zlo, zhi`` are the extremes
   of ``z``.  ``Az`` is the largest ``|p8 X| + |p9 Y| + |p10 Z| + |p11|`` over the corners, ``Aq`` the same for rows 0 and 1,
   and ``m = 2^-20 (Az + trunc)`` = 16 eps of everything that is added in this test.
2. Skip the view if ``zhi + m <= depth_min`` or ``zlo - m >= depth_max``.
3. The pixel box is the whole image if ``zlo - m <= depth_min`` (some corner is at or behind the camera plane), or if
   ``2^-20 (Aq + max(w, h) Az) >= zlo / 4`` (so close to it that a rounding could move a projection by a quarter pixel).
   Otherwise it is the bounding box of the corners' ``floor(qx / z), floor(qy / z)`` padded by one pixel and clipped.
4. The brick is touched if a pixel of the box has ``depth_min < d < depth_max`` and
   ``(zlo - trunc) - m <= d <= (zhi + trunc) + m``.

Why ``A`` contains ``L``.  Let ``b`` be a band sample of view ``v`` within Chebyshev distance 1 of a sample of the brick:
its float32 position lies in the grown box, because ``o + float(i) * voxel`` is monotone in ``i``.  *Linearity for z*: in
exact arithmetic ``z`` is an affine function, so ``z(b)`` lies between the corners' extremes; the dense kernel's float32
``z(b)`` and the corners' float32 values each differ from the exact ones by at most ``4 eps Az``, ``sdf = d - z`` rounds once
and the two bounds of step 4 round twice each, in all fewer than the ``16 eps (Az + trunc)`` of ``m``; ``|sdf| <= trunc`` and
``z > depth_min`` therefore give step 4's interval and survive step 2.  *Convexity for the pixel box*: when all corners are
in front of the camera the perspective map takes the box into the convex hull of the corners' projections, so ``b``'s exact
projection lies in their bounding box; step 3's guard bounds every rounding of a projection that lands in the image by a
quarter pixel, so the pixel ``(floor(u), floor(w_))`` that the dense kernel reads for ``b`` is at most one pixel outside the
corners' floored box.  That pixel holds the ``d`` of step 4, so the brick is touched.

``allocate`` may be called any number of times before the first ``integrate`` and the calls accumulate; an ``integrate``
on a volume without an allocation first allocates for its own views; ``allocate`` after an ``integrate`` is a ValueError
(a brick allocated late would lack the earlier views' free-space counts).

Integration
-----------
Per sample of an allocated brick inside ``dims``, steps 1-6 of ``tsdf.py`` in ascending view order, by the same device
function (``tsdf_integrate_view``).  So on every allocated sample ``S, W, CS, CW`` are the dense volume's bits, and
``allocate(all)``, ``integrate(0..2)``, ``integrate(3..4)`` gives the bits of ``integrate(0..4)``.

Extraction
----------
Cells are owned by the brick of their corner 0.  A corner in a brick that is not allocated, or outside ``dims``, counts as
weight 0; ``min_weight >= 1`` is required (``min_weight <= 0`` is a ValueError: an absent corner cannot be "seen").  Edge
keys are the **dense** keys ``((k ny + j) nx + i) * 8 + dirbits`` on the virtual grid; vertices are computed from the key
alone and come in ascending key; tetrahedra, cases and winding are the dense ones.  **Faces come in ascending brick key,
then cell-in-brick index ``(lk * 8 + lj) * 8 + li``, then tetrahedron, then triangle: this order differs from the dense
one.**

The equality claim.  A cell that emits a triangle in the dense volume has a corner with ``tsdf < 0``.  That corner
received a negative ``sdf >= -trunc`` from some view, so it is a band sample.  All 8 corners of the cell are within
Chebyshev distance 1 of it, so their bricks are in ``L``, hence allocated, and carry the dense bits; the sparse volume
emits the same triangles with the same keys.  Conversely a cell with a corner that is not allocated has no band corner,
hence no negative corner, and the dense volume emits nothing for it.  Therefore, for ``min_weight >= 1``, ``vertices``,
``colours`` and ``keys`` equal the dense ones byte for byte and the face lists are equal as multisets of rows.

The route: touch, ``torch.nonzero`` of the flags (plumbing, as ``camera_maps.compact``), the neighbour table, the
integration; then as in ``tsdf.extract_mesh``: count, ``torch.cumsum``, emit, ``torch.unique``, vertices.

Out of scope
------------
Brick sizes other than 8; de-integration; freeing bricks; per-brick view culling in the integration; a coarse-to-fine touch
pass; trilinear sampling; hashing.
"""
import math

import torch

from . import _lib, camera_maps as cm
from .render import _world_maps
from .tsdf import MAX_VIEWS, MAX_VIEWS_COLOUR, _check_depth_range, _check_grid

_WHO = "SparseTSDFVolume"
BRICK, BRICK_SAMPLES = 8, 512
MAX_VIRTUAL_SAMPLES = 2 ** 60 - 1
MAX_AXIS = 2 ** 20                                 # PF_SPARSE_TSDF_MAX_AXIS of include/pointflow_hip.h
MAX_BRICKS = (2 ** 31 - 1) // BRICK_SAMPLES


class SparseTSDFVolume(object):
    """The volume of the module docstring on ``device``.  ``allocate(...)`` any number of times, ``integrate(...)`` any number
    of times; then the accessors and ``extract(min_weight)``.  Arguments are checked before a GPU is needed; there is no
    CPU path."""

    def __init__(self, origin, voxel, dims, trunc, with_colour=False, device="cuda"):
        self.origin, self.voxel, self.dims = _check_grid(_WHO, origin, voxel, dims, MAX_VIRTUAL_SAMPLES)
        if max(self.dims) > MAX_AXIS:
            raise ValueError("%s: %d x %d x %d samples; an axis has at most 2^20" % ((_WHO,) + self.dims))
        self.bricks = tuple((n + BRICK - 1) // BRICK for n in self.dims)
        self.virtual_bricks = self.bricks[0] * self.bricks[1] * self.bricks[2]
        if self.virtual_bricks > 2 ** 31 - 1:
            raise ValueError("%s: %d virtual bricks; a volume has fewer than 2^31" % (_WHO, self.virtual_bricks))
        self.trunc = float(trunc)
        if not (self.trunc > 0.0 and math.isfinite(self.trunc)):
            raise ValueError("%s: trunc must be a positive length" % _WHO)
        self.with_colour = bool(with_colour)
        self.device = torch.device(device)
        self.views = 0                                   # integrated so far: the host's bound on every W and CW
        self._touched = None                             # one byte per virtual brick until the first integrate
        self._keys = self._rows = None                   # after it: the sorted keys and the neighbour table
        self.S = self.W = self.CS = self.CW = None

    # ---- allocation -------------------------------------------------------------------------------------------------
    def _inputs(self, who, depths, intrinsics, extrinsics, images, depth_min, depth_max):
        depths = cm.stack_depths(who, depths, 1)
        V = int(depths.shape[0])
        cams = cm.decompose(who, intrinsics, extrinsics, V)            # bad arguments are reported before a missing GPU
        depth_min, depth_max = _check_depth_range(who, depth_min, depth_max)
        return depths, V, cams, depth_min, depth_max

    def _on_device(self, who, depths, images):
        depths, images, V, h, w, dev = cm.normalise_inputs(who, depths, images, 1)
        if h * w > (2 ** 31 - 1) // 4:
            raise ValueError("%s: maps of %d x %d are outside what the kernel is built for" % (who, h, w))
        if dev != self.device and not (dev.type == self.device.type and self.device.index is None):
            raise ValueError("%s: the depth maps are on %s, the volume on %s" % (who, dev, self.device))
        self.device = dev
        return depths, images, V, h, w, dev

    def _touch(self, depths, cams, V, h, w, depth_min, depth_max):
        if self._touched is None:
            self._touched = torch.zeros((self.virtual_bricks,), dtype=torch.uint8, device=self.device)
        if V and h and w:
            proj = torch.from_numpy(_world_maps(cams)).to(self.device)
            # per brick and view: the 12 floats, and at least one pixel box of depths (a lower bound: 4 bytes)
            _lib.call("pf_sparse_tsdf_touch", _lib.ptr(depths), _lib.ptr(proj), V, h, w, self.origin[0], self.origin[1],
                      self.origin[2], self.voxel, self.dims[0], self.dims[1], self.dims[2], self.trunc, depth_min, depth_max,
                      _lib.ptr(self._touched), _lib.stream(), algo_bytes=self.virtual_bricks * (1 + 4 * V))

    def allocate(self, depths, intrinsics, extrinsics, depth_min=1e-3, depth_max=1e5):
        """Allocate the bricks near the surfaces of ``depths`` (V, h, w) seen by the cameras, by the module docstring's
        brick test; the calls before the first ``integrate`` accumulate.  Returns the volume."""
        who = _WHO + ".allocate"
        depths, V, cams, depth_min, depth_max = self._inputs(who, depths, intrinsics, extrinsics, None, depth_min, depth_max)
        if self._keys is not None:
            raise ValueError("%s: the volume has been integrated into; a brick allocated now would lack the earlier views' "
                             "free-space counts" % who)
        depths, _, V, h, w, dev = self._on_device(who, depths, None)
        with _lib.on_device(dev):
            self._touch(depths, cams, V, h, w, depth_min, depth_max)
        return self

    def _current_keys(self):
        if self._keys is not None:
            return self._keys
        if self._touched is None:
            return torch.zeros((0,), dtype=torch.int64, device=self.device)
        return torch.nonzero(self._touched).view(-1)                                # ascending: sorted and unique

    def _freeze(self):
        """The first call that needs the state: flags -> sorted keys, the neighbour table and zeroed sums."""
        if self._keys is not None:
            return
        keys = self._current_keys()
        nb = int(keys.numel())
        if nb > MAX_BRICKS:
            raise ValueError("%s: %d bricks are allocated; the state addresses at most %d (2^31 - 1 samples)" %
                             (_WHO, nb, MAX_BRICKS))
        _lib.require_gpu(keys)
        dev = self.device
        self._keys, self._touched = keys.contiguous(), None
        self._rows = torch.empty((nb, 7), dtype=torch.int32, device=dev)
        if nb:
            _lib.call("pf_sparse_tsdf_neighbours", _lib.ptr(self._keys), nb, self.dims[0], self.dims[1], self.dims[2],
                      _lib.ptr(self._rows), _lib.stream(), algo_bytes=nb * (8 + 28))
        self.S = torch.zeros((nb, BRICK_SAMPLES), dtype=torch.float32, device=dev)
        self.W = torch.zeros((nb, BRICK_SAMPLES), dtype=torch.int32, device=dev)
        if self.with_colour:
            self.CS = torch.zeros((nb, BRICK_SAMPLES, 3), dtype=torch.int32, device=dev)
            self.CW = torch.zeros((nb, BRICK_SAMPLES), dtype=torch.int32, device=dev)

    # ---- integration ------------------------------------------------------------------------------------------------
    def integrate(self, depths, intrinsics, extrinsics, images=None, depth_min=1e-3, depth_max=1e5):
        """``TSDFVolume.integrate`` on the allocated bricks; a volume without an allocation first allocates for these
        views.  Returns the volume."""
        who = _WHO + ".integrate"
        depths, V, cams, depth_min, depth_max = self._inputs(who, depths, intrinsics, extrinsics, images, depth_min, depth_max)
        if (images is not None) != self.with_colour:
            raise ValueError("%s: a volume with_colour needs images, a volume without takes none" % who)
        if self.views + V > (MAX_VIEWS_COLOUR if self.with_colour else MAX_VIEWS):
            raise ValueError("%s: %d views after %d would overflow the volume's int32 sums" % (who, V, self.views))
        depths, images, V, h, w, dev = self._on_device(who, depths, images)
        with _lib.on_device(dev):
            if self._keys is None and self._touched is None:
                self._touch(depths, cams, V, h, w, depth_min, depth_max)
            self._freeze()
            nb = int(self._keys.numel())
            if nb and V and h and w:
                proj = torch.from_numpy(_world_maps(cams)).to(dev)
                n = nb * BRICK_SAMPLES
                _lib.call("pf_sparse_tsdf_integrate_f32", _lib.ptr(self._keys), nb, _lib.ptr(depths), _lib.ptr(images),
                          _lib.ptr(proj), V, h, w, self.origin[0], self.origin[1], self.origin[2], self.voxel, self.dims[0],
                          self.dims[1], self.dims[2], self.trunc, depth_min, depth_max, _lib.ptr(self.S), _lib.ptr(self.W),
                          _lib.ptr(self.CS), _lib.ptr(self.CW), _lib.stream(),
                          algo_bytes=n * ((48 if self.with_colour else 16) + V * (7 if self.with_colour else 4)))
        self.views += V
        return self

    # ---- accessors --------------------------------------------------------------------------------------------------
    def _state(self):
        with _lib.on_device(self.device):
            self._freeze()
        return self.S, self.W, self.CS, self.CW

    def brick_keys(self):
        """The allocated bricks' keys (Nb,) int64, ascending."""
        return self._current_keys()

    def brick_coords(self):
        """``(bi, bj, bk)`` of the allocated bricks, (Nb, 3) int64, in key order."""
        keys = self._current_keys()
        nbx, nby = self.bricks[0], self.bricks[1]
        return torch.stack([keys % nbx, torch.div(keys, nbx, rounding_mode="floor") % nby,
                            torch.div(keys, nbx * nby, rounding_mode="floor")], dim=1)

    def _bricked(self, a):
        return a.view((a.shape[0], BRICK, BRICK, BRICK) + tuple(a.shape[2:]))

    def _tsdf(self):
        S, W = self._state()[:2]
        return torch.where(W > 0, S / W.to(torch.float32), torch.ones_like(S))

    def _colour(self):
        CS, CW = self._state()[2:]
        cw = CW.to(torch.int64).unsqueeze(-1)
        mean = torch.div(2 * CS.to(torch.int64) + cw, 2 * cw.clamp(min=1), rounding_mode="floor")
        return torch.where(cw > 0, mean, torch.zeros_like(mean)).to(torch.uint8)

    def tsdf(self):
        """``S / W`` in float32 (Nb, 8, 8, 8) indexed ``[brick, lk, lj, li]``, 1.0 where ``W == 0``."""
        return self._bricked(self._tsdf())

    def weight(self):
        """``W`` (Nb, 8, 8, 8) int32."""
        return self._bricked(self._state()[1])

    def colour(self):
        """``(2 CS + CW) // (2 CW)`` (Nb, 8, 8, 8, 3) uint8, 0 where ``CW == 0``; None for a volume without colour."""
        return self._bricked(self._colour()) if self.with_colour else None

    def to_dense(self):
        """``(S, W, CS, CW)`` scattered into dense ``(nz, ny, nx[, 3])`` arrays, zero where no brick is allocated (``CS`` and
        ``CW`` None without colour).  For tests and small volumes: a ValueError above 2^31 samples."""
        nx, ny, nz = self.dims
        if nx * ny * nz > 2 ** 31 - 1:
            raise ValueError("%s.to_dense: %d x %d x %d samples; a dense volume has fewer than 2^31" % ((_WHO,) + self.dims))
        S, W, CS, CW = self._state()
        dev = S.device
        local = torch.arange(BRICK, device=dev)
        coords = self.brick_coords() * BRICK
        i = (coords[:, 0, None] + local)[:, None, None, :].expand(-1, BRICK, BRICK, BRICK)
        j = (coords[:, 1, None] + local)[:, None, :, None].expand(-1, BRICK, BRICK, BRICK)
        k = (coords[:, 2, None] + local)[:, :, None, None].expand(-1, BRICK, BRICK, BRICK)
        inside = ((i < nx) & (j < ny) & (k < nz)).reshape(-1)
        at = ((k * ny + j) * nx + i).reshape(-1)[inside]
        out = []
        for a in (S, W, CS, CW):
            if a is None:
                out.append(None)
                continue
            dense = torch.zeros((nz * ny * nx,) + tuple(a.shape[2:]), dtype=a.dtype, device=dev)
            dense[at] = a.reshape((-1,) + tuple(a.shape[2:]))[inside]
            out.append(dense.view((nz, ny, nx) + tuple(a.shape[2:])))
        return tuple(out)

    def report(self):
        """``{"virtual_bricks", "allocated_bricks", "state_bytes", "dense_state_bytes"}``: the state is 8 (with colour 24)
        bytes per sample of an allocated brick, the dense figure the same per sample of the grid."""
        nb = 0 if self._keys is None and self._touched is None else int(self._current_keys().numel())
        per = 24 if self.with_colour else 8
        return {"virtual_bricks": self.virtual_bricks, "allocated_bricks": nb, "state_bytes": nb * BRICK_SAMPLES * per,
                "dense_state_bytes": self.dims[0] * self.dims[1] * self.dims[2] * per}

    # ---- extraction -------------------------------------------------------------------------------------------------
    def extract(self, min_weight=1):
        """Marching tetrahedra by the module docstring: ``(vertices (Nv, 3) float32, faces (Nf, 3) int32, colours (Nv, 3)
        uint8 or None, keys (Nv,) int64)``.  Synchronises with the host twice, as ``tsdf.extract_mesh``."""
        who = _WHO + ".extract"
        if isinstance(min_weight, bool) or int(min_weight) != min_weight or not -2 ** 31 <= int(min_weight) < 2 ** 31:
            raise ValueError("%s: min_weight must be an integer" % who)
        if int(min_weight) < 1:
            raise ValueError("%s: min_weight must be at least 1: a corner in a brick that is not allocated has not been seen"
                             % who)
        min_weight = int(min_weight)
        dev = self.device
        nx, ny, nz = self.dims
        with _lib.on_device(dev):
            self._freeze()
            nb = int(self._keys.numel())
            cells = nb * BRICK_SAMPLES
            tsdf, weight = self._tsdf(), self.W
            colour = self._colour() if self.with_colour else None
            faces_n = 0
            if cells:
                count = torch.empty((cells,), dtype=torch.int32, device=dev)
                _lib.call("pf_sparse_tsdf_count_triangles", _lib.ptr(tsdf), _lib.ptr(weight), _lib.ptr(self._rows), nb,
                          min_weight, _lib.ptr(count), _lib.stream(), algo_bytes=12 * cells)
                incl = torch.cumsum(count, dim=0, dtype=torch.int64)               # plumbing, as camera_maps.compact
                faces_n = int(incl[-1])
            if faces_n > (2 ** 31 - 1) // 3:
                raise ValueError("%s: %d faces are more than int32 indices address" % (who, faces_n))
            tri_keys = torch.empty((faces_n, 3), dtype=torch.int64, device=dev)
            if faces_n:
                _lib.call("pf_sparse_tsdf_emit_triangles", _lib.ptr(self._keys), nb, _lib.ptr(tsdf), _lib.ptr(weight),
                          _lib.ptr(self._rows), nx, ny, nz, min_weight, _lib.ptr(incl), faces_n, _lib.ptr(tri_keys),
                          _lib.stream(), algo_bytes=20 * cells + 24 * faces_n)
            keys, rank = torch.unique(tri_keys.view(-1), sorted=True, return_inverse=True)   # plumbing: sorted keys, ranks
            faces = rank.view(faces_n, 3).to(torch.int32)
            nv = int(keys.numel())
            vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
            colours = torch.empty((nv, 3), dtype=torch.uint8, device=dev) if colour is not None else None
            if nv:
                _lib.call("pf_sparse_tsdf_vertices_f32", _lib.ptr(keys), nv, _lib.ptr(self._keys), nb, _lib.ptr(tsdf),
                          _lib.ptr(colour), self.origin[0], self.origin[1], self.origin[2], self.voxel, nx, ny, nz,
                          _lib.ptr(vertices), _lib.ptr(colours), _lib.stream(),
                          algo_bytes=nv * (8 + 8 + 12 + (9 if colour is not None else 0)))
        return vertices, faces, colours, keys
