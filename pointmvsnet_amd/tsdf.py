"""Meshing a scan on the GPU: volumetric fusion of the depth maps (a truncated signed distance field) and the extraction
of its zero surface by marching tetrahedra.

The fusers (``fusion.py``, ``geometric.py``) turn depth maps into points; ``normals.py`` orients them because meshing
expects that; nothing so far produced a surface.  This module is the classical alternative to point fusion (KinectFusion,
Open3D's ``ScalableTSDFVolume``): every sample of a regular grid averages, over the views that see it, its signed distance
to the surface along the view's optical axis, and the surface is where that average changes sign.  The reference has no
such step, so **the specification below is this project's own**; parity with Open3D or KinectFusion is neither claimed nor
tested.  It runs as four HIP kernels (csrc/tsdf.hip).  The library is built with ``-ffp-contract=off``, so "float32 in this
order" is meant literally.  Pixel centres are at ``(x + 0.5, y + 0.5)``, as everywhere else in this pipeline, so the pixel
that contains an image position ``(u, w_)`` is ``(floor(u), floor(w_))``.

The volume
----------
``dims = (nx, ny, nz)`` samples; sample ``(i, j, k)`` sits at ``origin + voxel * (i, j, k)``, evaluated per coordinate in
float32 as ``o + float(i) * voxel``.  The state is indexed ``[k, j, i]`` (x fastest): ``S`` (nz, ny, nx) float32, ``W``
(nz, ny, nx) int32 and, with colour, ``CS`` (nz, ny, nx, 3) int32 and ``CW`` (nz, ny, nx) int32, all zero at first.
Limits, stated on the host: ``voxel > 0``, ``trunc > 0``, ``nx ny nz < 2^31``, and the number of views ever integrated
into one volume is at most ``2^31 - 1`` (with colour ``(2^31 - 1) // 255``), so that neither ``W`` nor ``CS`` overflows.

Integration
-----------
``proj[v] = K_v [R_v | t_v]`` (3 x 4, row-major ``p0 .. p11``) is composed in float64 and handed over as float32
(``render.world_maps``).  Per sample ``(X, Y, Z)`` and view ``v``, in **ascending** ``v``, in float32 with exactly this
operation order:

1. ``qx = ((p0 X + p1 Y) + p2 Z) + p3``, ``qy`` and ``z`` likewise from rows 1 and 2 (steps 1-2 of ``render.py``).  Skip
   the view unless ``depth_min < z < depth_max``.  This is false for NaN.
2. ``u = qx / z``, ``w_ = qy / z``, ``(x, y) = (floor(u), floor(w_))``.  Skip unless ``0 <= u < w`` and ``0 <= w_ < h``: the
   pixel that contains the projection, no interpolation, the choice ``fusion.py`` makes.
3. ``d = depths[v, y, x]``.  Skip unless ``depth_min < d < depth_max``.
4. ``sdf = d - z``: projective, along the optical axis.  Skip if ``sdf < -trunc`` (the sample is behind the surface).
5. ``S += fminf(sdf, trunc) / trunc``; ``W += 1``.
6. With images, and if ``fabsf(sdf) <= trunc``: ``CS += rgb(v, y, x)`` as integers, ``CW += 1``.

A sample is owned by one thread: no atomics, and the sum has one order.  ``integrate`` continues the sums that are there,
so integrating views ``0..2`` and then ``3..4`` gives the bits of integrating ``0..4`` at once, and two runs give identical
bytes.  ``tsdf() = S / W`` in float32, ``1.0`` where ``W == 0``; ``weight() = W``; ``colour() = (2 CS + CW) // (2 CW)`` as
uint8 (the mean, rounded half up), 0 where ``CW == 0``.

Extraction
----------
``extract_mesh(tsdf, weight, origin, voxel, min_weight=1, colour=None)``.

Cells and corners.  A sample is *inside* iff ``tsdf < 0``; exactly 0 (and NaN) is outside.  Cell ``(i, j, k)`` with
``i < nx-1``, ``j < ny-1``, ``k < nz-1`` is *active* iff all 8 corners have ``weight >= min_weight``.  Corner
``c = dx + 2 dy + 4 dz``.  Every active cell is cut into six tetrahedra (the Kuhn decomposition), in this order:
``(0,1,3,7) (0,3,2,7) (0,2,6,7) (0,6,4,7) (0,4,5,7) (0,5,1,7)``.  Every cube is cut the same way, so neighbouring cubes
agree on every shared face and the surface is closed wherever the active cells are.

Edges and vertices.  Every tetrahedron edge runs from a sample ``a`` to ``a + (dx, dy, dz)`` with direction bits
``dirbits = dx + 2 dy + 4 dz`` in ``1..7``; its key is ``((k ny + j) nx + i) * 8 + dirbits`` of the lower end ``a``, an
int64.  A mesh vertex lies on an edge whose ends differ in insideness.  It is computed **from the key alone**, so every
cell that refers to it sees the same bits: ``t = f_a / (f_a - f_b)``, position ``p_a + t * (p_b - p_a)`` per coordinate in
float32 with ``p`` as above; colour ``floor(c_a + t * (c_b - c_a) + 0.5)`` clamped to uint8.

Triangles.  ``P`` are a tetrahedron's inside corners and ``Q`` its outside ones, each in the tetrahedron's listed order.

* ``|P| = 1``: one triangle on the edges ``(P0,Q0) (P0,Q1) (P0,Q2)``.
* ``|Q| = 1``: one triangle on the edges ``(P0,Q0) (P1,Q0) (P2,Q0)``.
* ``|P| = |Q| = 2``: the quad ``e0..e3 = (P0,Q0) (P0,Q1) (P1,Q1) (P1,Q0)`` as the triangles ``(e0,e1,e2)`` then
  ``(e0,e2,e3)``.

Winding.  Fixed per (tetrahedron, case): take the triangle through the edge *midpoints in index space*; its right-hand
normal must have a positive dot product with ``mean(Q) - mean(P)``, and if it does not the last two vertices are swapped.
So normals point from inside to outside, towards the cameras.

Order.  Faces come in ascending cell index ``(k (ny-1) + j)(nx-1) + i``, then tetrahedron, then triangle; the rotation of
a face's three indices is free.  Vertices come in ascending key.  Zero-area triangles arise when ``f_b == 0``; they are
kept, so the surface stays combinatorially closed.

Returns ``vertices`` (Nv, 3) float32, ``faces`` (Nf, 3) int32, ``colours`` (Nv, 3) uint8 or None, ``keys`` (Nv,) int64.
The route: a count kernel per cell, ``torch.cumsum`` (as ``camera_maps.compact``), an emit kernel writing three keys per
triangle, the sorted unique keys and their ranks by ``torch.unique`` (plumbing, as in the cloud cleaners), and a vertex
kernel over the keys.

Out of scope
------------
Hashed volumes (a volume stored only near the surface, in bricks found by binary search, is ``sparse_tsdf.py``: the same
specification and, for ``min_weight >= 1``, the same mesh byte for byte); per-axis voxel sizes; weighting by angle or confidence; de-integration; trilinear depth
sampling; vertex normals from the TSDF gradient; mesh smoothing; Poisson reconstruction.  (Looking at
the mesh from a camera is ``render.render_mesh_depth_maps``; dropping its small components, area-weighted vertex normals
and samples of its surface are ``mesh_ops.py``; simplifying it is ``mesh_simplify.py``.)
"""
import math

import numpy as np
import torch

from . import _lib, camera_maps as cm
from .render import _world_maps

_WHO = "TSDFVolume"
MAX_SAMPLES = 2 ** 31 - 1                      # PF_TSDF_MAX_SAMPLES of include/pointflow_hip.h
MAX_VIEWS, MAX_VIEWS_COLOUR = 2 ** 31 - 1, (2 ** 31 - 1) // 255


def _check_grid(who, origin, voxel, dims, max_samples=MAX_SAMPLES):
    """``((ox, oy, oz), voxel, (nx, ny, nz))`` as Python numbers, or the ValueError of ``who``.  ``max_samples`` is the dense
    volume's limit unless the caller states another (``sparse_tsdf.py``: its grid is virtual)."""
    try:
        origin = tuple(float(o) for o in np.asarray(cm.host_f64(origin)).reshape(-1))
        dims_f = tuple(float(d) for d in np.asarray(dims).reshape(-1))
    except (TypeError, ValueError):
        raise ValueError("%s: origin must be three numbers and dims three integers" % who)
    if len(origin) != 3 or not all(math.isfinite(o) for o in origin):
        raise ValueError("%s: origin must be three finite numbers" % who)
    if len(dims_f) != 3 or any(d != int(d) or d < 1 for d in dims_f):
        raise ValueError("%s: dims must be three integers (nx, ny, nz) of at least 1" % who)
    dims = tuple(int(d) for d in dims_f)
    if dims[0] * dims[1] * dims[2] > max_samples:
        raise ValueError("%s: %d x %d x %d samples; a volume has fewer than 2^%d" %
                         ((who,) + dims + ((max_samples + 1).bit_length() - 1,)))
    voxel = float(voxel)
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError("%s: voxel must be a positive length" % who)
    return origin, voxel, dims


def _check_depth_range(who, depth_min, depth_max):
    depth_min, depth_max = float(depth_min), float(depth_max)
    if not 0.0 <= depth_min < depth_max:
        raise ValueError("%s: need 0 <= depth_min < depth_max" % who)
    return depth_min, depth_max


class TSDFVolume(object):
    """The volume of the module docstring on ``device``.  ``integrate(...)`` any number of times; then ``tsdf()``,
    ``weight()``, ``colour()`` and ``extract(min_weight)``.  Arguments are checked before a GPU is needed; the state is
    allocated by the first call that needs it.  There is no CPU path."""

    def __init__(self, origin, voxel, dims, trunc, with_colour=False, device="cuda"):
        self.origin, self.voxel, self.dims = _check_grid(_WHO, origin, voxel, dims)
        self.trunc = float(trunc)
        if not (self.trunc > 0.0 and math.isfinite(self.trunc)):
            raise ValueError("%s: trunc must be a positive length" % _WHO)
        self.with_colour = bool(with_colour)
        self.device = torch.device(device)
        self.views = 0                                   # integrated so far: the host's bound on every W and CW
        self.S = self.W = self.CS = self.CW = None

    def _state(self):
        if self.S is None:
            nx, ny, nz = self.dims
            with _lib.on_device(self.device):
                self.S = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
                self.W = torch.zeros((nz, ny, nx), dtype=torch.int32, device=self.device)
                if self.with_colour:
                    self.CS = torch.zeros((nz, ny, nx, 3), dtype=torch.int32, device=self.device)
                    self.CW = torch.zeros((nz, ny, nx), dtype=torch.int32, device=self.device)
        return self.S, self.W, self.CS, self.CW

    def integrate(self, depths, intrinsics, extrinsics, images=None, depth_min=1e-3, depth_max=1e5):
        """Integrate ``depths`` (V, h, w) float32 on the volume's GPU (0 = no depth; a sequence of (h, w) maps is stacked)
        with cameras ``intrinsics`` (V, 3, 3, of that grid) and ``extrinsics`` (V, 3, 4) or (V, 4, 4) in one launch, by the
        module docstring.  A volume ``with_colour`` needs ``images`` (V, h, w, 3) uint8, any other takes none.  Works on
        the current stream without a host synchronisation; returns the volume."""
        who = _WHO + ".integrate"
        depths = cm.stack_depths(who, depths, 1)
        V = int(depths.shape[0])
        cams = cm.decompose(who, intrinsics, extrinsics, V)            # bad arguments are reported before a missing GPU
        depth_min, depth_max = _check_depth_range(who, depth_min, depth_max)
        if (images is not None) != self.with_colour:
            raise ValueError("%s: a volume with_colour needs images, a volume without takes none" % who)
        if self.views + V > (MAX_VIEWS_COLOUR if self.with_colour else MAX_VIEWS):
            raise ValueError("%s: %d views after %d would overflow the volume's int32 sums" % (who, V, self.views))
        depths, images, V, h, w, dev = cm.normalise_inputs(who, depths, images, 1)
        if h * w > (2 ** 31 - 1) // 4:
            raise ValueError("%s: maps of %d x %d are outside what the kernel is built for" % (who, h, w))
        if dev != self.device and not (dev.type == self.device.type and self.device.index is None):
            raise ValueError("%s: the depth maps are on %s, the volume on %s" % (who, dev, self.device))
        self.device = dev
        with _lib.on_device(dev):
            S, W, CS, CW = self._state()
            if V and h and w:
                proj = torch.from_numpy(_world_maps(cams)).to(dev)
                n = self.dims[0] * self.dims[1] * self.dims[2]
                # per sample: its sums in and out; per sample-view that reads a depth (an upper bound: all of them) 4 bytes
                _lib.call("pf_tsdf_integrate_f32", _lib.ptr(depths), _lib.ptr(images), _lib.ptr(proj), V, h, w,
                          self.origin[0], self.origin[1], self.origin[2], self.voxel, self.dims[0], self.dims[1], self.dims[2],
                          self.trunc, depth_min, depth_max, _lib.ptr(S), _lib.ptr(W), _lib.ptr(CS), _lib.ptr(CW), _lib.stream(),
                          algo_bytes=n * ((48 if self.with_colour else 16) + V * (7 if self.with_colour else 4)))
        self.views += V
        return self

    def tsdf(self):
        """``S / W`` in float32 (nz, ny, nx), 1.0 where ``W == 0``."""
        S, W = self._state()[:2]
        return torch.where(W > 0, S / W.to(torch.float32), torch.ones_like(S))

    def weight(self):
        """``W`` (nz, ny, nx) int32: the views that reached step 5 at each sample."""
        return self._state()[1]

    def colour(self):
        """``(2 CS + CW) // (2 CW)`` (nz, ny, nx, 3) uint8, 0 where ``CW == 0``; None for a volume without colour."""
        if not self.with_colour:
            return None
        CS, CW = self._state()[2:]
        cw = CW.to(torch.int64).unsqueeze(-1)
        mean = torch.div(2 * CS.to(torch.int64) + cw, 2 * cw.clamp(min=1), rounding_mode="floor")
        return torch.where(cw > 0, mean, torch.zeros_like(mean)).to(torch.uint8)

    def extract(self, min_weight=1):
        """``extract_mesh`` of this volume: ``(vertices, faces, colours, keys)``."""
        return extract_mesh(self.tsdf(), self.weight(), self.origin, self.voxel, min_weight, self.colour())


def extract_mesh(tsdf, weight, origin, voxel, min_weight=1, colour=None):
    """Marching tetrahedra by the module docstring on ``tsdf`` (nz, ny, nx) float32 and ``weight`` (nz, ny, nx) int32 on
    one GPU, optionally ``colour`` (nz, ny, nx, 3) uint8.

    Returns ``(vertices (Nv, 3) float32, faces (Nf, 3) int32, colours (Nv, 3) uint8 or None, keys (Nv,) int64)`` on that
    device.  Synchronises with the host twice (the numbers of faces and of vertices).  There is no CPU path."""
    who = "extract_mesh"
    if not isinstance(tsdf, torch.Tensor) or not isinstance(weight, torch.Tensor) or tsdf.dim() != 3 or \
            tsdf.dtype != torch.float32 or weight.shape != tsdf.shape or weight.dtype != torch.int32:
        raise ValueError("%s: tsdf must be (nz, ny, nx) float32 and weight int32 of the same shape" % who)
    nz, ny, nx = (int(s) for s in tsdf.shape)
    origin, voxel, _ = _check_grid(who, origin, voxel, (max(nx, 1), max(ny, 1), max(nz, 1)))
    if min(nx, ny, nz) < 1:
        raise ValueError("%s: an empty volume" % who)
    if isinstance(min_weight, bool) or int(min_weight) != min_weight or not -2 ** 31 <= int(min_weight) < 2 ** 31:
        raise ValueError("%s: min_weight must be an integer" % who)
    if colour is not None and (not isinstance(colour, torch.Tensor) or tuple(colour.shape) != (nz, ny, nx, 3) or
                               colour.dtype != torch.uint8):
        raise ValueError("%s: colour must be (nz, ny, nx, 3) uint8" % who)
    _lib.require_gpu(tsdf, weight, colour)
    dev = tsdf.device
    if weight.device != dev or (colour is not None and colour.device != dev):
        raise ValueError("%s: tsdf, weight and colour must be on one device" % who)
    cells = (nx - 1) * (ny - 1) * (nz - 1)
    with _lib.on_device(dev):
        tsdf, weight = tsdf.contiguous(), weight.contiguous()
        colour = None if colour is None else colour.contiguous()
        faces_n = 0
        if cells:
            count = torch.empty((cells,), dtype=torch.int32, device=dev)
            _lib.call("pf_tsdf_count_triangles", _lib.ptr(tsdf), _lib.ptr(weight), nx, ny, nz, int(min_weight), _lib.ptr(count),
                      _lib.stream(), algo_bytes=12 * cells)
            incl = torch.cumsum(count, dim=0, dtype=torch.int64)               # plumbing, as camera_maps.compact
            faces_n = int(incl[-1])
        if faces_n > (2 ** 31 - 1) // 3:
            raise ValueError("%s: %d faces are more than int32 indices address" % (who, faces_n))
        tri_keys = torch.empty((faces_n, 3), dtype=torch.int64, device=dev)
        if faces_n:
            _lib.call("pf_tsdf_emit_triangles", _lib.ptr(tsdf), _lib.ptr(weight), nx, ny, nz, int(min_weight), _lib.ptr(incl),
                      faces_n, _lib.ptr(tri_keys), _lib.stream(), algo_bytes=20 * cells + 24 * faces_n)
        keys, rank = torch.unique(tri_keys.view(-1), sorted=True, return_inverse=True)   # plumbing: sorted keys, their ranks
        faces = rank.view(faces_n, 3).to(torch.int32)
        nv = int(keys.numel())
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        colours = torch.empty((nv, 3), dtype=torch.uint8, device=dev) if colour is not None else None
        if nv:
            _lib.call("pf_tsdf_vertices_f32", _lib.ptr(keys), nv, _lib.ptr(tsdf), _lib.ptr(colour), origin[0], origin[1],
                      origin[2], voxel, nx, ny, nz, _lib.ptr(vertices), _lib.ptr(colours), _lib.stream(),
                      algo_bytes=nv * (8 + 8 + 12 + (9 if colour is not None else 0)))
    return vertices, faces, colours, keys


def volume_bounds(depths, intrinsics, extrinsics, depth_min=1e-3, depth_max=1e5, pad=0.0):
    """``(lo (3,), hi (3,))`` float64 NumPy: the axis-aligned box of the back-projections ``A (x + .5, y + .5, 1) d + C`` of
    all pixels with ``depth_min < d < depth_max``, grown by ``pad`` on every side.  Plain torch in float32 on the device of
    ``depths`` (CPU tensors work).  A ValueError if no pixel is valid."""
    who = "volume_bounds"
    depths = cm.stack_depths(who, depths, 1)
    V, h, w = (int(s) for s in depths.shape)
    cams = cm.decompose(who, intrinsics, extrinsics, V)
    depth_min, depth_max = _check_depth_range(who, depth_min, depth_max)
    if not float(pad) >= 0.0:
        raise ValueError("%s: pad must be at least 0" % who)
    d = depths.float()
    maps = torch.from_numpy(cm.view_maps(cams)).to(d.device)
    ys, xs = torch.meshgrid(torch.arange(h, device=d.device, dtype=torch.float32) + 0.5,
                            torch.arange(w, device=d.device, dtype=torch.float32) + 0.5, indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], dim=-1)                               # (h, w, 3)
    rays = torch.einsum("vab,hwb->vhwa", maps[:, :9].view(V, 3, 3), pix)
    points = rays * d.unsqueeze(-1) + maps[:, None, None, 9:]
    valid = (d > depth_min) & (d < depth_max)
    if not bool(valid.any()):
        raise ValueError("%s: no pixel has a depth between depth_min and depth_max" % who)
    inf = torch.full_like(points, float("inf"))
    lo = torch.where(valid.unsqueeze(-1), points, inf).amin(dim=(0, 1, 2))
    hi = torch.where(valid.unsqueeze(-1), points, -inf).amax(dim=(0, 1, 2))
    return lo.double().cpu().numpy() - float(pad), hi.double().cpu().numpy() + float(pad)


def dims_for(bounds, voxel, max_samples=None):
    """``(origin (3,) float64, dims (nx, ny, nz))`` of the smallest volume of pitch ``voxel`` whose samples span the box
    ``bounds = (lo, hi)``: ``origin = lo`` and ``n = ceil((hi - lo) / voxel) + 1`` per axis.  ``max_samples``: the dense
    volume's limit unless the caller states another (a sparse volume's grid is virtual)."""
    lo, hi = (np.asarray(cm.host_f64(b), dtype=np.float64).reshape(-1) for b in bounds)
    voxel = float(voxel)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError("dims_for: bounds must be (lo, hi), two finite points with lo <= hi")
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError("dims_for: voxel must be a positive length")
    dims = tuple(int(n) for n in np.ceil((hi - lo) / voxel).astype(np.int64) + 1)
    if dims[0] * dims[1] * dims[2] > (MAX_SAMPLES if max_samples is None else max_samples):
        raise ValueError("dims_for: %d x %d x %d samples; a volume has fewer than 2^%d" %
                         (dims + (31 if max_samples is None else (max_samples + 1).bit_length() - 1,)))
    return lo.copy(), dims
