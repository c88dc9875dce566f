"""Normal maps of depth maps on the GPU, and from them the oriented normals of the fused clouds.

fusibile's ``final3d_model.ply`` and DTU's own clouds carry a normal per point; the clouds of ``fusion.py`` and
``geometric.py`` carried positions and colours only.  A depth map knows two things that a later kNN + PCA estimate on the
unstructured cloud has lost: the pixel grid, which names every point's true surface neighbours, and the camera, which says
which side of the surface was seen.  This module uses both; it runs as HIP kernels (csrc/depth_normals.hip).  **The
specification below is this project's own**; parity with fusibile's normals (a by-product of its plane sweep) is neither
claimed nor tested.  Pixel centres are at ``(x + 0.5, y + 0.5)``, as everywhere else in this pipeline.

Rays and points.  For view ``i`` let ``A_i = R_i^-1 K_i^-1``, the first 9 floats of the ``camera_maps.view_maps`` row.  For a
pixel ``q = (xq, yq)``: ``r(q) = A_i (xq + .5, yq + .5, 1)`` and ``P(q) = r(q) d_i(q)``, the vector in world axes from the
camera centre to the surface point.  The centre ``C_i`` is deliberately not added: every tangent below is a difference of
two such vectors, which then cancels at the size of the depth and not at the size of ``|C_i|``.

Validity and links, at the pixel ``p = (x, y)`` whose normal is sought:

* ``valid(q)``: ``q`` is inside the map and ``depth_min < d(q) < depth_max``;
* ``linked(q)``: ``valid(q)`` and ``|d(q) - d(p)| <= rel_jump * d(p)``.

Both are evaluated in float32 exactly as written (the library is built with ``-ffp-contract=off``), so a NumPy float32
statement reproduces every such decision bit for bit.

The horizontal tangent ``tx`` at ``p``, with ``e = (step, 0)``:

* ``P(p + e) - P(p - e)`` if ``p + e`` and ``p - e`` are both linked;
* else ``P(p + e) - P(p)`` if ``p + e`` is linked;
* else ``P(p) - P(p - e)`` if ``p - e`` is linked;
* else there is none.

The vertical tangent ``ty`` likewise with ``e = (0, step)``.

The normal.  ``c = cross(tx, ty)``, ``n = c / |c|``; if ``dot(n, P(p)) > 0`` then ``n = -n``, so that the normal faces the
camera that saw the pixel.  The pixel is undefined, and its normal ``(0, 0, 0)``, if ``p`` is not valid, a tangent is
missing, ``|c|`` is 0 or not finite, or the dot product is exactly 0.

``step >= 1`` is the finite-difference baseline in pixels: the network's depth noise makes 1-pixel differences rough, and
``step=2`` or ``3`` is the cheap remedy.  ``rel_jump`` keeps a tangent from bridging a depth discontinuity: next to one the
one-sided difference on the pixel's own side is used.

Normals of the fused clouds
---------------------------
``fusion.fuse_depth_maps(..., with_normals=True)``.  Stage A averages a pixel's back-projection with those of its consistent
partners; the normal of an emitted pixel ``p`` of view ``i`` is defined the same way: ``s = n_i(p) + sum of n_j(match)`` over
the slots of Stage A's ``match`` table in ascending order, only those with ``match >= 0``, and ``n = s / |s|``, or
``(0, 0, 0)`` if ``|s|`` is 0 or not finite (an undefined normal contributes nothing).  The rows are compacted in the order
of the points.

``geometric.geometric_filter(..., with_normals=True)``.  Its points are the back-projections at ``depth_avg``, so its
normals are ``depth_normals(depth_avg, ...)`` at the masked pixels, compacted with the same mask.

Neither fuser tests normals for agreement (the reference switches fusibile's test off with ``normal_thresh=360``).
"""
import torch

from . import _lib, camera_maps as cm

_WHO = "depth_normals"


def check_step(who, step, rel_jump):
    """``(int(step), float(rel_jump))``, or the ValueError of ``who`` for a ``step`` under 1 or a negative ``rel_jump``."""
    if isinstance(step, bool) or int(step) != step or int(step) < 1:
        raise ValueError("%s: step must be an integer of at least 1" % who)
    if not float(rel_jump) >= 0.0:
        raise ValueError("%s: rel_jump must be at least 0" % who)
    return int(step), float(rel_jump)


def normal_maps(depths, view_maps, step, rel_jump, depth_min, depth_max):
    """The kernel behind ``depth_normals`` on checked inputs: ``depths`` (V, h, w) float32 contiguous and ``view_maps``
    (V, 12) float32 on one GPU.  To be called inside the caller's ``_lib.on_device`` block."""
    V, h, w = (int(s) for s in depths.shape)
    normal = torch.empty((V, h, w, 3), dtype=torch.float32, device=depths.device)
    # per pixel: its own depth in (the four neighbour taps are other pixels' own), 12 bytes out
    _lib.call("pf_depth_normals_f32", _lib.ptr(depths), _lib.ptr(view_maps), V, h, w, int(step), float(rel_jump),
              float(depth_min), float(depth_max), _lib.ptr(normal), _lib.stream(), algo_bytes=16 * V * h * w, tag="step %d" % step)
    return normal


def fused_normals(normal, match, emit):
    """The disparity fuser's normals of the module docstring: ``normal`` (V, h, w, 3), Stage A's ``match`` (V, V-1, h, w)
    int32 and Stage B's ``emit`` (V, h, w) uint8 -> (N, 3) float32, the rows in the order of the fused points.  To be called
    inside the caller's ``_lib.on_device`` block."""
    V, h, w = (int(s) for s in emit.shape)
    out = torch.empty((V, h, w, 3), dtype=torch.float32, device=emit.device)
    _lib.call("pf_fuse_normals_f32", _lib.ptr(normal), _lib.ptr(match), _lib.ptr(emit), V, h, w, _lib.ptr(out), _lib.stream())
    return cm.compact(emit, out, None)[0]


def depth_normals(depths, intrinsics, extrinsics, step=1, rel_jump=0.01, depth_min=1e-3, depth_max=1e5):
    """Normal maps of ``depths`` (V, h, w) float32 on the GPU (0 = no depth; a sequence of (h, w) maps is stacked) with
    cameras ``intrinsics`` (V, 3, 3, of that h x w grid) and ``extrinsics`` (V, 3, 4) or (V, 4, 4), by the specification in
    this module's docstring.

    Returns ``(V, h, w, 3)`` float32 unit normals in world axes on the device of ``depths``, facing their camera;
    ``(0, 0, 0)`` where the normal is undefined.  There is no CPU path."""
    depths = cm.stack_depths(_WHO, depths, 1)
    step, rel_jump = check_step(_WHO, step, rel_jump)
    cams = cm.decompose(_WHO, intrinsics, extrinsics, int(depths.shape[0]))    # bad arguments are reported before a missing GPU
    depths, _, V, h, w, dev = cm.normalise_inputs(_WHO, depths, None, 1)
    with _lib.on_device(dev):
        return normal_maps(depths, torch.from_numpy(cm.view_maps(cams)).to(dev), step, rel_jump, depth_min, depth_max)
