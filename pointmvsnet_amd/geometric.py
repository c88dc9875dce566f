"""Round-trip geometric consistency filtering of depth maps on the GPU: per-view masks, averaged depth maps and a cloud.

The PyTorch MVS code bases published after the reference (MVSNet-pytorch, CasMVSNet and their descendants) dropped
fusibile for this check: project a pixel into a source view, sample the source depth bilinearly, project that point back,
keep the pixel if it returns close enough in enough source views, and replace its depth by the mean of the returned depths.
The reference has no such step and OpenCV is not a dependency, so **the specification below is this project's own**; it
runs as one HIP kernel (csrc/geo_filter.hip).  Pixel centres are at ``(x + 0.5, y + 0.5)``, as everywhere else in this
pipeline (``fusion.py``).

For reference view ``i``, take a pixel ``p = (x, y)`` with ``depth_min < d < depth_max``, where ``d = d_i(p)``.  For each
``j`` in ``sources[i]``, in the listed order, skipping ``-1`` and ``j == i``:

1. ``X = R_i^-1 (K_i^-1 (x+.5, y+.5, 1) d - t_i)``, ``q = K_j (R_j X + t_j)`` and ``(u, v) = q.xy / q.z``.  Skip ``j`` if
   ``q.z <= 0``.
2. ``(fx, fy) = (u - .5, v - .5)`` and ``(x0, y0) = floor(fx, fy)``.

   - Skip unless ``0 <= x0``, ``x0 + 1 <= w - 1``, ``0 <= y0`` and ``y0 + 1 <= h - 1``.  There is no border replication.
   - Skip unless all four taps ``d_j(y0.., x0..)`` are inside ``(depth_min, depth_max)``.
   - ``ds`` is the bilinear value: horizontal first, then vertical, with weights ``wx = fx - x0`` and ``wy = fy - y0``:
     ``top = d_j(y0, x0) (1 - wx) + d_j(y0, x0+1) wx``, ``bot`` likewise on row ``y0 + 1``, ``ds = top (1 - wy) + bot wy``.
3. ``Xs`` is the back-projection of ``(u, v)`` at ``ds`` from view ``j``.  Then ``q' = K_i (R_i Xs + t_i)``, ``d' = q'.z``
   and ``(u', v') = q'.xy / d'``.
4. ``j`` is consistent iff all three hold:

   - ``d' > 0``;
   - ``hypot(u' - (x+.5), v' - (y+.5)) < pix_threshold``;
   - ``|d' - d| / d < rel_depth_threshold``.
5. The outputs per pixel are:

   - ``count`` is the number of consistent sources.
   - ``depth_avg = (d + sum of d') / (count + 1)``, summed in list order.
   - ``mask = count >= num_consistent``.
   - ``depth_avg`` is written as 0 where the mask is false.
   - ``point`` is the back-projection of ``p`` at ``depth_avg`` (0 where the mask is false).

Defaults are ``pix_threshold=1.0``, ``rel_depth_threshold=0.01``, ``num_consistent=3``, ``depth_min=1e-3`` and
``depth_max=1e5``.  ``sources=None`` means all other views in ascending order.

The cloud is every masked pixel's ``point``, with the pixel's own colour if images are given, compacted view-major then
row-major, so two runs give identical bytes.  **There is no cross-view de-duplication**: a surface point seen by several
views appears once per view that keeps it.  That is what those code bases do; ``evaluation.thin_points`` exists for
evaluation, and ``fusion.fuse_depth_maps`` is the route that claims its matches.

Departures from the ``cv2.remap``-based implementations that are known: those sample at integer pixel centres and
replicate or zero-pad the border, so a projection in the outermost half pixel still reads a value there, where it is
skipped here; they interpolate across missing (zero) depths, where a tap outside ``(depth_min, depth_max)`` skips the
source here.

The matrices are composed here in float64 and handed to the kernel as float32, as ``fusion.camera_maps`` does; only the
listed pairs are composed, so cost and memory are linear in the number of views.
"""
import numpy as np
import torch

from . import _lib, camera_maps as cm, normals as nm

_WHO = "geometric_filter"


def sources_from_pairs(pair_list, view_num, num_src):
    """The ``(view_num, num_src)`` int32 source table from what ``DTUDataset`` has parsed of ``Cameras/pair.txt``
    (``dataset.cluster_list``, the file's whitespace-separated words: word 0 the number of entries, entry ``p`` = the view,
    its partner count, then (partner, score) pairs): the first ``num_src`` listed partners of every view, padded with
    ``-1``.  A view without an entry has no sources."""
    words = list(pair_list)
    view_num, num_src = int(view_num), int(num_src)
    if view_num < 1 or num_src < 0:
        raise ValueError("sources_from_pairs: view_num must be at least 1 and num_src at least 0")
    table = np.full((view_num, num_src), -1, np.int32)
    pos = 1
    for _ in range(int(words[0])):
        view, partners = int(words[pos]), int(words[pos + 1])
        listed = [int(words[pos + 2 + 2 * k]) for k in range(partners)]
        pos += 2 + 2 * partners
        if not 0 <= view < view_num:
            continue
        listed = [j for j in listed if 0 <= j < view_num][:num_src]
        table[view, :len(listed)] = listed
    return table


def view_maps_of(intrinsics, extrinsics):
    """``view_maps (V, 12)`` float32 of ``fusion.camera_maps`` alone (that function also composes all V x V pairs)."""
    return cm.view_maps(cm.decompose("view_maps_of", intrinsics, extrinsics))


def source_maps(intrinsics, extrinsics, sources):
    """``pair_maps (V, M, 2, 16)`` float32 of ``pf_geo_filter_f32`` for the ``(V, M)`` table ``sources``, composed in
    float64: entry ``[i, m, 0]`` is ``fusion.camera_maps``' ``i -> j`` layout for ``j = sources[i, m]``, ``[i, m, 1]`` the
    ``j -> i`` one (the disparity scale ``fb`` is left 0: nothing reads it); pads and ``j == i`` stay 0."""
    return _source_maps(cm.decompose("source_maps", intrinsics, extrinsics), sources)


def _source_maps(cams, sources):
    out = np.zeros(sources.shape + (2, cm.PAIR_FLOATS))
    for i, m in np.ndindex(*sources.shape):
        j = int(sources[i, m])
        if j >= 0 and j != i:
            cm.pair_row(cams, i, j, out[i, m, 0])
            cm.pair_row(cams, j, i, out[i, m, 1])
    return out.astype(np.float32)


def _source_table(sources, V):
    if sources is None:
        return np.array([[j for j in range(V) if j != i] for i in range(V)], np.int32).reshape(V, max(V - 1, 0))
    if isinstance(sources, torch.Tensor):
        if sources.is_floating_point() or sources.dtype == torch.bool:
            raise ValueError("%s: sources must be a (V, M) integer table" % _WHO)
        sources = sources.detach().cpu().numpy()
    sources = np.asarray(sources)
    if sources.ndim != 2 or sources.shape[0] != V or sources.dtype.kind not in "iu":
        raise ValueError("%s: sources must be a (V, M) integer table with the V of depths" % _WHO)
    if sources.size and (int(sources.min()) < -1 or int(sources.max()) >= V):
        raise ValueError("%s: the entries of sources must be in [-1, %d)" % (_WHO, V))
    return np.ascontiguousarray(sources, dtype=np.int32)


def geometric_filter(depths, intrinsics, extrinsics, images=None, sources=None, pix_threshold=1.0,
                     rel_depth_threshold=0.01, num_consistent=3, depth_min=1e-3, depth_max=1e5, return_points=True,
                     return_stages=False, with_normals=False, normal_step=1, normal_rel_jump=0.01):
    """Filter ``depths`` (V, h, w) float32 on the GPU (0 = no depth; a sequence of (h, w) maps is stacked) with cameras
    ``intrinsics`` (V, 3, 3, of that h x w grid) and ``extrinsics`` (V, 3, 4) or (V, 4, 4), optionally ``images``
    (V, h, w, 3) uint8, against the source views ``sources`` (V, M) (integers, ``-1`` pads; None: all other views) by the
    specification in this module's docstring.

    Returns ``(depth_avg (V, h, w) float32, mask (V, h, w) bool, count (V, h, w) int32)`` and, with ``return_points``,
    also ``(points (N, 3) float32, colours (N, 3) uint8 or None)``: five values; with ``return_stages`` last the dict of
    the kernel's per-pixel ``point`` (V, h, w, 3) and ``emit`` (V, h, w) uint8.  With ``with_normals`` (which needs
    ``return_points``) the points' unit normals (N, 3) float32 follow ``colours``: the points are back-projections at
    ``depth_avg``, so they are ``normals.depth_normals(depth_avg, ..., step=normal_step, rel_jump=normal_rel_jump)`` at the
    masked pixels (``(0, 0, 0)`` where undefined), and the stages gain those maps as ``normal`` (V, h, w, 3).  No normal is
    compared between views.  Everything is on the device of ``depths``.  There is no CPU path."""
    depths = cm.stack_depths(_WHO, depths, num_consistent)
    if with_normals:
        if not return_points:
            raise ValueError("%s: with_normals needs return_points" % _WHO)
        normal_step, normal_rel_jump = nm.check_step(_WHO, normal_step, normal_rel_jump)
    table = _source_table(sources, int(depths.shape[0]))               # a bad table is reported before a missing GPU
    depths, images, V, h, w, dev = cm.normalise_inputs(_WHO, depths, images, num_consistent)
    cams = cm.decompose(_WHO, intrinsics, extrinsics, V)
    maps, M = (cm.view_maps(cams), table, _source_maps(cams, table)), int(table.shape[1])
    with _lib.on_device(dev):
        view_maps, src, pair_maps = (torch.from_numpy(a).to(dev) for a in maps)
        count = torch.empty((V, h, w), dtype=torch.int32, device=dev)
        depth_avg = torch.empty((V, h, w), dtype=torch.float32, device=dev)
        point = torch.empty((V, h, w, 3), dtype=torch.float32, device=dev)
        emit = torch.empty((V, h, w), dtype=torch.uint8, device=dev)
        # per pixel: its own depth, four gathered depths per listed source, the outputs (count, depth, point, mask)
        listed = int(((table >= 0) & (table != np.arange(V)[:, None])).sum())
        algo = h * w * (V * (4 + 4 + 4 + 12 + 1) + 16 * listed)
        _lib.call("pf_geo_filter_f32", _lib.ptr(depths), _lib.ptr(view_maps), _lib.ptr(src), _lib.ptr(pair_maps), V, M, h, w,
                  float(pix_threshold), float(rel_depth_threshold), int(num_consistent), float(depth_min), float(depth_max),
                  _lib.ptr(count), _lib.ptr(depth_avg), _lib.ptr(point), _lib.ptr(emit), _lib.stream(), algo_bytes=algo)
        out = (depth_avg, emit.bool(), count)
        stages = {"point": point, "emit": emit}
        if return_points:
            out += cm.compact(emit, point, images)
        if with_normals:
            stages["normal"] = nm.normal_maps(depth_avg, view_maps, normal_step, normal_rel_jump, depth_min, depth_max)
            out += (cm.compact(emit, stages["normal"], None)[0],)
        return out + ((stages,) if return_stages else ())
