"""What the two fusers (``fusion.py``, ``geometric.py``) share on the host: the float64 composition of the camera maps in
the layout of csrc/pf_camera.h, the checks of their common arguments, and the ordered compaction of the kept points."""
import numpy as np
import torch

from . import _lib

VIEW_FLOATS, PAIR_FLOATS = 12, 16       # PF_FUSE_VIEW_FLOATS, PF_FUSE_PAIR_FLOATS of include/pointflow_hip.h


def host_f64(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def decompose(who, intrinsics, extrinsics, V=None):
    """``(K, R, t, A, C)`` in float64 of ``intrinsics`` (V, 3, 3) and ``extrinsics`` (V, 3, 4) or (V, 4, 4), the cameras of
    ``V`` depth maps: ``A = R^-1 K^-1`` and the camera centres ``C = -R^-1 t``."""
    K, E = host_f64(intrinsics), host_f64(extrinsics)
    if K.ndim != 3 or K.shape[1:] != (3, 3) or E.ndim != 3 or E.shape[0] != K.shape[0] or E.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError("%s: intrinsics must be (V, 3, 3) and extrinsics (V, 3, 4) or (V, 4, 4)" % who)
    if V is not None and K.shape[0] != V:
        raise ValueError("%s: %d depth maps but %d cameras" % (who, V, K.shape[0]))
    R, t = E[:, :3, :3], E[:, :3, 3]
    Rinv = np.linalg.inv(R)
    return K, R, t, Rinv @ np.linalg.inv(K), -np.einsum("vab,vb->va", Rinv, t)


def view_maps(cams):
    """``(V, 12)`` float32: ``A`` row-major, then ``C``."""
    K, _, _, A, C = cams
    return np.concatenate([A.reshape(K.shape[0], 9), C], axis=1).astype(np.float32)


def pair_row(cams, a, b, out, with_fb=False):
    """The map ``a -> b`` into the 16-float row ``out``: ``K_b R_b A_a``, ``K_b R_b C_a + K_b t_b`` and, ``with_fb``, the
    disparity scale ``K_b[0, 0] |C_a - C_b|``.  One pair per call: a form vectorised over the pairs rounds differently."""
    K, R, t, A, C = cams
    KR = K[b] @ R[b]
    out[:9] = (KR @ A[a]).reshape(9)
    out[9:12] = KR @ C[a] + K[b] @ t[b]
    if with_fb:
        out[12] = K[b, 0, 0] * np.linalg.norm(C[a] - C[b])


def stack_depths(who, depths, num_consistent):
    """``depths`` (V, h, w), or a sequence of (h, w) maps, as one tensor; needs no GPU."""
    if not isinstance(depths, torch.Tensor):
        depths = list(depths)
        if len(set(tuple(d.shape) for d in depths)) > 1:
            raise ValueError("%s: the depth maps have different sizes" % who)
        depths = torch.stack([torch.as_tensor(d) for d in depths])
    if depths.dim() != 3:
        raise ValueError("%s: depths must be (V, h, w)" % who)
    if int(num_consistent) < 1:
        raise ValueError("%s: num_consistent must be at least 1" % who)
    return depths


def normalise_inputs(who, depths, images, num_consistent):
    """``(depths, images, V, h, w, dev)``: ``stack_depths`` as contiguous float32 on its GPU ``dev``, ``images`` (None or
    (V, h, w, 3) uint8) on that device."""
    depths = stack_depths(who, depths, num_consistent)
    V, h, w = (int(s) for s in depths.shape)
    _lib.require_gpu(depths, images if isinstance(images, torch.Tensor) else None)
    dev = depths.device
    if images is not None:
        images = torch.as_tensor(images).to(dev).contiguous()
        if tuple(images.shape) != (V, h, w, 3) or images.dtype != torch.uint8:
            raise ValueError("%s: images must be (V, h, w, 3) uint8 of the depth maps' size" % who)
    return depths.contiguous().float(), images, V, h, w, dev


def compact(emit, point, colour):
    """``(points (N, 3), colours (N, 3) or None)``: the rows of ``point`` and ``colour`` (uint8 or None) whose ``emit`` byte
    is set, in order.  To be called inside the caller's ``_lib.on_device`` block."""
    # the offsets are plumbing (an int64 prefix sum of the mask); the ordered scatter is fusion.hip's
    rank = torch.cumsum(emit.view(-1), dim=0, dtype=torch.int64)
    rows = int(rank[-1]) if rank.numel() else 0
    points = torch.empty((rows, 3), dtype=torch.float32, device=emit.device)
    colours = torch.empty((rows, 3), dtype=torch.uint8, device=emit.device) if colour is not None else None
    _lib.call("pf_fuse_compact_f32", _lib.ptr(emit), _lib.ptr(rank), _lib.ptr(point), _lib.ptr(colour), emit.numel(), rows,
              _lib.ptr(points), _lib.ptr(colours), _lib.stream())
    return points, colours
