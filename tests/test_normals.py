"""Normal maps of depth maps and the normals of the fused clouds (pointmvsnet_amd/normals.py, csrc/depth_normals.hip)
against a float64 NumPy statement of the module's docstring.

The yardstick is ``statement_normals`` below, written from that text (plain array shifts, no code shared with the product).
Its DECISIONS -- ``valid`` and ``linked`` -- are taken in ``np.float32`` exactly as the docstring writes them, so they equal
the kernel's bit for bit and there is no tie band: the defined-mask must be EQUAL.  Its VALUES are float64 on the float64
cameras.

The angular bound of the GPU comparison (``angle_bound``)
---------------------------------------------------------
eps = 2^-24 per float32 rounding.  The kernel evaluates every coordinate of ``P(q) = ((a0 px + a1 py) + a2) d`` with 8
roundings: the three matrix entries rounded from float64, two products, two sums, the product with ``d`` (``px``, ``py`` and
``d`` are exact).  Each is relative to an intermediate no larger than ``(|a0| px + |a1| py + |a2|) d``, so with
``B(q) = d(q) |(|A| (px, py, 1))|`` (the Euclidean norm over the three coordinates; ``B >= |P|``)

* ``|dP(q)| <= 8 eps B(q)``;
* a tangent ``t = P(a) - P(b)``: ``|dt| <= 8 eps (B(a) + B(b)) + eps |t|`` (the subtraction rounds once per coordinate);
* ``c = cross(tx, ty)``: ``|dc| <= |dtx| |ty| + |tx| |dty| + |dtx| |dty| + 4 eps |tx| |ty|``; the last term is the cross
  product's own arithmetic: per coordinate two products and a difference, at most ``2 eps (|u v| + |w z|)``, and the vector of
  those sums is at most ``sqrt(3) |tx| |ty|`` long;
* the direction of ``c`` then moves by at most ``asin(|dc| / |c|)``; the normalisation scales all coordinates by one rounded
  length (no change of direction) and divides each (4 eps covers a division that is 1 ulp off).

``bound = SAFETY x (asin(|dc| / |c|) + 4 eps)`` with ``SAFETY = 2`` for the second-order terms left out above.  It scales
like ``2^-24 |P| (|tx| + |ty|) / |c|``: the cancellation of the tangents at the size of the depth.  The bound is per pixel
and nothing is excused: a pixel is *ill-conditioned* when its bound exceeds 1 degree or ``|cos(n, P)|`` is below the bound
(the facing flip could then go either way), and the scenes below are CHOSEN so that the statement alone finds no such pixel
(``test_the_scenes_have_no_ill_conditioned_pixel``; focal length ~100 pixels at depth ~600, bumps of height 3 over ~17 pixels:
slopes against the view rays stay under ~35 degrees).

``| |n| - 1 |``: the squared length carries 3 eps (squares and sums), its root 1.5 eps + 1, the quotients 1 more: 3.5 eps,
5.5 eps with a root and quotients that are 1 ulp off -- ``4 x 2^-23`` (4 ulp of 1) covers both.

The fused normals (``test_fused_normals_teacher_forced``): the float64 statement sums the GPU's OWN float32 normal maps over
the GPU's own ``match``.  The kernel's T-term float32 sum rounds T - 1 times, addition k relative to a partial sum of at most
k unit vectors: ``eps (2 + .. + T) = eps (T (T + 1) / 2 - 1)`` per coordinate.  Provided the summed normals do not cancel --
``|s| >= 0.9 T``, asserted on the statement for every emitted row -- that is at most ``((T + 1) / 1.8) eps`` relative to
``|s|``, the normalisation adds 3.5 eps: within ``(V + 4) eps`` for every T <= V.
"""
import os

import numpy as np
import pytest
import torch

from conftest import report
from test_fusion import _pixel_centres, make_plane_scene
from pointmvsnet_amd.utils import io as IO

EPS32 = 2.0 ** -24
SAFETY = 2.0
H, W, V5 = 37, 45, 5                    # not multiples of the 16 x 16 tile: 3 x 3 blocks per view
DEG = np.pi / 180.0


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def _shift(a, dy, dx, fill=0.0):
    """``out[y, x] = a[y + dy, x + dx]`` where that is inside the map, else ``fill``; and the inside mask."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    inside = np.zeros((h, w), bool)
    ys, xs = slice(max(-dy, 0), max(min(h - dy, h), 0)), slice(max(-dx, 0), max(min(w - dx, w), 0))
    yq, xq = slice(max(dy, 0), max(min(h + dy, h), 0)), slice(max(dx, 0), max(min(w + dx, w), 0))
    if abs(dy) < h and abs(dx) < w:
        out[ys, xs] = a[yq, xq]
        inside[ys, xs] = True
    return out, inside


def statement_normals(depths, K, E, step=1, rel_jump=0.01, depth_min=1e-3, depth_max=1e5):
    """The docstring of pointmvsnet_amd/normals.py: ``(normal (V,h,w,3) float64, defined (V,h,w) bool, diag)``.  Decisions
    in float32 on ``float32(depths)``, values in float64 on ``depths`` as given.  ``diag`` per view: ``P``, ``B``, the
    tangents with the ``B`` of their two end points, ``c`` and the modes (+1 forward, -1 backward, 2 central, 0 none)."""
    D64, D32 = np.asarray(depths, np.float64), np.asarray(depths, np.float32)
    K, E = np.asarray(K, np.float64), np.asarray(E, np.float64)
    V, h, w = D64.shape
    lo, hi, rj = np.float32(depth_min), np.float32(depth_max), np.float32(rel_jump)
    pix = _pixel_centres(h, w)
    normal, defined, diag = np.zeros((V, h, w, 3)), np.zeros((V, h, w), bool), []
    for i in range(V):
        A = np.linalg.inv(E[i, :3, :3]) @ np.linalg.inv(K[i])
        d = D32[i]
        valid = (d > lo) & (d < hi)
        P = (pix @ A.T) * D64[i][..., None]
        B = np.linalg.norm(pix @ np.abs(A).T, axis=-1) * np.abs(D64[i])

        def linked(dy, dx):
            dq, inside = _shift(d, dy, dx)
            with np.errstate(invalid="ignore", over="ignore"):
                return valid & inside & (dq > lo) & (dq < hi) & (np.abs(dq - d) <= rj * d)        # float32 throughout

        def tangent(dy, dx):
            f, b = linked(dy, dx), linked(-dy, -dx)
            (Pf, _), (Pb, _) = _shift(P, dy, dx), _shift(P, -dy, -dx)
            (Bf, _), (Bb, _) = _shift(B, dy, dx), _shift(B, -dy, -dx)
            head, tail = np.where(f[..., None], Pf, P), np.where(b[..., None], Pb, P)
            mode = np.where(f & b, 2, np.where(f, 1, np.where(b, -1, 0)))
            return head - tail, np.where(f, Bf, B) + np.where(b, Bb, B), mode

        tx, Bx, mx = tangent(0, step)
        ty, By, my = tangent(step, 0)
        c = np.cross(tx, ty)
        length = np.linalg.norm(c, axis=-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            n = c / length[..., None]
            facing = (n * P).sum(-1)
        n = np.where((facing > 0)[..., None], -n, n)
        ok = valid & (mx != 0) & (my != 0) & (length > 0) & np.isfinite(length) & (facing != 0) & ~np.isnan(facing)
        normal[i], defined[i] = np.where(ok[..., None], n, 0.0), ok
        diag.append(dict(P=P, B=B, tx=tx, ty=ty, Bx=Bx, By=By, c=c, mode_x=mx, mode_y=my, valid=valid))
    return normal, defined, diag


def angle_bound(diag):
    """(V, h, w) radians: the module docstring's bound (meaningful where the statement's normal is defined)."""
    out = []
    for g in diag:
        ntx, nty = np.linalg.norm(g["tx"], axis=-1), np.linalg.norm(g["ty"], axis=-1)
        dtx, dty = 8 * EPS32 * g["Bx"] + EPS32 * ntx, 8 * EPS32 * g["By"] + EPS32 * nty
        dc = dtx * nty + ntx * dty + dtx * dty + 4 * EPS32 * ntx * nty
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = dc / np.linalg.norm(g["c"], axis=-1)
        out.append(SAFETY * (np.arcsin(np.minimum(np.nan_to_num(ratio, nan=1.0), 1.0)) + 4 * EPS32))
    return np.stack(out)


def ill_conditioned(normal, defined, diag, bound):
    """(V, h, w) bool: defined pixels whose bound exceeds 1 degree or whose facing is undecided within the bound."""
    P = np.stack([g["P"] for g in diag])
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.abs((normal * P).sum(-1)) / np.linalg.norm(P, axis=-1)
    return defined & ((bound > DEG) | (cos < bound))


def angle_between(a, b):
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))


# ---------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------
def _camera(h, w, f=100.0, tilt=True):
    """One camera: f = 100 pixels, the principal point at the map's centre, rotated a little and moved off the origin."""
    K = np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
    R = np.eye(3)
    if tilt:
        a, b = 0.11, -0.07
        R = (np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]) @
             np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]]))
    centre = np.array([40.0, -25.0, 10.0]) if tilt else np.zeros(3)
    return K, np.concatenate([R, (-R @ centre)[:, None]], 1)


def plane_depth(K, E, n, offset, h, w):
    """float64 depth map of the world plane ``n . X = offset`` by exact ray-plane intersection."""
    R, t = E[:3, :3], E[:3, 3]
    ray = _pixel_centres(h, w) @ np.linalg.inv(K).T
    return (offset + n @ (np.linalg.inv(R) @ t)) / (ray @ (R @ n))


def tilted_plane(h, w):
    """``(depth (1,h,w) float64, K (1,3,3), E (1,3,4), unit normal)``: a plane ~600 ahead of ``_camera``, tilted ~25
    degrees against its axis."""
    K, E = _camera(h, w)
    R, t = E[:3, :3], E[:3, 3]
    n = R.T @ np.array([0.35, -0.25, 1.0])
    n /= np.linalg.norm(n)
    offset = n @ (np.linalg.inv(R) @ (np.array([0.0, 0.0, 600.0]) - t))
    return plane_depth(K, E, n, offset, h, w)[None], K[None], E[None], n


def bumpy_scene():
    """The main scene on ``make_plane_scene``'s five cameras at 37 x 45: its exact tilted plane and its block of zeros
    (holes), plus smooth bumps of height 3, a region 4 % farther (a depth step larger than ``rel_jump``), a column beyond
    ``depth_max`` and a few pixels under ``depth_min``.  float32 depth maps."""
    depths, K, E, _, _ = make_plane_scene(V5, sigma=0.0, h=H, w=W)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = depths.astype(np.float64)
    for i in range(V5):
        out[i] += 3.0 * np.sin(2 * np.pi * xs / 19.0 + i) * np.cos(2 * np.pi * ys / 15.0 - 0.5 * i)
        out[i][25:, 12:] *= 1.04
        out[i][:, 5] = 2.0e5
        out[i][30, 7:10] = 5.0e-4
    out[depths == 0] = 0.0
    return out.astype(np.float32), K, E


def two_plane_scene(h=21, w=40, column=20):
    """One untilted camera at the origin; depth 100 left of ``column``, 110 from it on: two fronto-parallel planes."""
    K, E = _camera(h, w, tilt=False)
    d = np.full((1, h, w), 100.0, np.float32)
    d[:, :, column:] = 110.0
    return d, K[None], E[None]


def facing_camera(n, K, E, h, w):
    """``n`` or ``-n``, whichever faces the camera from the middle of the map."""
    ray = np.linalg.inv(E[:3, :3]) @ np.linalg.inv(K) @ np.array([w / 2.0, h / 2.0, 1.0])
    return -n if n @ ray > 0 else n


# ---------------------------------------------------------------------------------------------------------------------
# 1. CPU: the statement against the closed form, its conditioning on the chosen scenes, the files, the arguments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,step", [(H, W, 1), (H, W, 2), (6, W, 3), (4, W, 3), (3, W, 3), (1, 20, 1), (20, 1, 1), (H, 2, 2), (H, 3, 2)])
def test_statement_returns_the_plane_normal_exactly_where_the_rules_define_one(h, w, step):
    """Finite differences of coplanar points span the plane: on an exact plane (float64 depths) the statement returns the
    plane's normal, facing the camera, exactly at the pixels that have a neighbour ``step`` away on both axes: all of them
    when ``h >= 2 step`` and ``w >= 2 step`` (the border ring of width ``step`` through the one-sided fall-back), none when
    ``h <= step`` or ``w <= step`` (``h == 1`` and ``w == 1`` among them), and in between not the middle rows / columns.
    (``rel_jump`` 0.02: the plane's own slope, 0.35 % of the depth per pixel, must not cut a link 3 pixels long.)"""
    depth, K, E, n = tilted_plane(h, w)
    normal, defined, diag = statement_normals(depth, K, E, step=step, rel_jump=0.02)
    xs, ys = np.arange(w)[None, :], np.arange(h)[:, None]
    want_x = np.where((xs + step < w) & (xs - step >= 0), 2, np.where(xs + step < w, 1, np.where(xs - step >= 0, -1, 0)))
    want_y = np.where((ys + step < h) & (ys - step >= 0), 2, np.where(ys + step < h, 1, np.where(ys - step >= 0, -1, 0)))
    assert np.array_equal(diag[0]["mode_x"], np.broadcast_to(want_x, (h, w)))
    assert np.array_equal(diag[0]["mode_y"], np.broadcast_to(want_y, (h, w)))
    expect = np.broadcast_to((want_x != 0) & (want_y != 0), (h, w))
    assert np.array_equal(defined[0], expect) and (normal[0][~expect] == 0).all()
    assert expect.all() == (h >= 2 * step and w >= 2 * step) and expect.any() == (h > step and w > step)
    if expect.any():
        want = facing_camera(n, K[0], E[0], h, w)
        assert angle_between(normal[0][expect], want).max() < 1e-9
        assert ((normal[0] * diag[0]["P"]).sum(-1)[expect] < 0).all()       # towards the camera at every pixel


def test_statement_is_undefined_exactly_where_a_pixel_or_its_neighbours_are_missing():
    depth, K, E, n = tilted_plane(9, 11)
    depth[0, 4, 3] = 0.0                                        # a hole with neighbours: they fall back, the hole is undefined
    depth[0, 6, 6] = depth[0, 6, 8] = 0.0                       # (6, 7) keeps no horizontal neighbour at step 1
    depth[0, 0, 5] = 2.0e5                                      # beyond depth_max
    depth[0, 2, 0] *= 1.02                                      # a jump: this pixel is linked to nobody
    normal, defined, diag = statement_normals(depth, K, E)
    missing = np.zeros((9, 11), bool)
    for y, x in ((4, 3), (6, 6), (6, 8), (6, 7), (0, 5), (2, 0)):
        missing[y, x] = True
    assert np.array_equal(defined[0], ~missing)
    assert diag[0]["mode_x"][4, 2] == -1 and diag[0]["mode_x"][4, 4] == 1 and diag[0]["mode_y"][3, 3] == -1
    assert diag[0]["mode_x"][2, 1] == 1 and diag[0]["mode_y"][1, 0] == -1 and diag[0]["mode_y"][3, 0] == 1
    assert angle_between(normal[0][defined[0]], facing_camera(n, K[0], E[0], 9, 11)).max() < 1e-9
    # with step 2 the pixel between the two holes has both horizontal neighbours again
    assert statement_normals(depth, K, E, step=2)[1][0, 6, 7]


def _gpu_scenes():
    yield ("bumpy",) + bumpy_scene()
    depth, K, E, _ = tilted_plane(H, W)
    yield "plane", depth.astype(np.float32), K, E
    yield ("two_planes",) + two_plane_scene()
    depths, K, E, _, _ = make_plane_scene(V5, sigma=0.2, h=H, w=W)
    yield "fused", depths, K, E


def test_the_scenes_have_no_ill_conditioned_pixel():
    """The precondition of every GPU comparison below, on the statement alone: the cap on excused pixels is zero."""
    for name, depths, K, E in _gpu_scenes():
        for step in (1, 2):
            normal, defined, diag = statement_normals(depths, K, E, step=step)
            bound = angle_bound(diag)
            ill = ill_conditioned(normal, defined, diag, bound)
            print("%s step %d: defined %.3f, largest bound %.4f deg, ill-conditioned %d"
                  % (name, step, defined.mean(), bound[defined].max() / DEG, ill.sum()))
            assert defined.any() and not ill.any()
    # the main scene exercises every rule: holes, both bounds, the jump, one-sided and central differences
    depths, K, E = bumpy_scene()
    _, defined, diag = statement_normals(depths, K, E)
    modes = np.stack([g["mode_x"] for g in diag])
    assert all((modes == m).any() for m in (-1, 0, 1, 2))
    assert (depths == 0).any() and (depths > 1e5).any() and ((depths > 0) & (depths < 1e-3)).any()
    inner = (slice(None), slice(26, H - 1), slice(13, W - 1))
    assert defined[inner].all() and (modes[:, 27:H - 1, 12] == 1).all() and (modes[:, 27:H - 1, 11] == -1).all()


def test_ply_round_trip_with_normals(tmp_path):
    rng = np.random.default_rng(1)
    pts = rng.normal(size=(29, 3)).astype(np.float32)
    nrm = rng.normal(size=(29, 3)).astype(np.float32)
    col = rng.integers(0, 256, (29, 3), dtype=np.uint8)
    path = str(tmp_path / "a.ply")
    IO.write_ply(path, pts, col, nrm)
    blob = open(path, "rb").read()
    head = blob[:blob.index(b"end_header\n") + 11]
    assert head == (b"ply\nformat binary_little_endian 1.0\nelement vertex 29\nproperty float x\nproperty float y\nproperty float z\n"
                    b"property float nx\nproperty float ny\nproperty float nz\n"
                    b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert len(blob) == len(head) + 29 * 27
    row = np.frombuffer(blob[len(head):len(head) + 27], dtype=np.uint8)
    assert row[:24].view("<f4").tolist() == pts[0].tolist() + nrm[0].tolist() and row[24:].tolist() == col[0].tolist()
    p, c, n = IO.load_ply(path, return_normals=True)
    assert np.array_equal(p, pts) and np.array_equal(c, col) and np.array_equal(n, nrm) and n.dtype == np.float32
    assert len(IO.load_ply(path)) == 2 and np.array_equal(IO.load_ply(path)[1], col)
    assert np.array_equal(IO.load_ply_points(path), pts)
    IO.write_ply(path, pts, normals=nrm)                        # without colours
    p, c, n = IO.load_ply(path, return_normals=True)
    assert np.array_equal(p, pts) and c is None and np.array_equal(n, nrm)
    assert os.path.getsize(path) == len(head) - len(b"property uchar red\nproperty uchar green\nproperty uchar blue\n") + 29 * 24
    IO.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.float32))
    p, c, n = IO.load_ply(path, return_normals=True)
    assert p.shape == c.shape == n.shape == (0, 3)
    with pytest.raises(Exception):
        IO.write_ply(path, pts, col, nrm[:-1])


def _todays_ply_bytes(points, colors):
    """The writer as it was before it knew normals, byte for byte: header, then packed ``<f4 x 3 [u1 x 3]`` rows."""
    n = points.shape[0]
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % n
    if colors is None:
        return (head + "end_header\n").encode("ascii") + points.astype("<f4").tobytes()
    head += "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
    rows = np.concatenate([points.astype("<f4").view(np.uint8).reshape(n, 12), colors], axis=1)
    return head.encode("ascii") + rows.tobytes()


def test_ply_without_normals_is_unchanged(tmp_path):
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(31, 3)).astype(np.float32)
    col = rng.integers(0, 256, (31, 3), dtype=np.uint8)
    path = str(tmp_path / "a.ply")
    for colours in (col, None):
        IO.write_ply(path, pts, colours)
        assert open(path, "rb").read() == _todays_ply_bytes(pts, colours)
        IO.write_ply(path, pts, colours, normals=None)
        assert open(path, "rb").read() == _todays_ply_bytes(pts, colours)
        got = IO.load_ply(path)                                 # old files: the default return value is what it was
        assert len(got) == 2 and np.array_equal(got[0], pts)
        assert (got[1] is None) if colours is None else np.array_equal(got[1], colours)
        assert IO.load_ply(path, return_normals=True)[2] is None


def test_normals_refuse_bad_arguments_before_asking_for_a_gpu():
    from pointmvsnet_amd import fusion, geometric, normals, scan
    depths, K, E, _, _ = make_plane_scene(3, h=12, w=14)
    d = torch.from_numpy(depths)                                # a CPU tensor: a good call ends at "no CPU path"
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="step"):
            normals.depth_normals(d, K, E, step=bad)
    with pytest.raises(ValueError, match="rel_jump"):
        normals.depth_normals(d, K, E, rel_jump=-0.1)
    with pytest.raises(ValueError, match=r"\(V, h, w\)"):
        normals.depth_normals(d[0], K, E)
    with pytest.raises(ValueError, match="different sizes"):
        normals.depth_normals([depths[0], depths[1][:, :-1]], K[:2], E[:2])
    with pytest.raises(ValueError, match="3 depth maps but 2 cameras"):
        normals.depth_normals(d, K[:2], E[:2])
    with pytest.raises(ValueError, match="intrinsics"):
        normals.depth_normals(d, K[:, :2], E)
    with pytest.raises(RuntimeError, match="no CPU path"):
        normals.depth_normals(d, K, E, step=2)
    with pytest.raises(ValueError, match="step"):
        fusion.fuse_depth_maps(d, K, E, with_normals=True, normal_step=0)
    with pytest.raises(ValueError, match="step"):
        geometric.geometric_filter(d, K, E, with_normals=True, normal_step=0)
    with pytest.raises(ValueError, match="return_points"):
        geometric.geometric_filter(d, K, E, with_normals=True, return_points=False)
    for call in (fusion.fuse_depth_maps, geometric.geometric_filter):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(d, K, E, with_normals=True)
    acc = scan.ScanAccumulator(2)
    with pytest.raises(ValueError, match="have not been added"):
        acc.normals()
    with pytest.raises(ValueError, match="have not been added"):
        acc.fuse(with_normals=True)


# ---------------------------------------------------------------------------------------------------------------------
# 2. GPU
# ---------------------------------------------------------------------------------------------------------------------
def _normals(dev, depths, K, E, **kw):
    from pointmvsnet_amd import normals
    out = normals.depth_normals(torch.from_numpy(np.ascontiguousarray(depths)).to(dev), K, E, **kw)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(depths.shape) + (3,)
    return out.cpu()


def _compare(name, got, depths, K, E, **kw):
    """The kernel's maps against the statement: equal defined-mask, every defined pixel within its own bound, unit length;
    no pixel is excused.  Returns the statement's normals and mask."""
    normal, defined, diag = statement_normals(depths, K, E, **kw)
    bound = angle_bound(diag)
    assert not ill_conditioned(normal, defined, diag, bound).any()
    g = got.numpy().astype(np.float64)
    g_defined = (g != 0).any(-1)
    print("%s %s: defined %d of %d (GPU %d)" % (name, kw, defined.sum(), defined.size, g_defined.sum()))
    if not defined.any():
        assert not g_defined.any()
        return normal, defined
    ratio = angle_between(g, normal)[defined] / bound[defined]
    length = np.abs(np.linalg.norm(g, axis=-1) - 1.0)[g_defined]
    print("%s %s: angle / bound max %.4f, bound max %.3e rad, | |n| - 1 | max %.3e" % (name, kw, ratio.max(), bound[defined].max(), length.max()))
    report("normals_" + name, step=kw.get("step", 1), angle_over_bound_max=ratio.max(), bound_max_rad=bound[defined].max(),
           angle_max_rad=angle_between(g, normal)[defined].max(), unit_length_err_max=length.max(), defined_share=defined.mean())
    assert np.array_equal(g_defined, defined)
    assert ratio.max() <= 1.0
    assert length.max() <= 4 * 2.0 ** -23
    return normal, defined


@pytest.mark.gpu
@pytest.mark.parametrize("step", [1, 2])
def test_kernel_matches_the_float64_statement(dev, step):
    depths, K, E = bumpy_scene()
    got = _normals(dev, depths, K, E, step=step)
    _, defined = _compare("bumpy", got, depths, K, E, step=step)
    assert 0.5 < defined.mean() < 0.95
    # other bounds and another jump: the same statement
    kw = dict(step=step, rel_jump=0.002, depth_min=500.0, depth_max=640.0)
    _compare("bumpy_narrow", _normals(dev, depths, K, E, **kw), depths, K, E, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(1, 20), (20, 1), (16, 16), (17, 33)])
def test_kernel_on_maps_of_one_row_one_column_and_whole_tiles(dev, h, w):
    depth, K, E, _ = tilted_plane(h, w)
    depths = np.concatenate([depth, depth * 1.1]).astype(np.float32)
    K, E = np.concatenate([K, K]), np.concatenate([E, E])
    for step in (1, 3):                                         # rel_jump 0.02: the plane's slope must not cut a 3-pixel link
        got = _normals(dev, depths, K, E, step=step, rel_jump=0.02)
        _, defined = _compare("plane_%dx%d" % (h, w), got, depths, K, E, step=step, rel_jump=0.02)
        assert defined.all() if min(h, w) >= 2 * step else not defined.any()


@pytest.mark.gpu
def test_exact_plane_against_the_closed_form(dev):
    depth, K, E, n = tilted_plane(H, W)
    depths = depth.astype(np.float32)
    want = facing_camera(n, K[0], E[0], H, W)
    for step in (1, 2):
        got = _normals(dev, depths, K, E, step=step)
        normal, defined = _compare("plane", got, depths, K, E, step=step)
        assert defined.all()
        # the float32 depth map is the plane to one rounding of d: the statement on it is off the closed form by that much
        # (measured here in float64), the kernel off the statement by at most its bound
        off = angle_between(normal[0], want)
        bound = angle_bound(statement_normals(depths, K, E, step=step)[2])[0]
        angle = angle_between(got.numpy().astype(np.float64)[0], want)
        print("step %d: angle to the plane's normal max %.3e rad, bound max %.3e, statement off by %.3e"
              % (step, angle.max(), bound.max(), off.max()))
        assert (angle <= bound + off).all()
        assert (bound + off).max() < 0.05 * DEG                  # the scene: what the test above lets pass is a small angle


@pytest.mark.gpu
def test_a_tangent_does_not_bridge_a_depth_discontinuity(dev):
    """Two fronto-parallel planes meeting at a column: the pixels on both sides of the step get the fronto-parallel normal
    through their one-sided differences.  A kernel that ignores ``linked`` tilts them by atan(10 / 2) ~ 79 degrees."""
    depths, K, E = two_plane_scene()
    want = np.array([0.0, 0.0, -1.0])
    for step in (1, 2):
        got = _normals(dev, depths, K, E, step=step)
        normal, defined = _compare("two_planes", got, depths, K, E, step=step)
        assert defined.all() and angle_between(normal[0], want).max() < 1e-12
        g = got.numpy().astype(np.float64)[0]
        bound = angle_bound(statement_normals(depths, K, E, step=step)[2])[0]
        assert (angle_between(g, want) <= bound).all()          # the columns 20 - step .. 20 + step - 1 among them
    # the same map with the jump allowed: the statement (and the kernel) do bridge it -- the test above is not vacuous
    loose = statement_normals(depths, K, E, rel_jump=0.2)[0]
    assert angle_between(loose[0][:, 19:21], want).min() > 45 * DEG
    _compare("two_planes_bridged", _normals(dev, depths, K, E, rel_jump=0.2), depths, K, E, rel_jump=0.2)


@pytest.mark.gpu
def test_two_runs_give_identical_bytes_and_views_permute(dev):
    depths, K, E = bumpy_scene()
    a, b = _normals(dev, depths, K, E, step=2), _normals(dev, depths, K, E, step=2)
    assert a.numpy().tobytes() == b.numpy().tobytes()
    perm = [3, 0, 4, 1, 2]
    c = _normals(dev, depths[perm], K[perm], E[perm], step=2)
    assert c.numpy().tobytes() == a[perm].contiguous().numpy().tobytes()
    one = _normals(dev, depths[2:3], K[2:3], E[2:3], step=2)     # a view alone
    assert torch.equal(one[0], a[2])


def statement_fused_normals(normal, match, emit):
    """The fused normals of the docstring in float64 from per-view maps ``normal`` (V,h,w,3), ``match`` (V,V-1,h,w) and
    ``emit`` (V,h,w): ``(rows (N,3), |s| (N,), terms (N,))`` in the order of the points."""
    V, h, w = emit.shape
    N = np.asarray(normal, np.float64).reshape(V, h * w, 3)
    rows, lengths, terms = [], [], []
    for i in range(V):
        s = N[i].copy()
        t = (N[i] != 0).any(-1).astype(np.int64)
        for slot in range(V - 1):
            j = slot if slot < i else slot + 1
            m = match[i, slot].reshape(-1)
            ok = m >= 0
            s[ok] += N[j][m[ok]]
            t[ok] += (N[j][m[ok]] != 0).any(-1)
        e = emit[i].reshape(-1)
        length = np.linalg.norm(s[e], axis=-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            rows.append(np.where((length > 0)[:, None], s[e] / length[:, None], 0.0))
        lengths.append(length)
        terms.append(t[e])
    return np.concatenate(rows), np.concatenate(lengths), np.concatenate(terms)


@pytest.fixture(scope="module")
def consistent5():
    """``make_plane_scene`` at 37 x 45 with little noise (sigma 0.2: neighbouring views agree, so the normals of a pixel's
    matches point the same way) and its seeded colours."""
    return make_plane_scene(V5, sigma=0.2, h=H, w=W)


@pytest.mark.gpu
def test_fused_normals_teacher_forced(dev, consistent5):
    """The GPU's own ``match``, ``emit`` and normal maps through the float64 statement of the sum (module docstring)."""
    from pointmvsnet_amd import fusion
    depths, K, E, images, _ = consistent5
    d, im = torch.from_numpy(depths).to(dev), torch.from_numpy(images).to(dev)
    kw = dict(images=im, num_consistent=2)
    # normal_step 2: nearly every pixel has a normal.  A jump of 0.1 % at step 1 is under the plane's own slope per pixel along x,
    # so most pixels have no horizontal link and some emitted rows are left with no term at all
    for label, nkw in (("step2", dict(normal_step=2)), ("sparse", dict(normal_step=1, normal_rel_jump=0.001))):
        pts, col, nrm, st = fusion.fuse_depth_maps(d, K, E, return_stages=True, with_normals=True, **kw, **nkw)
        assert nrm.dtype == torch.float32 and tuple(nrm.shape) == tuple(pts.shape) and pts.shape[0] > 100
        maps = st["normal"].cpu()
        assert torch.equal(maps, _normals(dev, depths, K, E, step=nkw["normal_step"], rel_jump=nkw.get("normal_rel_jump", 0.01)))
        emit, match = st["emit"].cpu().numpy(), st["match"].cpu().numpy()
        assert torch.equal(pts.cpu(), st["point"].cpu()[st["emit"].cpu()])      # rows in the order of the points
        want, length, terms = statement_fused_normals(maps.numpy(), match, emit)
        assert (length[terms > 0] >= 0.9 * terms[terms > 0]).all()           # the bound's precondition: no cancellation
        got = nrm.cpu().numpy().astype(np.float64)
        err = np.linalg.norm(got - want, axis=-1)
        undefined = (want == 0).all(-1)
        print("fused normals %s: %d rows, %d undefined, terms up to %d, largest error %.3e (bound %.3e)"
              % (label, len(want), undefined.sum(), terms.max(), err.max(), (V5 + 4) * EPS32))
        report("normals_fused_" + label, rows=len(want), undefined=undefined.sum(), err_max=err.max(), bound=(V5 + 4) * EPS32)
        assert np.array_equal((got == 0).all(-1), undefined) and int(undefined.sum()) == int((terms == 0).sum())
        assert err.max() <= (V5 + 4) * EPS32                                 # |want| = 1: relative IS absolute
        assert terms.max() >= 3 and (np.abs(np.linalg.norm(got[~undefined], axis=-1) - 1.0) <= 4 * 2.0 ** -23).all()
        assert (label == "sparse") == bool(undefined.any())                  # the scene: both kinds of row are exercised
    nkw = dict(normal_step=1, normal_rel_jump=0.001)
    # the option changes nothing else: same points, colours and stages as without it; the default returns two values
    plain = fusion.fuse_depth_maps(d, K, E, **kw)
    assert len(plain) == 2
    assert plain[0].cpu().numpy().tobytes() == pts.cpu().numpy().tobytes() and torch.equal(plain[1], col)
    staged = fusion.fuse_depth_maps(d, K, E, return_stages=True, **kw)
    assert len(staged) == 3 and "normal" not in staged[2]
    for k in ("count", "point", "colour", "match", "emit"):
        assert torch.equal(staged[2][k], st[k]), k
    again = fusion.fuse_depth_maps(d, K, E, with_normals=True, **kw, **nkw)
    assert len(again) == 3 and again[2].cpu().numpy().tobytes() == nrm.cpu().numpy().tobytes()
    # nothing emits: three empty tensors
    none = fusion.fuse_depth_maps(d[:3], K[:3], E[:3], with_normals=True, num_consistent=3)
    assert none[0].shape == (0, 3) and none[1] is None and none[2].shape == (0, 3)


@pytest.mark.gpu
def test_round_trip_route_takes_the_normals_of_depth_avg(dev, consistent5):
    from pointmvsnet_amd import geometric, normals
    depths, K, E, images, _ = consistent5
    d, im = torch.from_numpy(depths).to(dev), torch.from_numpy(images).to(dev)
    kw = dict(images=im, num_consistent=2)
    out = geometric.geometric_filter(d, K, E, with_normals=True, normal_step=2, normal_rel_jump=0.02, return_stages=True, **kw)
    assert len(out) == 7
    depth_avg, mask, _, pts, col, nrm, st = out
    maps = normals.depth_normals(depth_avg, K, E, step=2, rel_jump=0.02)
    assert pts.shape[0] > 100 and tuple(nrm.shape) == tuple(pts.shape)
    assert torch.equal(nrm, maps[mask]) and torch.equal(st["normal"], maps)   # bit for bit
    assert float((nrm != 0).any(dim=1).float().mean()) > 0.5
    plain = geometric.geometric_filter(d, K, E, **kw)
    assert len(plain) == 5 and all(torch.equal(a, b) for a, b in zip(plain, out[:5]))


@pytest.mark.gpu
def test_through_the_scan_accumulator_and_the_file(dev, consistent5, tmp_path):
    """Synthetic predictions of the five views (confidences that keep every pixel) through ``ScanAccumulator``:
    ``write_ply(..., with_normals=True)`` then ``load_ply(..., return_normals=True)`` returns the rows of the fuser."""
    from pointmvsnet_amd import fusion, geometric, normals, scan
    depths, K, E, images, cams = consistent5
    acc = scan.ScanAccumulator(V5, mode="NEAREST")
    for v in range(V5):
        preds = {"flow2": torch.from_numpy(depths[v])[None, None].to(dev), "flow2_prob": torch.full((1, 5, H, W), 0.2).to(dev),
                 "coarse_prob_map": torch.ones(1, 1, H, W).to(dev)}
        cam = cams[v:v + 1][None].clone()
        batch = {"cam_params_list": cam.to(dev), "cam_params_list_host": cam, "img_list": torch.zeros(1, 1, 3, H, W),
                 "ref_img": torch.from_numpy(images[v:v + 1, :, :, ::-1].copy())}
        acc.add(batch, preds, view_index=v)
    assert torch.equal(acc.filtered().cpu(), torch.from_numpy(depths))
    Ka, Ea = acc.cameras()
    assert torch.equal(acc.normals(step=2), normals.depth_normals(acc.filtered(), Ka, Ea, step=2))
    assert tuple(acc.normals().shape) == (V5, H, W, 3)
    fuse = dict(num_consistent=2, with_normals=True, normal_step=2)
    want = fusion.fuse_depth_maps(acc.filtered(), Ka, Ea, images=acc.images(), **fuse)
    path = str(tmp_path / "oriented.ply")
    got = acc.write_ply(path, **fuse)
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want)) and got[0].shape[0] > 100
    p, c, n = IO.load_ply(path, return_normals=True)
    assert p.tobytes() == want[0].cpu().numpy().tobytes() and np.array_equal(c, want[1].cpu().numpy())
    assert n.tobytes() == want[2].cpu().numpy().tobytes()
    two = acc.write_ply(path, num_consistent=2)                 # the default: no normals in the file
    assert len(two) == 2 and torch.equal(two[0], want[0]) and IO.load_ply(path, return_normals=True)[2] is None
    # the other method passes the option through as well
    geo = geometric.geometric_filter(acc.filtered(), Ka, Ea, images=acc.images(), **fuse)
    rt = acc.write_ply(path, method="roundtrip", **fuse)
    assert len(rt) == 3 and all(torch.equal(a, b) for a, b in zip(rt, geo[3:6]))
    assert IO.load_ply(path, return_normals=True)[2].tobytes() == geo[5].cpu().numpy().tobytes()
    assert len(acc.fuse(method="roundtrip", num_consistent=2)) == 2
