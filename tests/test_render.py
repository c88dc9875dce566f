"""Point-cloud rendering (pointmvsnet_amd/render.py, csrc/cloud_render.hip) against a float64 NumPy statement of its
specification, and the per-view depth errors built on it.

The reference has no such step: the specification is the text in pointmvsnet_amd/render.py and the yardstick is
``statement`` below, written from that text with no code shared with the product.  It is fed the float32-rounded ``proj``
and points, so input rounding is not part of the error.

The bounds of the GPU comparison (test_random_scene_matches_the_float64_statement)
----------------------------------------------------------------------------------
The kernel works in float32, eps = 2^-24 per rounding.  ``q = ((p0 X + p1 Y) + p2 Z) + p3`` is three products and three
sums, six roundings, each at most eps times a partial result that is at most ``A = |p0 X| + |p1 Y| + |p2 Z| + |p3|``:
``e_q = 6 eps A / (1 - 6 eps)`` (the classic gamma_6; the denominator takes the second-order terms).  So
``eps_z = e_q`` of row 2.  ``u = qx / z`` divides two such numbers and rounds once:
``r = (e_qx + |u| eps_z) / (z - eps_z)``, ``eps_u = r + eps (|u| + r)``, and ``eps_v`` likewise.  Nothing is tuned, and
there is no factor on top.

Point ``n`` covers pixel ``(x, y)`` iff ``x - s <= u < x + s + 1``, ``y - s <= v < y + s + 1`` (which is the text's
``|x - floor(u)| <= s`` and implies its range test for a pixel of the map) and ``depth_min < z < depth_max``.  It *surely*
covers it when all six inequalities hold with the interval shrunk by eps_u / eps_v / eps_z at both ends -- then the kernel's
float32 values satisfy them too --, and it *possibly* covers it when they hold with the interval widened by the same.
With ``return_index=True`` every pixel is judged on its own; no share of pixels is excused:

* a filled pixel with winner ``n``: (a) ``n`` possibly covers it; (b) the depth is within ``eps_z(n)`` of ``z64(n)``; (c) no
  sure coverer ``m`` has ``z64(m) < z64(n) - (eps_z(n) + eps_z(m))`` (every term is at most the scene's largest eps_z, so
  this asks no less than "2 eps_z"), and among the sure coverers whose float32 ``z`` -- NumPy float32 arithmetic in the
  text's order, which is the kernel's -- is bit-equal to the map's depth none has a lower index than ``n``;
* an empty pixel: no point surely covers it.

The scene (``make_scene``) is a wavy front patch before a tilted back plane seen by three cameras, with exact duplicates
(ties), points behind the cameras and beyond ``depth_max``, and a NaN and an inf row.  The statement alone verifies on the
CPU that it is not vacuous: at least half of the pixels have a sure coverer, and at least a tenth of those have two whose
``z`` differ by more than twice the largest eps_z (test_statement_scene_is_not_vacuous).

Not yet measured on an MI355X.  On tests/hipemu (the kernel source compiled for the host): no pixel violates a condition at
splat 0, 1 or 2 (87 %, 91 % and 93 % of the pixels filled); largest |depth - z64| / eps_z 0.31 in the random scene and 0.34 in
the round trip (eps_z up to 4.5e-6 and 2.7e-4 there).  ``conftest.report`` carries the same figures from the hardware
(``render_random_scene``, ``render_round_trip``: depth error / eps_z).
"""
import numpy as np
import pytest
import torch

from conftest import report
from pointmvsnet_amd import camera_maps as cm
from pointmvsnet_amd import render

EPS32 = 2.0 ** -24
H, W, V = 24, 40, 3                   # not a multiple of any tile
DEPTH_MIN, DEPTH_MAX = 1e-3, 10.6     # depth_max cuts the far edge of the back plane


# ---------------------------------------------------------------------------------------------------------------------
# the float64 statement
# ---------------------------------------------------------------------------------------------------------------------
def project64(points, proj):
    """Per view and point, in float64 from float32 inputs: u, v, z and the derived eps_u, eps_v, eps_z (module docstring)."""
    P = np.asarray(proj, np.float64).reshape(-1, 3, 4)
    X = np.concatenate([np.asarray(points, np.float64), np.ones((len(points), 1))], axis=1)
    with np.errstate(all="ignore"):
        terms = P[:, None, :, :] * X[None, :, None, :]                           # (V, N, 3, 4): the four terms of each row
        q = ((terms[..., 0] + terms[..., 1]) + terms[..., 2]) + terms[..., 3]
        e_q = 6 * EPS32 * np.abs(terms).sum(axis=-1) / (1 - 6 * EPS32)
        z, e_z = q[..., 2], e_q[..., 2]
        out = {"z": z, "eps_z": e_z}
        for name, k in (("u", 0), ("v", 1)):
            val = q[..., k] / z
            r = (e_q[..., k] + np.abs(val) * e_z) / (z - e_z)
            out[name], out["eps_" + name] = val, r + EPS32 * (np.abs(val) + r)
    return out


def z32_of(points, proj):
    """The kernel's own float32 z: NumPy float32 arithmetic in the text's order (no fused multiply-add in either)."""
    P = np.asarray(proj, np.float32).reshape(-1, 3, 4)
    X, Y, Z = (np.asarray(points, np.float32)[:, k][None, :] for k in range(3))
    with np.errstate(all="ignore"):
        return ((P[:, 2, 0, None] * X + P[:, 2, 1, None] * Y) + P[:, 2, 2, None] * Z) + P[:, 2, 3, None]


def coverers(points, proj, h, w, splat, depth_min, depth_max):
    """``(sure, possible)`` boolean (V, N, h, w) and the projection dict."""
    g = project64(points, proj)
    lo, hi = float(np.float32(depth_min)), float(np.float32(depth_max))         # the kernel compares with these
    xs, ys = np.arange(w)[None, None, :], np.arange(h)[None, None, :]
    with np.errstate(invalid="ignore"):
        def axis(val, eps, grid, sign):
            val, eps = val[..., None], eps[..., None]
            return (val >= grid - splat + sign * eps) & (val < grid + splat + 1 - sign * eps)

        def depth(sign):
            return (g["z"] > lo + sign * g["eps_z"]) & (g["z"] < hi - sign * g["eps_z"])

        both = []
        for sign in (1, -1):
            in_x, in_y = axis(g["u"], g["eps_u"], xs, sign), axis(g["v"], g["eps_v"], ys, sign)
            both.append(depth(sign)[:, :, None, None] & in_y[:, :, :, None] & in_x[:, :, None, :])
    return both[0], both[1], g


def judge(depth, index, points, proj, splat, depth_min, depth_max):
    """Every pixel of the GPU's maps against the statement; returns the figures, asserts nothing."""
    nv, h, w = depth.shape
    sure, possible, g = coverers(points, proj, h, w, splat, depth_min, depth_max)
    z32 = z32_of(points, proj)
    filled = index >= 0
    bad = {"a": 0, "b": 0, "c": 0, "tie": 0, "empty": 0, "filled_is_nonzero": int((filled != (depth != 0)).sum())}
    worst = 0.0
    for v in range(nv):
        for y in range(h):
            for x in range(w):
                cov = np.nonzero(sure[v, :, y, x])[0]
                if not filled[v, y, x]:
                    bad["empty"] += int(len(cov) > 0)
                    continue
                n = int(index[v, y, x])
                zn, en = g["z"][v, n], g["eps_z"][v, n]
                bad["a"] += int(not possible[v, n, y, x])
                dev = abs(float(depth[v, y, x]) - zn) / en
                worst = max(worst, dev)
                bad["b"] += int(not dev <= 1.0)
                bad["c"] += int((g["z"][v, cov] < zn - (en + g["eps_z"][v, cov])).any())
                tied = cov[z32[v, cov] == depth[v, y, x]]
                bad["tie"] += int((tied < n).any())
    return bad, worst, sure, g


def make_scene(seed=0):
    """``(points (N, 3) float32, K (3, 3, 3), E (3, 3, 4))``: the scene of the module docstring, shuffled."""
    rng = np.random.default_rng(seed)
    f = 30.0
    K = np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    Es = []
    for cx, angle in ((0.0, 0.0), (-1.5, 0.15), (1.2, -0.12)):                   # centre on the x axis, turned towards the scene
        c, s = np.cos(angle), np.sin(angle)
        R = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
        Es.append(np.concatenate([R, (-R @ np.array([cx, 0.1 * cx, 0.0]))[:, None]], axis=1))

    def jittered(x0, x1, y0, y1, pitch):
        gx, gy = np.meshgrid(np.arange(x0, x1, pitch), np.arange(y0, y1, pitch), indexing="ij")
        return gx.ravel() + rng.uniform(-0.4, 0.4, gx.size) * pitch, gy.ravel() + rng.uniform(-0.4, 0.4, gx.size) * pitch

    bx, by = jittered(-9.0, 9.0, -5.5, 5.5, 0.25)
    back = np.stack([bx, by, 10.0 + 0.1 * bx + 0.05 * by], axis=1)               # z up to 10.9: cut by DEPTH_MAX
    fx, fy = jittered(-2.5, 2.5, -2.0, 2.0, 0.15)
    front = np.stack([fx, fy, 7.0 + 0.3 * np.sin(2.0 * fx) * np.cos(2.0 * fy)], axis=1)
    behind = np.stack([rng.uniform(-3, 3, 40), rng.uniform(-3, 3, 40), rng.uniform(-9.0, -0.5, 40)], axis=1)
    pts = np.concatenate([back, front, behind]).astype(np.float32)
    dup = pts[rng.choice(len(back) + len(front), 150, replace=False)]             # exact ties, at other indices
    odd = np.array([[np.nan, 0.0, 8.0], [0.0, np.inf, 8.0], [0.0, 0.0, -np.inf]], np.float32)
    pts = np.concatenate([pts, dup, odd])
    pts = pts[rng.permutation(len(pts))]
    if len(pts) % 64 == 0:
        pts = pts[:-1]
    return pts, np.stack([K] * V), np.stack(Es)


@pytest.fixture(scope="module")
def scene():
    pts, K, E = make_scene()
    return pts, K, E, render.world_maps(K, E)


# ---------------------------------------------------------------------------------------------------------------------
# 1. CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_world_maps_against_float64():
    from test_fusion import make_plane_scene
    _, K, E, _, _ = make_plane_scene(3, h=37, w=53)
    got = render.world_maps(K, E)
    assert got.dtype == np.float32 and got.shape == (3, 12)
    for v in range(3):
        want = K[v] @ E[v][:3, :4]
        assert np.array_equal(got[v], want.reshape(12).astype(np.float32))
    E44 = np.concatenate([E, np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (3, 1, 4))], axis=1)
    assert np.array_equal(render.world_maps(torch.from_numpy(K), torch.from_numpy(E44)), got)
    # it undoes view_maps: a pixel centre back-projected at depth d projects to itself at depth d
    A = cm.view_maps(cm.decompose("test", K, E)).astype(np.float64)
    X = (A[1, :9].reshape(3, 3) @ np.array([17.5, 23.5, 1.0])) * 611.0 + A[1, 9:]
    q = got[1].astype(np.float64).reshape(3, 4) @ np.append(X, 1.0)
    assert np.allclose([q[0] / q[2], q[1] / q[2], q[2]], [17.5, 23.5, 611.0], rtol=1e-5)
    with pytest.raises(ValueError):
        render.world_maps(K[:2], E)


def test_arguments_are_checked_before_a_device_is_needed(scene):
    pts, K, E, _ = scene
    p = torch.from_numpy(pts)
    for bad in (pts, p.double(), p[:, :2], p[0], p.view(1, -1, 3)):
        with pytest.raises(ValueError, match="points"):
            render.render_depth_maps(bad, K, E, H, W)
    for kw in (dict(height=-1, width=W), dict(height=H, width=2.5), dict(height=H, width=W, splat=9),
               dict(height=H, width=W, splat=-1), dict(height=1 << 16, width=1 << 16)):
        with pytest.raises(ValueError):
            render.render_depth_maps(p, K, E, **kw)
    with pytest.raises(ValueError, match="intrinsics"):
        render.render_depth_maps(p, K[:, :2], E, H, W)
    with pytest.raises(ValueError, match="intrinsics"):
        render.render_depth_maps(p, K[:2], E, H, W)
    with pytest.raises(RuntimeError, match="no CPU path"):
        render.render_depth_maps(p, K, E, H, W)


def test_depth_map_errors_on_hand_made_maps():
    gt = torch.tensor([[[1.0, 2.0, 0.0, 4.0], [5.0, 0.0, 7.0, 8.0]],
                       [[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]],
                       [[3.0, 3.0, 3.0, 3.0], [3.0, 3.0, 3.0, 3.0]]])
    pred = torch.tensor([[[1.5, 0.0, 9.0, 4.0], [4.0, 6.0, 7.25, 10.0]],
                         [[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 2.0]],
                         [[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, -1.0]]])
    out = render.depth_map_errors(pred, gt, (0.5, 1.5))
    assert out["thresholds"] == [0.5, 1.5] and len(out["per_view"]) == 3
    a, b, c = out["per_view"]
    # view 0 compares five pixels with errors .5, 0, 1, .25, 2: the lower median of an odd count; "<" is strict at .5
    assert (a["n_gt"], a["n_pred"], a["n_compared"]) == (6, 7, 5) and a["coverage"] == 5 / 6.0
    assert a["abs_err_mean"] == 3.75 / 5 and a["abs_err_median"] == 0.5 and a["within"] == [2 / 5.0, 4 / 5.0]
    # no ground truth at all, and no prediction at all (a negative depth is none): every ratio over an empty set is nan
    assert (b["n_gt"], b["n_pred"], b["n_compared"]) == (0, 2, 0) and np.isnan(b["coverage"])
    assert (c["n_gt"], c["n_pred"], c["n_compared"]) == (8, 0, 0) and c["coverage"] == 0.0
    for row in (b, c):
        assert np.isnan(row["abs_err_mean"]) and np.isnan(row["abs_err_median"]) and all(np.isnan(x) for x in row["within"])
    t = out["total"]
    assert (t["n_gt"], t["n_pred"], t["n_compared"]) == (14, 9, 5) and t["coverage"] == 5 / 14.0
    assert t["abs_err_median"] == 0.5 and t["within"] == a["within"]
    # the lower median of an even count
    even = render.depth_map_errors(torch.tensor([[[1.0, 2.0, 4.0, 8.0]]]), torch.full((1, 1, 4), 1.0), [10.0])
    assert even["total"]["abs_err_median"] == 1.0 and even["total"]["within"] == [1.0]
    # the mean is a float64 sum: 2^24 errors of 1 and one of 2^-24 ... a float32 sum of 1 + 2^25 ones stops at 2^24
    n = (1 << 25) + 1
    big = render.depth_map_errors(torch.full((1, 1, n), 2.0), torch.ones((1, 1, n)), [1.5])
    assert big["total"]["abs_err_mean"] == 1.0 and big["total"]["n_compared"] == n
    assert all(isinstance(x, (int, float, list)) for row in out["per_view"] + [t] for x in row.values())
    with pytest.raises(ValueError):
        render.depth_map_errors(pred, gt[:2], [1.0])
    with pytest.raises(ValueError):
        render.depth_map_errors(pred[0], gt[0], [1.0])


def test_statement_scene_is_not_vacuous(scene):
    pts, K, E, proj = scene
    assert 2000 < len(pts) < 8000 and len(pts) % 64 != 0
    for splat in (0, 1, 2):
        sure, possible, g = coverers(pts, proj, H, W, splat, DEPTH_MIN, DEPTH_MAX)
        assert not (sure & ~possible).any()
        eps_z = float(np.nanmax(np.where(np.isfinite(g["eps_z"]), g["eps_z"], np.nan)))
        n_sure = sure.sum(axis=1)
        spread = np.zeros((V, H, W), bool)
        for v, y, x in zip(*np.nonzero(n_sure >= 2)):
            z = g["z"][v, sure[v, :, y, x]]
            spread[v, y, x] = z.max() - z.min() > 2 * eps_z
        filled = n_sure >= 1
        print("splat %d: filled %.3f, contested %.3f of them, eps_z %.3g, eps_u %.3g" % (
            splat, filled.mean(), spread.sum() / float(filled.sum()), eps_z, np.nanmax(np.where(sure.any(axis=(2, 3)), g["eps_u"], np.nan))))
        assert filled.mean() >= 0.5 and spread.sum() >= 0.1 * filled.sum()
        assert not filled.all() or splat > 0                                      # empty pixels occur at splat 0
        # both rejects occur among points that would otherwise land in the map
        lands = (g["u"] >= 0) & (g["u"] < W) & (g["v"] >= 0) & (g["v"] < H)
        assert (lands & (g["z"] >= DEPTH_MAX)).any() and (g["z"] < 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. GPU
# ---------------------------------------------------------------------------------------------------------------------
def _render(dev, pts, K, E, h=H, w=W, **kw):
    depth, index = render.render_depth_maps(torch.from_numpy(np.ascontiguousarray(pts)).to(dev), K, E, h, w,
                                            return_index=True, **kw)
    assert depth.dtype == torch.float32 and index.dtype == torch.int64 and depth.shape == index.shape == (len(K), h, w)
    return depth.cpu().numpy(), index.cpu().numpy()


def _identity_camera(f=20.0):
    K = np.array([[[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]]])
    return K, np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]


def _at(px, py, d, K):
    """The world point that an identity camera sees at image position (px, py) at depth d."""
    return [(px - K[0, 0, 2]) * d / K[0, 0, 0], (py - K[0, 1, 2]) * d / K[0, 1, 1], d]


@pytest.mark.gpu
def test_closed_form_plane_at_the_pixel_centres(dev):
    """Identity extrinsics, points on every other pixel centre of the plane z = d: the map is exactly d there (z is
    0 X + 0 Y + 1 Z + 0) and 0 elsewhere, the index the point's row."""
    K, E = _identity_camera()
    d = 7.25
    cells = [(y, x) for y in range(H) for x in range(W) if (x + y) % 2 == 0]
    pts = np.array([_at(x + 0.5, y + 0.5, d, K) for y, x in cells], np.float32)
    depth, index = _render(dev, pts, K, E)
    want_d, want_i = np.zeros((1, H, W), np.float32), np.full((1, H, W), -1, np.int64)
    for row, (y, x) in enumerate(cells):
        want_d[0, y, x], want_i[0, y, x] = d, row
    assert np.array_equal(depth, want_d) and np.array_equal(index, want_i)
    only = render.render_depth_maps(torch.from_numpy(pts).to(dev), K, E, H, W)     # without the index map
    assert isinstance(only, torch.Tensor) and np.array_equal(only.cpu().numpy(), want_d)


@pytest.mark.gpu
def test_occlusion_and_ties(dev):
    K, E = _identity_camera()
    near, far, same = _at(10.3, 5.6, 4.0, K), _at(10.7, 5.2, 6.0, K), _at(10.6, 5.4, 4.0, K)
    for pts, winner, z in (([near, far], 0, 4.0), ([far, near], 1, 4.0), ([far, near, same], 1, 4.0),
                           ([far, same, near], 1, 4.0), ([same, far, near], 0, 4.0)):
        depth, index = _render(dev, np.array(pts, np.float32), K, E)
        assert depth[0, 5, 10] == z and index[0, 5, 10] == winner
        assert (index >= 0).sum() == 1 and (depth != 0).sum() == 1
    depth, index = _render(dev, np.array([far, near], np.float32), K, E, splat=1)   # the footprint is the winner's everywhere
    assert (depth[0, 4:7, 9:12] == 4.0).all() and (index[0, 4:7, 9:12] == 1).all() and (depth != 0).sum() == 9


@pytest.mark.gpu
@pytest.mark.parametrize("splat", [0, 1, 2])
def test_random_scene_matches_the_float64_statement(dev, scene, splat):
    """All three views in one call; every pixel judged on its own (module docstring)."""
    pts, K, E, proj = scene
    depth, index = _render(dev, pts, K, E, splat=splat, depth_min=DEPTH_MIN, depth_max=DEPTH_MAX)
    bad, worst, sure, g = judge(depth, index, pts, proj, splat, DEPTH_MIN, DEPTH_MAX)
    filled = float((index >= 0).mean())
    print("splat", splat, "violations", bad, "largest |depth - z64| / eps_z", worst, "filled", filled)
    report("render_random_scene", splat=splat, depth_err_over_eps_z_max=worst, filled_share=filled,
           **{"violations_" + k: v for k, v in bad.items()})
    assert all(v == 0 for v in bad.values()), bad
    assert worst <= 1.0 and filled >= 0.5
    assert (index < len(pts)).all()


@pytest.mark.gpu
def test_borders_and_rejects(dev):
    K, E = _identity_camera()
    d = 5.0
    # just outside the map by less than the splat radius: the border pixels inside are filled, nothing else
    outside = np.array([_at(-0.4, 6.5, d, K), _at(W + 0.6, 3.5, d, K), _at(20.5, H + 0.9, d, K), _at(-0.7, -0.2, d, K)], np.float32)
    depth, index = _render(dev, outside, K, E, splat=1)
    want = np.full((H, W), -1, np.int64)
    want[5:8, 0] = 0
    want[2:5, W - 1] = 1
    want[H - 1, 19:22] = 2
    want[0, 0] = 3
    assert np.array_equal(index[0], want) and np.array_equal(depth[0], np.where(want >= 0, np.float32(d), np.float32(0)))
    assert (_render(dev, outside, K, E, splat=0)[1] == -1).all()
    far_out = np.array([_at(-1.2, 6.5, d, K), _at(W + 1.0, 3.5, d, K), _at(20.5, H + 1.5, d, K)], np.float32)
    assert (_render(dev, far_out, K, E, splat=1)[1] == -1).all()                  # u = -splat is in, u = w + splat is out
    edge = np.array([_at(-1.0, 6.5, d, K)], np.float32)
    assert (_render(dev, edge, K, E, splat=1)[1][0, 5:8, 0] == 0).all()
    # behind the camera, at either depth bound exactly, non-finite: nothing is written; the finite row among them is
    lo, hi = 2.0, 8.0
    rejects = np.array([_at(10.5, 10.5, -3.0, K), [0.0, 0.0, lo], [0.0, 0.0, hi], [np.nan, 0.0, d], [0.0, np.nan, d],
                        [0.0, 0.0, np.nan], [np.inf, 0.0, d], [0.0, -np.inf, d], [0.0, 0.0, np.inf], [0.0, 0.0, 0.0],
                        _at(3.5, 4.5, np.nextafter(np.float32(lo), np.float32(9)), K)], np.float32)
    depth, index = _render(dev, rejects, K, E, splat=2, depth_min=lo, depth_max=hi)
    assert (index >= 0).sum() == 25 and (index[0, 2:7, 1:6] == 10).all()
    assert (depth[0, 2:7, 1:6] == np.nextafter(np.float32(lo), np.float32(9))).all() and (depth != 0).sum() == 25
    assert (_render(dev, rejects[:-1], K, E, splat=2, depth_min=lo, depth_max=hi)[1] == -1).all()
    # nothing to do: empty or zero maps of the right shape, type and device
    p = torch.from_numpy(outside).to(dev)
    for kw, shape in ((dict(points=p[:0], height=H, width=W), (1, H, W)), (dict(points=p, height=0, width=W), (1, 0, W)),
                      (dict(points=p, height=H, width=0), (1, H, 0))):
        depth, index = render.render_depth_maps(kw["points"], K, E, kw["height"], kw["width"], splat=1, return_index=True)
        assert depth.shape == index.shape == shape and depth.dtype == torch.float32 and index.dtype == torch.int64
        assert depth.device == p.device and not depth.any() and (index == -1).all()


@pytest.mark.gpu
def test_determinism_and_permutation(dev, scene):
    pts, K, E, proj = scene
    kw = dict(splat=1, depth_min=DEPTH_MIN, depth_max=DEPTH_MAX)
    depth, index = _render(dev, pts, K, E, **kw)
    again = _render(dev, pts, K, E, **kw)
    assert depth.tobytes() == again[0].tobytes() and index.tobytes() == again[1].tobytes()
    perm = np.random.default_rng(7).permutation(len(pts))
    p_depth, p_index = _render(dev, pts[perm], K, E, **kw)
    assert p_depth.tobytes() == depth.tobytes() and np.array_equal(p_index >= 0, index >= 0)
    # where no other point of the cloud has the winner's float32 z in that view, the winner is the same point
    z32 = z32_of(pts, proj)
    filled = index >= 0
    unique = np.zeros_like(filled)
    for v in range(V):
        vals, counts = np.unique(z32[v][np.isfinite(z32[v])], return_counts=True)
        unique[v] = filled[v] & np.isin(depth[v], vals[counts == 1])
    assert unique.sum() > 0.5 * filled.sum() and (filled & ~unique).any()
    assert np.array_equal(perm[p_index[unique]], index[unique])
    assert np.array_equal(pts[perm][p_index[filled]].view(np.uint32), pts[index[filled]].view(np.uint32))     # ties: equal points


def _back_projected(depths, K, E):
    """Every pixel with a depth, view-major then row-major: ``X = (A (x+.5, y+.5, 1)) d + C`` with camera_maps.view_maps in
    float64, rounded to float32; and per point the bound of what the float32 roundings of the maps and of the point move
    its depth in the float32 ``proj`` by: 2^-24 (sum_k |R2k| (sum_j |A_kj p_j| d + |C_k|) + 2 sum_k |P2k X_k| + |P23|)."""
    maps = cm.view_maps(cm.decompose("test", K, E)).astype(np.float64)
    proj = render.world_maps(K, E).astype(np.float64).reshape(-1, 3, 4)
    pts, e_in = [], []
    for v in range(depths.shape[0]):
        ys, xs = np.nonzero(depths[v] > 0)
        pix = np.stack([xs + 0.5, ys + 0.5, np.ones(len(xs))], axis=1)
        d = depths[v][ys, xs].astype(np.float64)
        A, C = maps[v, :9].reshape(3, 3), maps[v, 9:]
        X = (pix @ A.T) * d[:, None] + C
        R2 = np.abs(np.asarray(E[v], np.float64)[2, :3])
        moved = ((np.abs(pix[:, None, :] * A[None]).sum(-1) * d[:, None] + np.abs(C)) * R2).sum(-1)
        e_in.append(EPS32 * (moved + 2 * (np.abs(proj[v, 2, :3]) * np.abs(X)).sum(-1) + abs(proj[v, 2, 3])))
        pts.append(X.astype(np.float32))
    return pts, e_in


@pytest.mark.gpu
def test_round_trip_with_the_back_projection(dev):
    """A random depth map with holes, back-projected with camera_maps.view_maps and rendered with the same camera at splat 0:
    every valid pixel is filled by its own row-major rank within eps_z, every hole stays 0."""
    from test_fusion import make_plane_scene
    h, w = 37, 53
    _, K, E, _, _ = make_plane_scene(3, h=h, w=w)
    K, E = K[1:2], E[1:2]
    rng = np.random.default_rng(3)
    depths = rng.uniform(450.0, 750.0, (1, h, w)).astype(np.float32)
    depths[0][rng.random((h, w)) < 0.3] = 0.0
    (pts,), (e_in,) = _back_projected(depths, K, E)
    depth, index = _render(dev, pts, K, E, h=h, w=w, splat=0)
    valid = depths[0] > 0
    want = np.full((h, w), -1, np.int64)
    want[valid] = np.arange(valid.sum())
    assert 0.6 < valid.mean() < 0.8 and np.array_equal(index[0], want) and (depth[0][~valid] == 0).all()
    g = project64(pts, render.world_maps(K, E))
    err64 = np.abs(depth[0][valid] - g["z"][0]) / g["eps_z"][0]
    err_in = np.abs(depth[0][valid] - depths[0][valid].astype(np.float64)) / (g["eps_z"][0] + e_in)
    print("round trip: |depth - z64| / eps_z", err64.max(), "|depth - d| / (eps_z + e_in)", err_in.max(), "eps_z", g["eps_z"].max())
    report("render_round_trip", depth_err_over_eps_z_max=err64.max(), depth_err_over_eps_with_inputs_max=err_in.max())
    assert err64.max() <= 1.0 and err_in.max() <= 1.0


@pytest.mark.gpu
def test_scan_accumulator_depth_errors(dev):
    """ScanAccumulator.depth_errors on the synthetic "tiny" scan through the model (the package's own helpers): a view's own
    unfiltered back-projected points give that view coverage 1 and within[t] 1 for a t above the derived bound; the cloud of
    all views still covers everything and never renders behind a view's own depth."""
    from pointmvsnet_amd import scan as S, synthetic
    from pointmvsnet_amd.model import PointMVSNet
    data, img_scales, inter_scales = synthetic.make_config("tiny", seed=3)
    nv = data["img_list"].shape[1]
    net = PointMVSNet()
    synthetic.seed_weights(net, seed=0)
    net = net.to(dev).train()
    acc = S.ScanAccumulator(nv, name="flow2", mode="NEAREST", keep_images=False)
    with pytest.raises(ValueError, match="have not been added"):
        acc.depth_errors(torch.zeros((1, 3)), [1.0])
    with torch.no_grad():
        for v in range(nv):
            order = [v] + [u for u in range(nv) if u != v]
            batch = {"img_list": data["img_list"][:, order].contiguous().to(dev), "mean": data["mean"].to(dev), "std": data["std"].to(dev),
                     "cam_params_list": data["cam_params_list"][:, order].contiguous().to(dev)}
            acc.add(batch, net(batch, img_scales, inter_scales, isFlow=True, isTest=True), view_index=v)
    raw = acc.predictions()[0]
    K, E = acc.cameras()
    h, w = raw.shape[1:]
    raw_np = raw.cpu().numpy()
    assert (raw_np > 0).all()
    pts, e_in = _back_projected(raw_np, K, E)
    proj = render.world_maps(K, E)
    for v in range(nv):
        bound = float((project64(pts[v], proj[v:v + 1])["eps_z"][0] + e_in[v]).max())
        out = acc.depth_errors(torch.from_numpy(pts[v]).to(dev), [2.0 * bound], splat=0, filtered=False)
        row = out["per_view"][v]
        print("view", v, "bound", bound, row)
        assert row["n_gt"] == row["n_pred"] == row["n_compared"] == h * w and row["coverage"] == 1.0
        assert row["within"][0] == 1.0 and row["abs_err_mean"] <= bound and row["abs_err_median"] <= bound
        report("render_scan_depth_errors", view=v, abs_err_mean_over_bound=row["abs_err_mean"] / bound)
    cloud = torch.from_numpy(np.concatenate(pts)).to(dev)
    for filtered in (False, True):
        out = acc.depth_errors(cloud, [1.0], splat=0, filtered=filtered)
        kept = acc.filtered() if filtered else raw
        assert out["total"]["n_gt"] == nv * h * w and out["total"]["n_pred"] == int((kept > 0).sum())
        assert out["total"]["n_compared"] == out["total"]["n_pred"] and [r["n_pred"] for r in out["per_view"]] == (kept > 0).flatten(1).sum(1).tolist()
    wide = acc.depth_errors(cloud, [1.0])                                         # the defaults: splat 1, the filtered maps
    assert wide["total"]["n_gt"] == nv * h * w and wide["total"]["n_pred"] == int((acc.filtered() > 0).sum())
    rendered = render.render_depth_maps(cloud, K, E, h, w).cpu().numpy()
    slack = np.concatenate([project64(pts[v], proj[v:v + 1])["eps_z"][0] + e_in[v] for v in range(nv)]).reshape(nv, h, w)
    assert (rendered > 0).all() and (rendered <= raw_np + slack).all()            # the nearest point wins: never behind one's own


@pytest.mark.gpu
def test_rows_past_two_to_the_31(dev):
    """2^31 + 300 rows, all NaN but four: the address of a row and the index map's bit pattern past 2^31 - 1."""
    if dev.type != "cuda":
        pytest.skip("a 26 GB cloud is for the hardware (tests/hipemu would walk 2^31 fibers)")
    K, E = _identity_camera()
    n = (1 << 31) + 300
    pts = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev)
    rows = [5, (1 << 31) - 1, (1 << 31), n - 1]
    cells = [(2, 3), (4, 5), (6, 7), (8, 9)]
    for r, (y, x) in zip(rows, cells):
        pts[r] = torch.tensor(_at(x + 0.5, y + 0.5, 3.0, K), dtype=torch.float32)
    depth, index = render.render_depth_maps(pts, K, E, H, W, return_index=True)
    del pts
    want = np.full((H, W), -1, np.int64)
    for r, (y, x) in zip(rows, cells):
        want[y, x] = r
    assert np.array_equal(index[0].cpu().numpy(), want) and np.array_equal(depth[0].cpu().numpy() == 3.0, want >= 0)
