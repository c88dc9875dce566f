"""Depth-map fusion (pointmvsnet_amd/fusion.py, csrc/fusion.hip) against a float64 NumPy statement of its specification.

fusibile, the program the reference runs for this step, exists neither here nor for ROCm: the specification is the text in
pointmvsnet_amd/fusion.py and the yardstick is ``statement_stage_a`` / ``statement_stage_b`` below, written from that text
in the manner of oracle/bruteforce.py (plain loops over views, no shared code with the product).

The tolerances of the GPU comparison (test_stage_a_matches_the_float64_statement)
----------------------------------------------------------------------------------
The kernel works in float32 (eps = 2^-24 per rounding) on matrices composed in float64 and rounded once.  With
S = w + max f_j b_ij / depth_min_of_scene (projected coordinates reach w, the disparity-sized translation term reaches
f b / z) and the scene's depth range:

* u = q.x / q.z.  q.x = (M0 px + M1 py + M2) d + T0: three rounded matrix entries, two products, two sums, the product
  with d, the rounded T0 and the last sum -- at most 9 roundings, each relative to an intermediate no larger than S q.z
  in magnitude; q.z likewise (9 roundings of terms of size q.z), which moves u by up to 9 eps |u| <= 9 eps S; the division
  adds one more.  |u_f32 - u_f64| <= 19 eps S.  ``tie_px`` = 4 x that.
* the disparities f b / z and f b / d_j: f b is rounded once, z carries 9 eps (above), each division 1 eps; d_j is an
  input and exact: 11 eps + 2 eps relative to a disparity of at most D = max f b / depth_min_of_scene, the subtraction's own
  rounding is relative to the difference (~ the threshold) and is covered by rounding 13 up to 14.  ``tie_disp`` = 4 x
  14 eps D.
* depth bounds: the kernel compares against the float32 nearest to depth_min / depth_max (1 eps relative), z carries
  9 eps relative to the depth scale: ``tie_rel`` = 4 x 10 eps, applied to d_i and d_j relative to the bound and to z
  (against the bound 0) relative to the scene's largest depth.
* point: X = (A p) d + C has 9 roundings relative to at most R = (largest depth) x (longest ray |K^-1 p|) + max |C|; the
  mean of n + 1 <= V such terms adds n sums and a division, each 1 eps relative to a partial sum of at most (n + 1) R, i.e.
  (n + 1) eps R per term of the mean: (9 + V + 1) eps R.  ``tol_point`` = 4 x that, in world units.
* colour: sums of at most V bytes are exact in float32; a quotient by n + 1 that is exactly k + 0.5 is representable and
  rounds (to even) identically in both precisions, any other quotient is at least 1 / (2 V) away from a tie.  Equal.

A pixel is near-tied in partner view j if the statement's u or v is within tie_px of an integer, a depth within tie_rel
of a bound, or the disparity difference within tie_disp of the threshold.  Outside those (pixel, view) pairs ``match`` must
be EQUAL, so ``count`` can differ only in the views that caused a tie; where no view is tied the point must agree within
tol_point.  The near-tied share is capped at 10 % of the valid pixels of every view (measured with these bands on the
committed scene, float64 statement alone: see test_statement_tie_share_stays_under_the_cap; worst view 1.4 %).
Measured on an MI355X (parity_report.jsonl, "fusion_stage_a"): tie_px 1.09e-3, tie_disp 2.66e-4, tol_point 3.36e-3; no
decision differs outside the bands, 6 of the 1 315 (pixel, view) pairs inside them do, largest point error 1.14e-4.
"""
import os

import numpy as np
import pytest
import torch

from conftest import report
from pointmvsnet_amd import synthetic
from pointmvsnet_amd.utils import io as IO

EPS32 = 2.0 ** -24
TIE_CAP = 0.10
H, W, V5 = 128, 160, 5
ZERO_BLOCK = (slice(10, 20), slice(30, 60))
OUTLIER_BLOCK = (slice(80, 90), slice(100, 130))


# ---------------------------------------------------------------------------------------------------------------------
# the float64 statement
# ---------------------------------------------------------------------------------------------------------------------
def _pixel_centres(h, w):
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    return np.stack([xs, ys, np.ones_like(xs)], -1)                      # (h, w, 3)


def _back_project(K, E, pix, depth):
    cam = (pix @ np.linalg.inv(K).T) * depth[..., None]
    return (cam - E[:3, 3]) @ np.linalg.inv(E[:3, :3]).T


def statement_stage_a(depths, K, E, images=None, disp_threshold=0.12, depth_min=1e-3, depth_max=1e5, views=None):
    """Stage A of the specification in float64.  Returns count (V,h,w), point (V,h,w,3), colour (V,h,w,3) uint8 or None,
    match (V,V-1,h,w) and ``diag``: per (i, slot) the u, v, z, d_j, disparity difference and how far the pair got.
    ``views``: compute these reference views only (tools/microbench_fusion.py times a few and scales)."""
    D = np.asarray(depths, np.float64)
    K = np.asarray(K, np.float64)
    E = np.asarray(E, np.float64)
    V, h, w = D.shape
    pix = _pixel_centres(h, w)
    C = np.stack([-np.linalg.inv(E[i, :3, :3]) @ E[i, :3, 3] for i in range(V)])
    count = np.zeros((V, h, w), np.int64)
    point = np.zeros((V, h, w, 3))
    colour = None if images is None else np.zeros((V, h, w, 3), np.uint8)
    match = np.full((V, V - 1, h, w), -1, np.int64)
    diag = {}
    for i in (range(V) if views is None else views):
        valid = (D[i] > depth_min) & (D[i] < depth_max)
        X = _back_project(K[i], E[i], pix, D[i])
        acc = np.where(valid[..., None], X, 0.0)
        cacc = None if images is None else np.where(valid[..., None], images[i].astype(np.float64), 0.0)
        slot = 0
        for j in range(V):
            if j == i:
                continue
            q = (X @ E[j, :3, :3].T + E[j, :3, 3]) @ K[j].T
            z = q[..., 2]
            with np.errstate(divide="ignore", invalid="ignore"):
                u, v = q[..., 0] / z, q[..., 1] / z
                xj, yj = np.floor(u), np.floor(v)
                inside = valid & (z > 0) & (xj >= 0) & (xj < w) & (yj >= 0) & (yj < h)
                xi = np.where(inside, xj, 0).astype(np.int64)
                yi = np.where(inside, yj, 0).astype(np.int64)
                dj = np.where(inside, D[j][yi, xi], 0.0)
                readable = inside & (dj > depth_min) & (dj < depth_max)
                fb = K[j, 0, 0] * np.linalg.norm(C[i] - C[j])
                diff = np.abs(fb / z - fb / np.where(readable, dj, 1.0))
            cons = readable & (diff < disp_threshold)
            match[i, slot] = np.where(cons, yi * w + xi, -1)
            Xj = _back_project(K[j], E[j], np.stack([xi + 0.5, yi + 0.5, np.ones_like(z)], -1), dj)
            acc = acc + np.where(cons[..., None], Xj, 0.0)
            if images is not None:
                cacc = cacc + np.where(cons[..., None], images[j][yi, xi].astype(np.float64), 0.0)
            count[i] += cons
            diag[(i, slot)] = dict(j=j, u=u, v=v, z=z, dj=dj, diff=diff, valid=valid, inside=inside, readable=readable, fb=fb)
            slot += 1
        point[i] = acc / (count[i] + 1)[..., None]
        if images is not None:
            colour[i] = np.rint(cacc / (count[i] + 1)[..., None]).astype(np.uint8)
    return count, point, colour, match, diag


def statement_stage_b(count, match, num_consistent):
    """Stage B of the specification (integers only): the emit masks (V, h, w) from count (V,h,w) and match (V,V-1,h,w)."""
    count = np.asarray(count)
    match = np.asarray(match)
    V, h, w = count.shape
    used = np.zeros((V, h * w), bool)
    emit = np.zeros((V, h * w), bool)
    for i in range(V):
        emit[i] = ~used[i] & (count[i].reshape(-1) >= num_consistent)
        for slot in range(V - 1):
            j = slot if slot < i else slot + 1
            m = match[i, slot].reshape(-1)[emit[i]]
            used[j, m[m >= 0]] = True
    return emit.reshape(V, h, w)


# ---------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------
def make_plane_scene(num_view, seed=0, sigma=1.5, h=H, w=W):
    """Cameras of synthetic.make_scene, a tilted world plane at depth 600 on view 0's axis, every view's depth map by exact
    ray-plane intersection plus seeded Gaussian noise (sigma 1.5 puts the disparity differences on both sides of the
    threshold), a block of zeros and a block of gross outliers (x 1.3); seeded random colours.  Depth maps are float32."""
    cams = synthetic.make_scene(h, w, num_view, 48, seed=seed)["cam_params_list"][0]
    E = cams[:, 0, :3, :4].double().numpy()
    K = cams[:, 1, :3, :3].double().numpy()
    R, t = E[:, :, :3], E[:, :, 3]
    n = R[0].T @ np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    c = n @ (np.linalg.inv(R[0]) @ (np.array([0.0, 0.0, 600.0]) - t[0]))
    pix = _pixel_centres(h, w)
    rng = np.random.default_rng(seed)
    depths = []
    for i in range(num_view):
        ray = pix @ np.linalg.inv(K[i]).T
        d = (c + n @ (np.linalg.inv(R[i]) @ t[i])) / (ray @ (R[i] @ n))       # n . (R^-1 (ray d - t)) = c
        d = d + rng.normal(0.0, 1.0, d.shape) * sigma
        d[ZERO_BLOCK] = 0.0
        d[OUTLIER_BLOCK] *= 1.3
        depths.append(d.astype(np.float32))
    images = rng.integers(0, 256, (num_view, h, w, 3), dtype=np.uint8)
    return np.stack(depths), K, E, images, cams


def derived_bands(depths, K, E):
    """tie_px, tie_disp, tie_rel, tol_point from float32 rounding (module docstring), each with its factor 4."""
    V, h, w = depths.shape
    good = depths[depths > 0]
    dmin, dmax = float(good.min()), float(good.max())
    C = np.stack([-np.linalg.inv(E[i, :3, :3]) @ E[i, :3, 3] for i in range(V)])
    fb = max(K[j, 0, 0] * np.linalg.norm(C[i] - C[j]) for i in range(V) for j in range(V))
    disp = fb / dmin
    corners = np.array([[0.5, 0.5, 1.0], [w - 0.5, 0.5, 1.0], [0.5, h - 0.5, 1.0], [w - 0.5, h - 0.5, 1.0]])
    ray = max(np.linalg.norm(np.linalg.inv(K[i]) @ p) for i in range(V) for p in corners)
    radius = dmax * ray + np.abs(C).max()
    return dict(tie_px=4 * 19 * EPS32 * (w + disp), tie_disp=4 * 14 * EPS32 * disp, tie_rel=4 * 10 * EPS32,
                tol_point=4 * (9 + V + 1) * EPS32 * radius, depth_scale=dmax)


def tie_masks(diag, V, h, w, bands, disp_threshold=0.12, depth_min=1e-3, depth_max=1e5):
    """(V, V-1, h, w) bool: the statement is too close to one of its own decisions in this (pixel, partner view)."""
    def near_bound(d):
        return (np.abs(d - depth_min) <= bands["tie_rel"] * depth_min) | (np.abs(d - depth_max) <= bands["tie_rel"] * depth_max)

    out = np.zeros((V, V - 1, h, w), bool)
    for (i, slot), g in diag.items():
        with np.errstate(invalid="ignore"):
            t = np.abs(g["z"]) <= bands["tie_rel"] * bands["depth_scale"]
            near_image = (g["z"] > 0) & (g["u"] > -1) & (g["u"] < w + 1) & (g["v"] > -1) & (g["v"] < h + 1)
            t |= near_image & ((np.abs(g["u"] - np.rint(g["u"])) <= bands["tie_px"]) |
                               (np.abs(g["v"] - np.rint(g["v"])) <= bands["tie_px"]))
            t |= g["inside"] & near_bound(g["dj"])
            t |= g["readable"] & (np.abs(g["diff"] - disp_threshold) <= bands["tie_disp"])
        out[i, slot] = t & g["valid"]
    return out


def own_depth_ties(depths, bands, depth_min=1e-3, depth_max=1e5):
    """(V, h, w) bool: the pixel's OWN depth is within tie_rel of a bound (every partner view is then undecided)."""
    d = np.asarray(depths, np.float64)
    return (np.abs(d - depth_min) <= bands["tie_rel"] * depth_min) | (np.abs(d - depth_max) <= bands["tie_rel"] * depth_max)


def tie_share(ties, own, depths):
    """Per view: near-tied pixels (any partner view, or the own depth) / valid pixels."""
    tied = ties.any(axis=1) | own
    valid = (depths > 1e-3) & (depths < 1e5)
    return [float((tied[i] & valid[i]).sum()) / max(int(valid[i].sum()), 1) for i in range(depths.shape[0])]


# ---------------------------------------------------------------------------------------------------------------------
# 1. CPU: the statement against closed forms, the PLY files, the missing CPU path
# ---------------------------------------------------------------------------------------------------------------------
def _two_camera_case():
    """Two fronto-parallel cameras (R = I) one baseline B = 6 apart along x, f = 100, a plane at depth 100 seen by both:
    the disparity is f B / 100 = 6 pixels exactly, so pixel (x, y) of view 0 lands on the CENTRE of (x - 6, y) of view 1.
    The right half of view 1 (columns >= 40) reports depth 101 (disparity difference |6 - 600 / 101| = 0.059 < 0.12:
    consistent, its own back-projection is on another plane) and the last 8 columns 103 (0.175: inconsistent)."""
    h, w, f, B = 6, 64, 100.0, 6.0
    K = np.array([[f, 0.0, 32.0], [0.0, f, 3.0], [0.0, 0.0, 1.0]])
    E0 = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    E1 = np.concatenate([np.eye(3), np.array([[-B], [0.0], [0.0]])], 1)
    d0 = np.full((h, w), 100.0)
    d1 = np.full((h, w), 100.0)
    d1[:, 40:] = 101.0
    d1[:, 56:] = 103.0
    return np.stack([d0, d1]), np.stack([K, K]), np.stack([E0, E1]), (h, w, f, B)


def test_statement_matches_the_closed_form_of_two_fronto_parallel_cameras():
    D, K, E, (h, w, f, B) = _two_camera_case()
    count, point, _, match, _ = statement_stage_a(D, K, E)
    xs = np.arange(w)
    ys = np.arange(h)
    # view 0: partner pixel x - 6, outside for x < 6; inconsistent where the partner reports 103 (x - 6 >= 56)
    exp0 = ((xs - 6 >= 0) & (xs - 6 < 56)).astype(int)
    assert np.array_equal(count[0], np.broadcast_to(exp0, (h, w)))
    exp_match = np.where(exp0[None, :] == 1, ys[:, None] * w + (xs[None, :] - 6), -1)
    assert np.array_equal(match[0, 0], exp_match)
    # the mean point in closed form: own X at depth 100, partner's at its depth dj through the centre of (x - 6, y)
    X_own = np.stack(np.broadcast_arrays((xs[None, :] + 0.5 - 32.0) / f * 100.0, (ys[:, None] + 0.5 - 3.0) / f * 100.0, 100.0), -1)
    dj = D[1][:, np.clip(xs - 6, 0, w - 1)]
    X_par = np.stack(np.broadcast_arrays((xs[None, :] - 6 + 0.5 - 32.0) / f * dj + B, (ys[:, None] + 0.5 - 3.0) / f * dj, dj), -1)
    expect = np.where(exp0[None, :, None] == 1, (X_own + X_par) / 2.0, X_own)
    assert np.abs(point[0] - expect).max() < 1e-9
    assert np.abs(point[0][:, 6:46] - X_own[:, 6:46]).max() < 1e-9        # same plane: the mean IS the point
    # view 1: depth 100 -> x + 6 exactly; 101 -> x + 0.5 + 5.94 -> x + 6; 103 -> 5.825 -> x + 6, but |5.825 - 6| > 0.12
    exp1 = ((xs + 6 < w) & (xs < 56)).astype(int)
    assert np.array_equal(count[1], np.broadcast_to(exp1, (h, w)))
    # stage B with one consistent view required: view 0 emits its h x 56 consistent pixels (columns 6 .. 61) and claims their partners,
    # which are exactly the pixels of view 1 that have a consistent partner themselves -> view 1 emits nothing
    emit = statement_stage_b(count, match, 1)
    assert emit[0].sum() == h * 56 and emit[1].sum() == 0
    assert statement_stage_b(count, match, 2).sum() == 0                   # two partners can never be consistent with V = 2


def test_statement_tie_share_stays_under_the_cap():
    """The float64 statement alone, with the derived bands, on the committed scenes: the near-tied share of every view
    must leave the GPU comparison at least 90 % of the valid pixels."""
    for nv in (V5, 3):
        depths, K, E, images, _ = make_plane_scene(nv)
        bands = derived_bands(depths, K, E)
        count, _, _, _, diag = statement_stage_a(depths, K, E, images)
        shares = tie_share(tie_masks(diag, nv, H, W, bands), own_depth_ties(depths, bands), depths)
        print("V=%d bands %s tie shares %s count>=3 %s" % (nv, {k: "%.3g" % v for k, v in bands.items()},
                                                           ["%.4f" % s for s in shares],
                                                           ["%.3f" % float((count[i] >= 3).mean()) for i in range(nv)]))
        assert max(shares) <= TIE_CAP, shares
        if nv == V5:                                # the scene exercises both sides of the threshold and Stage B
            assert all(0.02 < float((count[i] >= 3).mean()) < 0.6 for i in range(nv))
            assert 0 < statement_stage_b(count, statement_stage_a(depths, K, E)[3], 3).sum()


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(37, 3)).astype(np.float32)
    col = rng.integers(0, 256, (37, 3), dtype=np.uint8)
    IO.write_ply(str(tmp_path / "a.ply"), pts, col)
    p, c = IO.load_ply(str(tmp_path / "a.ply"))
    assert p.dtype == np.float32 and c.dtype == np.uint8 and np.array_equal(p, pts) and np.array_equal(c, col)
    blob = open(str(tmp_path / "a.ply"), "rb").read()
    head = blob[:blob.index(b"end_header\n") + 11]
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\n")
    assert b"property uchar blue\n" in head and len(blob) == len(head) + 37 * 15
    IO.write_ply(str(tmp_path / "b.ply"), pts)
    p, c = IO.load_ply(str(tmp_path / "b.ply"))
    assert c is None and np.array_equal(p, pts)
    assert os.path.getsize(str(tmp_path / "b.ply")) == len(head) - len(b"property uchar red\nproperty uchar green\nproperty uchar blue\n") + 37 * 12
    IO.write_ply(str(tmp_path / "c.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    p, c = IO.load_ply(str(tmp_path / "c.ply"))
    assert p.shape == (0, 3) and c.shape == (0, 3)
    with pytest.raises(Exception):
        IO.write_ply(str(tmp_path / "d.ply"), pts[:, :2])


def test_fusion_has_no_cpu_path():
    from pointmvsnet_amd import fusion
    depths, K, E, _, _ = make_plane_scene(3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion.fuse_depth_maps(torch.from_numpy(depths), K, E)
    with pytest.raises(ValueError):
        fusion.fuse_depth_maps([depths[0], depths[1][:, :-1]], K[:2], E[:2])      # views of different sizes


def test_camera_maps_reproduce_the_projection():
    """The composed float32 pair matrices describe q = K_j (R_j X + t_j) of the back-projected pixel (to float32)."""
    from pointmvsnet_amd import fusion
    depths, K, E, _, _ = make_plane_scene(3)
    view_maps, pair_maps = fusion.camera_maps(K, E)
    assert view_maps.shape == (3, fusion.VIEW_FLOATS) and pair_maps.shape == (3, 3, fusion.PAIR_FLOATS)
    p, d = np.array([17.5, 93.5, 1.0]), 611.0
    X = _back_project(K[0], E[0], p, np.float64(d))
    assert np.allclose(view_maps[0, :9].reshape(3, 3).astype(np.float64) @ p * d + view_maps[0, 9:], X, rtol=1e-5)
    q = K[2] @ (E[2, :3, :3] @ X + E[2, :3, 3])
    m = pair_maps[0, 2].astype(np.float64)
    assert np.allclose(m[:9].reshape(3, 3) @ p * d + m[9:12], q, rtol=1e-5)
    C = [-np.linalg.inv(E[i, :3, :3]) @ E[i, :3, 3] for i in (0, 2)]
    assert np.isclose(m[12], K[2, 0, 0] * np.linalg.norm(C[0] - C[1]), rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 2.-4. GPU
# ---------------------------------------------------------------------------------------------------------------------
def _run(dev, depths, K, E, images, **kw):
    from pointmvsnet_amd import fusion
    pts, col, st = fusion.fuse_depth_maps(torch.from_numpy(depths).to(dev), K, E,
                                          images=None if images is None else torch.from_numpy(images).to(dev),
                                          return_stages=True, **kw)
    return pts.cpu(), None if col is None else col.cpu(), {k: (None if v is None else v.cpu()) for k, v in st.items()}


@pytest.fixture(scope="module")
def scene5():
    return make_plane_scene(V5)


@pytest.fixture(scope="module")
def fused5(dev, scene5):
    depths, K, E, images, _ = scene5
    return _run(dev, depths, K, E, images)


@pytest.mark.gpu
def test_stage_a_matches_the_float64_statement(dev, scene5, fused5):
    """Tolerances and the near-tie rule: module docstring.  Measured worst cases go to parity_report.jsonl."""
    depths, K, E, images, _ = scene5
    _, _, st = fused5
    bands = derived_bands(depths, K, E)
    count, point, colour, match, diag = statement_stage_a(depths, K, E, images)
    ties = tie_masks(diag, V5, H, W, bands) | own_depth_ties(depths, bands)[:, None]
    shares = tie_share(ties, own_depth_ties(depths, bands), depths)
    g_count, g_match = st["count"].numpy().astype(np.int64), st["match"].numpy().astype(np.int64)
    g_point, g_colour = st["point"].numpy().astype(np.float64), st["colour"].numpy()
    clean = ~ties.any(axis=1)
    point_err = float(np.abs(g_point - point)[clean].max())
    flips = int((g_match != match)[ties].sum())
    print("bands", bands, "tie shares", shares, "point err", point_err, "decisions that differ inside the ties", flips)
    report("fusion_stage_a", tie_px=bands["tie_px"], tie_disp=bands["tie_disp"], tie_rel=bands["tie_rel"],
           tol_point=bands["tol_point"], worst_tie_share=max(shares), point_err_max=point_err, tied_decisions_flipped=flips,
           tied_decisions=int(ties.sum()), mismatches_outside_ties=int((g_match != match)[~ties].sum()))
    assert max(shares) <= TIE_CAP, shares
    assert np.array_equal(g_count, (g_match >= 0).sum(axis=1))                 # count IS the number of recorded matches
    assert np.array_equal(g_match[~ties], match[~ties])                        # so count differs only in tied views
    assert np.array_equal(g_count[clean], count[clean])
    assert point_err <= bands["tol_point"], (point_err, bands["tol_point"])
    assert np.array_equal(g_colour[clean], colour[clean])
    invalid = ~((depths > 1e-3) & (depths < 1e5))
    assert (g_count[invalid] == 0).all() and (g_match.transpose(0, 2, 3, 1)[invalid] == -1).all()
    assert (g_point[invalid] == 0).all()


def _check_teacher_forced(depths, pts, col, st, num_consistent):
    count, match = st["count"].numpy(), st["match"].numpy()
    emit = torch.from_numpy(statement_stage_b(count, match, num_consistent))
    assert torch.equal(st["emit"], emit)
    assert torch.equal(pts, st["point"][emit])                               # view-major, then row-major; same bytes
    if col is not None:
        assert torch.equal(col, st["colour"][emit])
    zero = torch.from_numpy(depths == 0)
    assert not bool(st["emit"][zero].any())
    V = depths.shape[0]
    for i in range(V):                                                        # a pixel without depth is never a match
        for slot in range(V - 1):
            j = slot if slot < i else slot + 1
            m = match[i, slot]
            assert (depths[j].reshape(-1)[m[m >= 0]] != 0).all()
    return emit


@pytest.mark.gpu
def test_stage_b_and_compaction_teacher_forced(dev, scene5, fused5):
    """The GPU's own Stage A count / match through the NumPy Stage B: emit masks, point order and point bytes are equal;
    two runs are byte-identical; the outlier block emits what the statement says (nothing is assumed about it)."""
    depths, K, E, images, _ = scene5
    pts, col, st = fused5
    emit = _check_teacher_forced(depths, pts, col, st, 3)
    assert pts.shape[0] == int(emit.sum()) > 0 and pts.dtype == torch.float32 and col.dtype == torch.uint8
    block = (slice(None),) + OUTLIER_BLOCK
    assert torch.equal(st["emit"][block], emit[block])
    pts2, col2, st2 = _run(dev, depths, K, E, images)
    assert torch.equal(pts2, pts) and torch.equal(col2, col)
    assert pts2.numpy().tobytes() == pts.numpy().tobytes()
    for k in ("count", "match", "point", "colour", "emit"):
        assert torch.equal(st2[k], st[k]), k
    report("fusion_stage_b", points=int(pts.shape[0]), emitting_share=float(emit.float().mean()))
    # one consistent view suffices: more points, same rules; no colours: None comes back
    pts1, col1, st1 = _run(dev, depths, K, E, None, num_consistent=1)
    _check_teacher_forced(depths, pts1, col1, st1, 1)
    assert col1 is None and st1["colour"] is None and pts1.shape[0] > pts.shape[0]
    assert torch.equal(st1["count"], st["count"]) and torch.equal(st1["match"], st["match"])


@pytest.mark.gpu
def test_three_views_can_never_reach_three_consistent_partners(dev):
    depths, K, E, images, _ = make_plane_scene(3)
    pts, col, st = _run(dev, depths, K, E, images)
    assert pts.shape == (0, 3) and col.shape == (0, 3) and not bool(st["emit"].any())
    assert int(st["count"].max()) <= 2
    pts2, col2, st2 = _run(dev, depths, K, E, images, num_consistent=2)
    _check_teacher_forced(depths, pts2, col2, st2, 2)
    assert pts2.shape[0] > 0


@pytest.mark.gpu
def test_end_to_end_through_the_evaluation_files(dev, scene5, tmp_path):
    """AsyncEvalWriter(filter_thresholds=...) writes every view's ``_prob_filtered.pfm`` and camera file from synthetic
    predictions; fuse_scene_folder reads them back and writes final3d_model.ply; the file equals fuse_depth_maps on the
    same arrays."""
    from pointmvsnet_amd import fusion
    from pointmvsnet_amd.utils import eval_file_logger as EL
    depths, K, E, _, cams = scene5
    g = torch.Generator().manual_seed(3)
    writer = EL.AsyncEvalWriter(filter_thresholds=(0.15, 0.3), write_points=False)
    for v in range(V5):
        preds = {"coarse_depth_map": torch.from_numpy(depths[v][::2, ::2].copy())[None, None],
                 "coarse_prob_map": torch.rand(1, 1, H // 2, W // 2, generator=g),
                 "flow1_prob": torch.softmax(2.0 * torch.randn(1, 5, H, W, generator=g), dim=1),
                 "flow1": torch.from_numpy(depths[v])[None, None]}
        cam = cams[v:v + 1][None].clone()                                    # (1, 1, 2, 4, 4): this view as the reference
        batch = {"cam_params_list": cam.to(dev), "cam_params_list_host": cam, "img_list": torch.zeros(1, 1, 3, H, W)}
        writer.submit(batch, {k: t.to(dev) for k, t in preds.items()},
                      str(tmp_path / "Eval" / "Rectified" / "scan1" / ("rect_%03d_3_r5000.png" % (v + 1))), "out")
    writer.close()
    scene = str(tmp_path / "Eval" / "out" / "scan1")
    pts, col = fusion.fuse_scene_folder(scene, "flow1", V5, device=dev)
    assert col is None
    filtered = np.stack([np.ascontiguousarray(IO.load_pfm(os.path.join(scene, "%08d_flow1_prob_filtered.pfm" % v))[0])
                         for v in range(V5)])
    kept = float((filtered != 0).mean())
    assert 0.2 < kept < 0.95 and np.array_equal(filtered[filtered != 0], depths[filtered != 0])   # the filter did filter
    # the camera files carry the float32 cameras in their shortest decimal form: read as float64 they are the arrays
    # fuse_scene_folder works on (equal to K, E to float32 precision, not bit for bit)
    file_cams = [IO.load_cam_dtu(open(os.path.join(scene, "cam_%08d_flow1.txt" % v))) for v in range(V5)]
    K_file, E_file = np.stack([c[1, :3, :3] for c in file_cams]), np.stack([c[0] for c in file_cams])
    assert np.allclose(K_file, K, rtol=1e-6, atol=0) and np.allclose(E_file[:, :3], E, rtol=1e-6, atol=1e-9)
    want, _ = fusion.fuse_depth_maps(torch.from_numpy(filtered).to(dev), K_file, E_file)
    got, got_col = IO.load_ply(os.path.join(scene, "final3d_model.ply"))
    assert got_col is None and want.shape[0] > 0
    assert torch.equal(torch.from_numpy(got.copy()), want.cpu()) and torch.equal(pts.cpu(), want.cpu())
    report("fusion_end_to_end", points=int(want.shape[0]), depth_kept_share=kept)
    other = str(tmp_path / "elsewhere.ply")
    fusion.fuse_scene_folder(scene, "flow1", V5, device=dev, out_path=other)
    assert open(other, "rb").read() == open(os.path.join(scene, "final3d_model.ply"), "rb").read()
