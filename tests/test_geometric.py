"""Round-trip geometric consistency filter (pointmvsnet_amd/geometric.py, csrc/geo_filter.hip) against a float64 NumPy
statement of its specification.

The reference has no such step and OpenCV is not installed: the specification is the text in pointmvsnet_amd/geometric.py
and the yardstick is ``statement`` below, written from that text with plain loops over views and sources and no code
shared with the product, in the manner of tests/test_fusion.py (whose ``make_plane_scene`` supplies the scenes).

The tolerances of the GPU comparison (test_kernel_matches_the_float64_statement)
--------------------------------------------------------------------------------
The kernel works in float32 (eps = 2^-24 per rounding) on matrices composed in float64 and rounded once.  S, D, R and
``ray`` are those of test_fusion.py: S = w + D with D = max f_j b_ij / (smallest depth of the scene), R = (largest depth)
x (longest ray) + max |C|.  B = the longest baseline, Z = (largest depth) + B.  Every ``e_`` below is WITHOUT the factor 4;
the factor is applied once, where a band or tolerance is formed.

1. Forward projection.  u = q.x / q.z has 19 roundings relative to S (test_fusion.py's count: 9 in q.x, 9 in q.z, the
   division): e_uv = 19 eps S.  fx = u - .5 adds one: e_w = 20 eps S, which is also the error of the weights wx = fx - x0,
   wy = fy - y0 (the subtraction of the floor is exact).
2. Sampling.  The taps are inputs and exact.  ds = top (1 - wy) + bot wy moves by at most |t01 - t00| e_w or |t11 - t10| e_w
   horizontally and |bot - top| e_w vertically, each at most ``spread`` = max tap - min tap of THIS 2 x 2 neighbourhood; the
   lerps are 7 roundings relative to the largest tap (1 - w, two products and a sum, twice, the outer 1 - wy shared), taken
   as 8: e_ds = 2 spread e_w + 8 eps max tap.  Per (pixel, source): noisy or stepped depth makes it large exactly where it is.
3. The way back, q' = (M' (u, v, 1)) ds + T'.  Its own arithmetic is that of step 1: 19 eps S on u', v' and 9 eps Z on d'
   (the terms of the z row are at most the depth plus |T'.z| <= B).  What it inherits from e_uv and e_ds is EVALUATED, not
   bounded: the statement repeats step 3 at the eight corners (u +- e_uv, v +- e_uv, ds +- e_ds) and takes the largest
   deviation of u', v' and d' (``prop``).  Step 3 is a smooth rational map, so the corners are its extremes to first order;
   the factor 4 covers the remainder.  e_ret = 19 eps S + prop_px, e_dr = 9 eps Z + prop_d.
4. The tests.  err = sqrt(ex^2 + ey^2) moves by at most |delta ex| + |delta ey| and has six roundings of its own (two
   differences, two squares, the sum, the root) relative to itself: e_err = e_ret_u + e_ret_v + 6 eps err.
   rel = |d' - d| / d: d is an input; the difference and the quotient round once each relative to rel; the threshold is
   rounded to float32 once: e_rel = e_dr / d + 3 eps rel.  Likewise pix_threshold: one more eps in e_err.
5. Outputs.  depth_avg is a mean of at most M + 1 terms whose errors are at most the largest e_dr of the pixel's sources;
   the sums and the division add (M + 1) eps of the largest depth: tol_depth = 4 (max e_dr + (M + 1) eps dmax), per pixel.
   point = (A p) depth_avg + C: 9 roundings relative to R, and the depth's error along a ray of length at most ``ray``:
   tol_point = 4 x 9 eps R + ray tol_depth.

A (pixel, source) pair is near-tied when the statement is within 4 x the error of one of its own decisions:
* z against 0 (|z| <= 4 x 9 eps Z) or d' against 0 (|d'| <= 4 e_dr);
* fx or fy within 4 e_w of an INTEGER: at the integers 0 and w - 1 (h - 1) that is the sampling border; at the others the
  two precisions may take 2 x 2 neighbourhoods one column (row) apart, whose taps can differ in validity;
* a tap, or the pixel's own depth (then every source is undecided), within 4 eps (relative) of a depth bound (the kernel
  compares with the float32 nearest to the bound);
* err within 4 e_err of pix_threshold, or rel within 4 e_rel of rel_depth_threshold.
The kernel reports no per-source decision, so the comparison is on ``count``: equal where no source of the pixel is tied,
else different by at most the number of tied sources.  Where no source is tied depth_avg and point must agree within
tol_depth / tol_point; ``mask == (count >= num_consistent)`` and the zeros off the mask hold exactly, everywhere.
The near-tied share is capped at 10 % of the valid pixels of every view
(test_statement_tie_share_and_both_sides_of_the_thresholds: float64 statement alone, worst view 1.1 % at V = 5, 0.8 % at V = 3).

Not yet measured on an MI355X.  On tests/hipemu (the kernel source compiled for the host; "geometric_kernel", V = 5 at
128 x 160): bands 4 e_w 1.14e-3 px, 4 e_err up to 6.1e-2 px (median 4.9e-3), 4 e_rel up to 7.4e-4 (median 1.7e-5); count
differs in 0 pixels outside the ties and in 1 of the 951 tied pixels; largest depth_avg error 7.1e-4 and point error 7.3e-4
units, each inside its per-pixel tolerance.  V = 3 at 37 x 53: 0 outside, 0 of 6 tied pixels, 1.5e-4 / 1.7e-4.
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_fusion import make_plane_scene

EPS32 = 2.0 ** -24
TIE_CAP = 0.10
H, W, V5 = 128, 160, 5
SMALL = (37, 53)                  # odd sizes: partial tiles, and x0 + 1 <= w - 1 at a width that is no multiple of anything
DEFAULTS = dict(pix_threshold=1.0, rel_depth_threshold=0.01, num_consistent=3, depth_min=1e-3, depth_max=1e5)
TABLE = np.array([[1, -1], [1, 2], [3, 0], [4, 2], [0, 3]])      # M = 2: a pad in row 0, row 1 names itself


# ---------------------------------------------------------------------------------------------------------------------
# the float64 statement
# ---------------------------------------------------------------------------------------------------------------------
def _centres(h, w):
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    return xs, ys


def _lift(K, E, u, v, depth):
    """World point of image position (u, v) of camera (K, E) at ``depth``."""
    cam = (np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T) * depth[..., None]
    return (cam - E[:3, 3]) @ np.linalg.inv(E[:3, :3]).T


def _drop(K, E, X):
    """(u, v, z) of world point X in camera (K, E)."""
    q = (X @ E[:3, :3].T + E[:3, 3]) @ K.T
    return q[..., 0] / q[..., 2], q[..., 1] / q[..., 2], q[..., 2]


def statement(depths, K, E, sources=None, pix_threshold=1.0, rel_depth_threshold=0.01, num_consistent=3, depth_min=1e-3,
              depth_max=1e5):
    """The specification in float64.  Returns count, depth_avg, mask, point and ``diag``: per (i, m) what every step saw."""
    D = np.asarray(depths, np.float64)
    K = np.asarray(K, np.float64)
    E = np.asarray(E, np.float64)
    V, h, w = D.shape
    if sources is None:
        sources = [[j for j in range(V) if j != i] for i in range(V)]
    px, py = _centres(h, w)
    count = np.zeros((V, h, w), np.int64)
    depth_avg = np.zeros((V, h, w))
    mask = np.zeros((V, h, w), bool)
    point = np.zeros((V, h, w, 3))
    diag = {}
    for i in range(V):
        d = D[i]
        valid = (d > depth_min) & (d < depth_max)
        total = d.copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            X = _lift(K[i], E[i], px, py, d)
            for m, j in enumerate(sources[i]):
                j = int(j)
                if j < 0 or j == i:
                    continue
                u, v, z = _drop(K[j], E[j], X)
                fx, fy = u - 0.5, v - 0.5
                x0, y0 = np.floor(fx), np.floor(fy)
                inside = valid & (z > 0) & (x0 >= 0) & (x0 + 1 <= w - 1) & (y0 >= 0) & (y0 + 1 <= h - 1)
                xi, yi = np.where(inside, x0, 0).astype(np.int64), np.where(inside, y0, 0).astype(np.int64)
                taps = np.stack([D[j][yi, xi], D[j][yi, np.minimum(xi + 1, w - 1)], D[j][np.minimum(yi + 1, h - 1), xi],
                                 D[j][np.minimum(yi + 1, h - 1), np.minimum(xi + 1, w - 1)]])
                readable = inside & ((taps > depth_min) & (taps < depth_max)).all(axis=0)
                wx, wy = fx - x0, fy - y0
                top = taps[0] * (1 - wx) + taps[1] * wx
                bot = taps[2] * (1 - wx) + taps[3] * wx
                ds = top * (1 - wy) + bot * wy
                ub, vb, dr = _drop(K[i], E[i], _lift(K[j], E[j], u, v, ds))
                err = np.hypot(ub - px, vb - py)
                rel = np.abs(dr - d) / d
                cons = readable & (dr > 0) & (err < pix_threshold) & (rel < rel_depth_threshold)
                total = total + np.where(cons, dr, 0.0)
                count[i] += cons
                diag[(i, m)] = dict(j=j, valid=valid, z=z, u=u, v=v, fx=fx, fy=fy, inside=inside, taps=taps,
                                    readable=readable, ds=ds, ub=ub, vb=vb, dr=dr, err=err, rel=rel, cons=cons)
            mask[i] = valid & (count[i] >= num_consistent)
            depth_avg[i] = np.where(mask[i], total / (count[i] + 1), 0.0)
            point[i] = np.where(mask[i][..., None], _lift(K[i], E[i], px, py, depth_avg[i]), 0.0)
    return count, depth_avg, mask, point, diag


def scene_scales(depths, K, E):
    """S, Z, R, ray, dmax of the module docstring."""
    V, h, w = depths.shape
    good = depths[depths > 0]
    dmin, dmax = float(good.min()), float(good.max())
    C = np.stack([-np.linalg.inv(E[i, :3, :3]) @ E[i, :3, 3] for i in range(V)])
    base = max(np.linalg.norm(C[i] - C[j]) for i in range(V) for j in range(V))
    disp = max(K[j, 0, 0] for j in range(V)) * base / dmin
    corners = np.array([[0.5, 0.5, 1.0], [w - 0.5, 0.5, 1.0], [0.5, h - 0.5, 1.0], [w - 0.5, h - 0.5, 1.0]])
    ray = max(np.linalg.norm(np.linalg.inv(K[i]) @ p) for i in range(V) for p in corners)
    return dict(S=w + disp, Z=dmax + base, R=dmax * ray + np.abs(C).max(), ray=ray, dmax=dmax)


def bands_and_ties(depths, K, E, diag, M, pix_threshold=1.0, rel_depth_threshold=0.01, depth_min=1e-3, depth_max=1e5, **_):
    """Per (i, m): the near-tie mask and e_dr (module docstring); the per-pixel tolerances; the largest bands."""
    V, h, w = depths.shape
    sc = scene_scales(depths, K, E)
    px, py = _centres(h, w)
    e_uv, e_w = 19 * EPS32 * sc["S"], 20 * EPS32 * sc["S"]

    def near_bound(t):
        return (np.abs(t - depth_min) <= 4 * EPS32 * depth_min) | (np.abs(t - depth_max) <= 4 * EPS32 * depth_max)

    own = near_bound(np.asarray(depths, np.float64))
    ties = {}
    tied_sources = np.zeros((V, h, w), np.int64)
    e_dr_max = np.zeros((V, h, w))
    worst = dict(tie_w=4 * e_w, tie_err=[], tie_rel=[])
    for (i, m), g in diag.items():
        with np.errstate(divide="ignore", invalid="ignore"):
            spread = g["taps"].max(axis=0) - g["taps"].min(axis=0)
            e_ds = 2 * spread * e_w + 8 * EPS32 * np.abs(g["taps"]).max(axis=0)
            prop_u, prop_v, prop_d = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
            for su in (-1, 1):
                for sv in (-1, 1):
                    for sd in (-1, 1):
                        ub, vb, dr = _drop(K[i], E[i], _lift(K[g["j"]], E[g["j"]], g["u"] + su * e_uv, g["v"] + sv * e_uv,
                                                             g["ds"] + sd * e_ds))
                        prop_u = np.fmax(prop_u, np.abs(ub - g["ub"]))
                        prop_v = np.fmax(prop_v, np.abs(vb - g["vb"]))
                        prop_d = np.fmax(prop_d, np.abs(dr - g["dr"]))
            e_dr = 9 * EPS32 * sc["Z"] + prop_d
            e_err = 2 * 19 * EPS32 * sc["S"] + prop_u + prop_v + 6 * EPS32 * g["err"] + EPS32 * pix_threshold
            e_rel = e_dr / depths[i].astype(np.float64) + 3 * EPS32 * g["rel"] + EPS32 * rel_depth_threshold
            t = np.abs(g["z"]) <= 4 * 9 * EPS32 * sc["Z"]
            near_image = (g["z"] > 0) & (g["fx"] > -1) & (g["fx"] < w) & (g["fy"] > -1) & (g["fy"] < h)
            t |= near_image & ((np.abs(g["fx"] - np.rint(g["fx"])) <= 4 * e_w) | (np.abs(g["fy"] - np.rint(g["fy"])) <= 4 * e_w))
            t |= g["inside"] & near_bound(g["taps"]).any(axis=0)
            t |= g["readable"] & (np.abs(g["dr"]) <= 4 * e_dr)
            t |= g["readable"] & (np.abs(g["err"] - pix_threshold) <= 4 * e_err)
            t |= g["readable"] & (np.abs(g["rel"] - rel_depth_threshold) <= 4 * e_rel)
        t = (t & g["valid"]) | own[i]
        ties[(i, m)] = t
        tied_sources[i] += t
        e_dr_max[i] = np.fmax(e_dr_max[i], np.where(g["readable"], e_dr, 0.0))
        worst["tie_err"].append(4 * e_err[g["readable"]])
        worst["tie_rel"].append(4 * e_rel[g["readable"]])
    tol_depth = 4 * (e_dr_max + (M + 1) * EPS32 * sc["dmax"])
    tol_point = 4 * 9 * EPS32 * sc["R"] + sc["ray"] * tol_depth
    for k in ("tie_err", "tie_rel"):
        both = np.concatenate(worst[k]) if worst[k] else np.zeros(1)
        worst[k], worst[k + "_median"] = float(both.max()), float(np.median(both))
    return ties, tied_sources, tol_depth, tol_point, worst


def tie_share(tied_sources, depths):
    valid = (depths > 1e-3) & (depths < 1e5)
    return [float(((tied_sources[i] > 0) & valid[i]).sum()) / max(int(valid[i].sum()), 1) for i in range(depths.shape[0])]


# ---------------------------------------------------------------------------------------------------------------------
# 1. CPU: the statement against a closed form, the tie share, the source table, the arguments, the missing CPU path
# ---------------------------------------------------------------------------------------------------------------------
def _two_camera_case():
    """Two fronto-parallel cameras (R = I) a baseline B = 6 apart along x, f = 100, both seeing the plane at depth 100: the
    disparity is f B / 100 = 6 pixels exactly.  View 1's principal point is a quarter pixel off view 0's in x and y, so
    pixel (x, y) of view 0 lands at fx = x - 6 + .25, fy = y + .25: every floor and border decision is clear, the taps are
    columns x - 6 and x - 5 with weights 3/4 and 1/4 (the rows are equal).  View 1 reports 100 up to column 23, then 100.2,
    from column 40 on 100.5 and from column 56 on 103.  A partner depth ds comes back at the pixel's own row, 600 / ds - 6
    pixels off in x, at depth d' = ds: the plane itself returns with error 0."""
    h, w, f, B = 6, 64, 100.0, 6.0
    K0 = np.array([[f, 0.0, 32.0], [0.0, f, 3.0], [0.0, 0.0, 1.0]])
    K1 = np.array([[f, 0.0, 32.25], [0.0, f, 3.25], [0.0, 0.0, 1.0]])
    E0 = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    E1 = np.concatenate([np.eye(3), np.array([[-B], [0.0], [0.0]])], 1)
    d1 = np.full((h, w), 100.0)
    d1[:, 24:] = 100.2
    d1[:, 40:] = 100.5
    d1[:, 56:] = 103.0
    return np.stack([np.full((h, w), 100.0), d1]), np.stack([K0, K1]), np.stack([E0, E1]), (h, w)


@pytest.mark.parametrize("pix_threshold", [1.0, 0.02])
def test_statement_matches_the_closed_form_of_two_fronto_parallel_cameras(pix_threshold):
    """Partner depths and what they give (pixel error |600 / ds - 6|, relative depth |ds - 100| / 100), all clear of the
    thresholds 1.0 or 0.02 pixels and 0.01: 100 -> (0, 0); 100.05 -> (.0030, .0005); 100.2 -> (.0120, .002); 100.275 ->
    (.0165, .00275); 100.5 -> (.0299, .005): fails 0.02 pixels only; 101.125 -> (.0667, .01125): fails the depth test only at
    1.0 pixel; 103 -> (.175, .03): fails the depth test, and the pixel test at 0.02."""
    D, K, E, (h, w) = _two_camera_case()
    count, depth_avg, mask, point, _ = statement(D, K, E, pix_threshold=pix_threshold, num_consistent=1)
    xs = np.arange(w)
    left, right = np.clip(xs - 6, 0, w - 1), np.clip(xs - 5, 0, w - 1)
    ds = 0.75 * D[1][0, left] + 0.25 * D[1][0, right]
    cons = (xs - 6 >= 0) & (np.abs(600.0 / ds - 6.0) < pix_threshold) & (np.abs(ds - 100.0) / 100.0 < 0.01)
    assert cons[6:30].all() and not cons[:6].any() and not cons[61:].any()       # both sides occur
    assert cons[45] and cons[50] == (pix_threshold == 1.0)                       # 100.275 passes; 100.5: the pixel test alone decides
    expect = np.broadcast_to(cons, (h, w)).copy()
    expect[h - 1] = False                                                        # fy = h - .75: the row below is outside
    assert np.array_equal(count[0], expect.astype(int)) and np.array_equal(mask[0], expect)
    want = np.where(expect, (100.0 + np.broadcast_to(ds, (h, w))) / 2.0, 0.0)
    assert np.abs(depth_avg[0] - want).max() < 1e-9
    ys = np.arange(h)
    X = np.stack(np.broadcast_arrays((xs[None, :] + 0.5 - 32.0) / 100.0 * want, (ys[:, None] + 0.5 - 3.0) / 100.0 * want, want), -1)
    assert np.abs(point[0] - X).max() < 1e-9
    assert statement(D, K, E, pix_threshold=pix_threshold, num_consistent=2)[2].sum() == 0     # one source: never two


def test_statement_tie_share_and_both_sides_of_the_thresholds():
    """The float64 statement alone with the derived bands on the committed scenes: at least 90 % of every view's valid
    pixels are left to the GPU comparison, and both sides of every decision occur."""
    for nv in (V5, 3):
        depths, K, E, _, _ = make_plane_scene(nv)
        count, _, mask, _, diag = statement(depths, K, E)
        _, tied_sources, tol_depth, tol_point, worst = bands_and_ties(depths, K, E, diag, nv - 1)
        shares = tie_share(tied_sources, depths)
        readable = np.stack([g["readable"] for g in diag.values()])
        fail_px = float((np.stack([g["err"] >= 1.0 for g in diag.values()]) & readable).sum()) / readable.sum()
        fail_rel = float((np.stack([g["rel"] >= 0.01 for g in diag.values()]) & readable).sum()) / readable.sum()
        kept = [float(mask[i].mean()) for i in range(nv)]
        print("V=%d bands %s tie shares %s fail px %.4f rel %.4f kept %s tol depth %.3g point %.3g" % (
            nv, {k: "%.3g" % v for k, v in worst.items()}, ["%.4f" % s for s in shares], fail_px, fail_rel,
            ["%.3f" % k for k in kept], tol_depth.max(), tol_point.max()))
        assert max(shares) <= TIE_CAP, shares
        assert 0.005 < fail_px < 0.3 and 0.005 < fail_rel < 0.3
        assert 0.3 < float(readable.mean()) < 1.0
        if nv == V5:
            assert all(0.1 < k < 0.6 for k in kept), kept
        else:
            assert not mask.any() and int(count.max()) == 2


def test_sources_from_pairs():
    from pointmvsnet_amd.geometric import sources_from_pairs
    words = "4  0 3 2 9.5 1 7.0 3 1.5  1 2 0 3.0 2 1.0  2 1 5 2.0  3 0".split()      # view 2 lists view 5, view 3 nothing
    table = sources_from_pairs(words, 4, 2)
    assert table.dtype == np.int32 and table.tolist() == [[2, 1], [0, 2], [-1, -1], [-1, -1]]
    assert sources_from_pairs(words, 4, 3).tolist() == [[2, 1, 3], [0, 2, -1], [-1, -1, -1], [-1, -1, -1]]
    assert sources_from_pairs(words, 6, 1).tolist() == [[2], [0], [5], [-1], [-1], [-1]]
    assert sources_from_pairs(words, 2, 2).tolist() == [[1, -1], [0, -1]]          # fewer views than the file: entries dropped
    assert sources_from_pairs(words, 3, 0).shape == (3, 0)
    with pytest.raises(ValueError):
        sources_from_pairs(words, 0, 2)
    # DTU's own layout (dataset.PAIR_WORDS = 22 words per entry): what DTUDataset reads at 22 p + 2 v + 3
    dtu = ["2"] + ["0", "10"] + sum([[str(k + 1), "1.0"] for k in range(10)], []) + ["1", "10"] + sum([[str(k), "1.0"] for k in range(10)], [])
    assert sources_from_pairs(dtu, 2, 10)[0].tolist() == [1] + [-1] * 9
    assert [int(dtu[22 * 1 + 2 * v + 3]) for v in range(3)] == [0, 1, 2]


def test_geometric_refuses_bad_arguments():
    from pointmvsnet_amd import geometric
    depths, K, E, _, _ = make_plane_scene(3, h=SMALL[0], w=SMALL[1])
    d = torch.from_numpy(depths)
    for bad in (np.zeros((3, 2)), np.zeros((2, 2), int), np.zeros(3, int), [[3, 0], [0, 1], [1, 0]], [[-2, 0], [0, 1], [1, 0]],
                torch.zeros(3, 2), torch.zeros(3, 2, dtype=torch.bool)):
        with pytest.raises(ValueError, match="sources"):
            geometric.geometric_filter(d, K, E, sources=bad)
    with pytest.raises(ValueError, match="different sizes"):
        geometric.geometric_filter([depths[0], depths[1][:, :-1]], K[:2], E[:2])
    with pytest.raises(ValueError, match=r"\(V, h, w\)"):
        geometric.geometric_filter(d[0], K, E)
    with pytest.raises(ValueError, match="num_consistent"):
        geometric.geometric_filter(d, K, E, num_consistent=0)


def test_geometric_has_no_cpu_path():
    from pointmvsnet_amd import geometric, scan
    depths, K, E, _, _ = make_plane_scene(3, h=SMALL[0], w=SMALL[1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometric.geometric_filter(torch.from_numpy(depths), K, E)
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometric.geometric_filter(torch.from_numpy(depths), K, E, sources=TABLE[:3] % 3)
    acc = scan.ScanAccumulator(2)
    with pytest.raises(ValueError, match="have not been added"):
        acc.geometric()
    with pytest.raises(ValueError, match="method"):
        acc.fuse(method="fusibile")


def test_source_maps_reproduce_both_projections():
    """The composed float32 matrices of a listed pair describe the way there and the way back (to float32)."""
    from pointmvsnet_amd import fusion, geometric
    depths, K, E, _, _ = make_plane_scene(3, h=SMALL[0], w=SMALL[1])
    table = np.array([[2, -1], [1, 0], [0, 1]], np.int32)
    maps = geometric.source_maps(K, E, table).astype(np.float64)
    assert maps.shape == (3, 2, 2, fusion.PAIR_FLOATS)
    assert not maps[0, 1].any() and not maps[1, 0].any()                          # the pad and the view itself
    p, d = np.array([17.5, 23.5, 1.0]), 611.0
    X = _lift(K[0], E[0], np.float64(17.5), np.float64(23.5), np.float64(d))
    u, v, z = _drop(K[2], E[2], X)
    fwd, back = maps[0, 0, 0], maps[0, 0, 1]
    assert np.allclose(fwd[:9].reshape(3, 3) @ p * d + fwd[9:12], np.array([u * z, v * z, z]), rtol=1e-5)
    q = back[:9].reshape(3, 3) @ np.array([u, v, 1.0]) * z + back[9:12]           # back at the depth it was seen at
    assert np.allclose(q, p * d, rtol=1e-5)
    assert np.array_equal(geometric.view_maps_of(K, E), fusion.camera_maps(K, E)[0])


def test_source_maps_are_the_pair_maps_of_the_fusion():
    """One composition serves both fusers: a listed pair's two rows are, byte for byte, the ``i -> j`` and ``j -> i``
    entries of ``fusion.camera_maps`` without the disparity scale; pads and a row naming itself stay zero."""
    from pointmvsnet_amd import fusion, geometric
    for scene, tables in ((make_plane_scene(V5), (None, TABLE)), (make_plane_scene(3, h=SMALL[0], w=SMALL[1]), (None, TABLE[:3] % 3))):
        _, K, E, _, _ = scene
        V = K.shape[0]
        view, pair = fusion.camera_maps(K, E)
        assert geometric.view_maps_of(K, E).tobytes() == view.tobytes()
        for table in tables:
            if table is None:
                table = np.array([[j for j in range(V) if j != i] for i in range(V)])
            src = geometric.source_maps(K, E, table)
            assert src.dtype == np.float32 and src.shape == table.shape + (2, fusion.PAIR_FLOATS)
            assert not src[..., 12:].any()
            listed = 0
            for i in range(V):
                for m, j in enumerate(table[i]):
                    if j < 0 or j == i:
                        assert not src[i, m].any()
                        continue
                    listed += 1
                    assert src[i, m, 0, :12].tobytes() == pair[i, j, :12].tobytes()
                    assert src[i, m, 1, :12].tobytes() == pair[j, i, :12].tobytes()
                    assert src[i, m, 0, :12].any() and pair[i, j, 12] > 0
            assert listed == int(((table >= 0) & (table != np.arange(V)[:, None])).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. GPU
# ---------------------------------------------------------------------------------------------------------------------
def _run(dev, depths, K, E, images=None, **kw):
    from pointmvsnet_amd import geometric
    out = geometric.geometric_filter(torch.from_numpy(depths).to(dev), K, E,
                                     images=None if images is None else torch.from_numpy(images).to(dev),
                                     return_stages=True, **kw)
    depth_avg, mask, count, points, colours, stages = out
    assert depth_avg.device == mask.device == count.device == points.device == torch.from_numpy(depths).to(dev).device
    return dict(depth_avg=depth_avg.cpu(), mask=mask.cpu(), count=count.cpu(), points=points.cpu(),
                colours=None if colours is None else colours.cpu(), point=stages["point"].cpu(), emit=stages["emit"].cpu())


@pytest.fixture(scope="module")
def scene5():
    return make_plane_scene(V5)


@pytest.fixture(scope="module")
def run5(dev, scene5):
    depths, K, E, images, _ = scene5
    return _run(dev, depths, K, E, images)


def _compare(name, got, depths, K, E, sources=None, **kw):
    """The kernel's outputs against the statement by the rules of the module docstring; returns the statement's count."""
    params = dict(DEFAULTS, **kw)
    V = depths.shape[0]
    M = V - 1 if sources is None else len(sources[0])
    count, depth_avg, mask, point, diag = statement(depths, K, E, sources=sources, **params)
    ties, tied_sources, tol_depth, tol_point, worst = bands_and_ties(depths, K, E, diag, M, **params)
    shares = tie_share(tied_sources, depths)
    g_count = got["count"].numpy().astype(np.int64)
    g_mask = got["mask"].numpy()
    g_depth, g_point = got["depth_avg"].numpy().astype(np.float64), got["point"].numpy().astype(np.float64)
    clean = tied_sources == 0
    differ = g_count != count
    depth_err = np.abs(g_depth - depth_avg)
    point_err = np.abs(g_point - point).max(axis=-1)
    values = dict(tie_w=worst["tie_w"], tie_err_max=worst["tie_err"], tie_err_median=worst["tie_err_median"],
                  tie_rel_max=worst["tie_rel"], tie_rel_median=worst["tie_rel_median"], worst_tie_share=max(shares),
                  tied_pixels=int((~clean).sum()), count_differs_in_tied_pixels=int(differ[~clean].sum()),
                  count_differs_outside_ties=int(differ[clean].sum()), depth_err_max=float(depth_err[clean].max()),
                  tol_depth_max=float(tol_depth.max()), point_err_max=float(point_err[clean].max()),
                  tol_point_max=float(tol_point.max()), depth_err_over_tol_max=float((depth_err / tol_depth)[clean].max()),
                  point_err_over_tol_max=float((point_err / tol_point)[clean].max()), kept_share=float(g_mask.mean()))
    print(name, values)
    report(name, **values)
    assert max(shares) <= TIE_CAP, shares
    assert np.array_equal(g_count[clean], count[clean])
    assert (np.abs(g_count - count) <= tied_sources).all()                      # a tied source moves count by at most one
    assert np.array_equal(g_mask, g_count >= params["num_consistent"])          # exactly, everywhere
    assert np.array_equal(got["emit"].numpy().astype(bool), g_mask)
    assert (g_depth[~g_mask] == 0).all() and (g_point[~g_mask] == 0).all()
    assert (depth_err[clean] <= tol_depth[clean]).all(), float((depth_err - tol_depth)[clean].max())
    assert (point_err[clean] <= tol_point[clean]).all(), float((point_err - tol_point)[clean].max())
    invalid = ~((depths > 1e-3) & (depths < 1e5))
    assert (g_count[invalid] == 0).all() and not g_mask[invalid].any()
    return count


@pytest.mark.gpu
def test_kernel_matches_the_float64_statement(dev, scene5, run5):
    """Tolerances and the near-tie rule: module docstring.  Measured worst cases go to parity_report.jsonl."""
    depths, K, E, _, _ = scene5
    _compare("geometric_kernel", run5, depths, K, E)
    assert 0.1 < float(run5["mask"].float().mean()) < 0.6


@pytest.mark.gpu
def test_kernel_matches_the_statement_on_odd_sizes(dev):
    """V = 3 at 37 x 53: partial tiles in both directions and the x0 + 1 <= w - 1 edge at an odd width.  Three views never
    reach three sources, so two are asked for."""
    depths, K, E, images, _ = make_plane_scene(3, h=SMALL[0], w=SMALL[1])
    got = _run(dev, depths, K, E, images, num_consistent=2)
    _compare("geometric_kernel_odd", got, depths, K, E, num_consistent=2)
    assert got["mask"].any() and not _run(dev, depths, K, E, images)["mask"].any()
    # the last column and row can never be the top-left tap, yet they are read as the other three
    _, _, _, _, diag = statement(depths, K, E, num_consistent=2)
    assert any(((np.floor(g["fx"]) == SMALL[1] - 2) & g["readable"]).any() for g in diag.values())


@pytest.mark.gpu
def test_source_table_is_honoured(dev, scene5, run5):
    """M = 2 on V = 5 with one pad and one entry naming the view itself: equal to the statement on that table, and different
    from the all-views result, so the comparison cannot pass by ignoring ``sources``."""
    depths, K, E, images, _ = scene5
    got = _run(dev, depths, K, E, images, sources=TABLE, num_consistent=1)
    count = _compare("geometric_sources", got, depths, K, E, sources=TABLE.tolist(), num_consistent=1)
    assert int(got["count"][0].max()) == 1 and int(got["count"][1].max()) == 1 and int(got["count"][2].max()) == 2
    every = _run(dev, depths, K, E, images, num_consistent=1)
    assert not torch.equal(every["count"], got["count"]) and int(every["count"].max()) == 4
    assert int((every["count"].numpy() != count).sum()) > 0.2 * count.size
    same = _run(dev, depths, K, E, images, sources=torch.from_numpy(TABLE).to(dev), num_consistent=1)      # a device tensor
    assert torch.equal(same["count"], got["count"]) and torch.equal(same["points"], got["points"])


@pytest.mark.gpu
def test_ordered_compaction_teacher_forced(dev, scene5, run5):
    """On the GPU's own mask: points = point[mask] view-major then row-major, the colours are the pixels' own, two calls
    give identical bytes; without images None comes back; return_points=False returns the three maps alone."""
    from pointmvsnet_amd import geometric
    depths, K, E, images, _ = scene5
    mask = run5["mask"]
    assert int(mask.sum()) > 0 and run5["points"].dtype == torch.float32 and run5["colours"].dtype == torch.uint8
    assert torch.equal(run5["points"], run5["point"][mask])
    assert torch.equal(run5["colours"], torch.from_numpy(images)[mask])
    again = _run(dev, depths, K, E, images)
    for k in ("depth_avg", "mask", "count", "points", "colours", "point"):
        assert again[k].numpy().tobytes() == run5[k].numpy().tobytes(), k
    plain = _run(dev, depths, K, E, None)
    assert plain["colours"] is None and torch.equal(plain["points"], run5["points"])
    three = geometric.geometric_filter(torch.from_numpy(depths).to(dev), K, E, return_points=False)
    assert len(three) == 3 and torch.equal(three[0].cpu(), run5["depth_avg"]) and three[1].dtype == torch.bool
    assert three[2].dtype == torch.int32
    report("geometric_compaction", points=int(mask.sum()), kept_share=float(mask.float().mean()))


@pytest.mark.gpu
def test_scan_layer_routes_both_methods(dev):
    """ScanAccumulator on the ``tiny`` synthetic scene (the model's own, untrained predictions, so the thresholds are loose
    enough for a cloud): fuse(method="roundtrip") is geometric_filter on filtered() / cameras() / images(), geometric()
    returns its five values, and method="disparity" is today's fuse() bit for bit."""
    from pointmvsnet_amd import geometric, scan as S
    from pointmvsnet_amd.fusion import fuse_depth_maps
    from test_scan import FUSE, NAME, _model, scan_batches
    batches, img_scales, inter_scales = scan_batches(dev)
    net = _model(dev)
    acc = S.ScanAccumulator(len(batches), name=NAME, mode="NEAREST")
    with torch.no_grad():
        for batch, _ in batches:
            acc.add(batch, net(batch, img_scales, inter_scales, isFlow=True, isTest=True))
    loose = dict(pix_threshold=50.0, rel_depth_threshold=0.5, num_consistent=1)
    K, E = acc.cameras()
    want = geometric.geometric_filter(acc.filtered(), K, E, images=acc.images(), **loose)
    pts, col = acc.fuse(method="roundtrip", **loose)
    assert pts.shape[0] > 0 and pts.cpu().numpy().tobytes() == want[3].cpu().numpy().tobytes() and torch.equal(col, want[4])
    five = acc.geometric(**loose)
    assert len(five) == 5 and all(torch.equal(a, b) for a, b in zip(five, want))
    assert five[0].shape == acc.filtered().shape and int(five[1].sum()) == pts.shape[0]
    table = np.array([[1], [2], [0]])
    one = acc.fuse(method="roundtrip", sources=table, **loose)
    assert torch.equal(one[0], geometric.geometric_filter(acc.filtered(), K, E, images=acc.images(), sources=table, **loose)[3])
    assert 0 < one[0].shape[0] <= pts.shape[0]
    today = fuse_depth_maps(acc.filtered(), K, E, images=acc.images(), **FUSE)
    for got in (acc.fuse(**FUSE), acc.fuse(method="disparity", **FUSE)):
        assert got[0].cpu().numpy().tobytes() == today[0].cpu().numpy().tobytes() and torch.equal(got[1], today[1])
    with pytest.raises(TypeError):
        acc.fuse(sources=table, **FUSE)
    report("geometric_scan_layer", points=int(pts.shape[0]), disparity_points=int(today[0].shape[0]))
