"""Photometric consistency (pointmvsnet_amd/photometric.py, csrc/photo_filter.hip): windowed ZNCC of depth maps.

The yardstick is ``statement`` below: the module docstring written out in NumPy, operation by operation, once in float32
(what the kernel must return bit for bit) and once in float64.  It shares no code with the product; the float32 pair rows it
reads are ``geometric.source_maps``', which ``test_geometric`` checks on their own and one test here composes again.

How far the two statements may differ (``bounds``)
--------------------------------------------------
``u = 2^-24`` is float32's unit roundoff; everything is to first order in ``u``.  Per tap, each of ``qx``, ``qy``, ``z`` is
``(m0 px + m1 py + m2) d + m9``: with ``a = m0 px``, ``b = m1 py`` and ``l = a + b + m2`` its six roundings add up to at most
``u A``, ``A = (|a| + |b| + |a + b| + |l|) d + |l d| + |l d + m9|`` (the running error, operation by operation).  ``rz`` and
the product add ``2 u`` relative, the subtraction of one half another ``u (|U| + 1)``, so

    e_x = u (A_x / z + |U| (A_z / z + 3) + 1),  U = qx / z,   likewise e_y

bounds the error of ``fx``.  The bilinear value moves by at most ``g_x e_x + g_y e_y`` with ``g_x``, ``g_y`` the larger of
the two horizontal (vertical) differences of the tap's four bytes, and its own seven roundings and the subtraction of ``c``
add ``8 u 255``: that is ``e_s`` per tap, ``E = sqrt(sum e_s^2)`` per window.  With ``s~`` the centred window,
``|s~| = sqrt(VS / n)`` and ``ncc = <R~, s~> / (|R~| |s~|)``: a perturbation ``delta`` of ``s`` moves the normalised vector
by at most ``2 |delta| / |s~|`` and ``R~`` is exact, so the samples contribute ``2 E sqrt(n / VS)``.  The one-pass sums add
their own roundings: ``n + 2`` operations on terms of size ``n S2 + S1^2`` in ``VS`` and ``n sum|R s| + |SR S1|`` in ``COV``,
then the product, square root, division: ``(n + 3) u ((n sum|R s| + |SR S1|) / sqrt(VR VS) + (n S2 + S1^2) / (2 VS)) + 4 u``.

    bound = 2 E sqrt(n / VS) + (n + 3) u (...) + 4 u                      evaluated on the float64 statement

Measured on the scene below (r = 2, all 28207 usable pairs): largest |ncc32 - ncc64| 6.6e-6, smallest bound 2.3e-5, largest
error / bound 0.054.  The bound is a worst case over 25 taps whose errors do not add up in one direction.

Near-tie bands (a pair is *tied* when a decision of either statement could flip inside the errors above, times ``TIE`` = 2
for the terms of second order): a tap with ``fx`` or ``fy`` within ``TIE e`` of an integer or ``|z| <= TIE u A_z``;
``|VS - var_min| <= TIE (2 E sqrt(n VS) + (n + 2) u (n S2 + S1^2))``; ``|ncc - threshold| <= TIE bound``.  Measured: 14 to 29
tied pairs per view of 4967 to 6467 usable ones, at most 0.45 %.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import report
from pointmvsnet_amd import synthetic

U32 = 2.0 ** -24
TIE = 2.0                 # the bands are first-order worst cases; the factor covers the terms of second order many times over
H, W, V5 = 48, 64, 5
SMALL = (37, 53)
ZERO_BLOCK = (slice(6, 14), slice(10, 22))
OUTLIER_BLOCK = (slice(26, 40), slice(34, 54))
PAIRS = [(0, 1), (0, 4), (2, 4)]
TEXTURE = [(7.0, -50.0), (5.0, 20.0), (12.0, 60.0)]       # (period in pixel footprints, direction on the plane in degrees)
DEFAULTS = dict(radius=2, min_variance=25.0, ncc_threshold=0.6, num_consistent=2, depth_min=1e-3, depth_max=1e5)


# ---------------------------------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_scene(num_view=V5, h=H, w=W, seed=0, blocks=True):
    """Cameras of synthetic.make_scene, the tilted world plane of test_fusion.make_plane_scene (depth 600 on view 0's axis),
    every view's depth map by exact ray-plane intersection, then a block of zeros and a block multiplied by 1.3.  Every view's
    image is rendered from ONE world texture on the plane: per channel three sinusoids with periods of 7, 5 and 12 pixel
    footprints, rounded to uint8.  Their three directions on the plane (``TEXTURE``) differ from each other and from the
    cameras' baselines, so that no displacement along a baseline leaves a sinusoid where it was."""
    cams = synthetic.make_scene(h, w, num_view, 48, seed=seed)["cam_params_list"][0]
    E = cams[:, 0, :3, :4].double().numpy()
    K = cams[:, 1, :3, :3].double().numpy()
    R, t = E[:, :, :3], E[:, :, 3]
    n = R[0].T @ np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    c = n @ (np.linalg.inv(R[0]) @ (np.array([0.0, 0.0, 600.0]) - t[0]))
    e1 = np.cross(n, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    foot = 600.0 / K[0, 0, 0]                                       # one pixel's footprint on the plane
    ys, xs = np.mgrid[0:h, 0:w]
    pix = np.stack([xs + 0.5, ys + 0.5, np.ones_like(xs, float)], -1).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0, 2 * np.pi, (3, 3))
    depths, images = [], []
    for i in range(num_view):
        ray = pix @ np.linalg.inv(K[i]).T
        d = (c + n @ (np.linalg.inv(R[i]) @ t[i])) / (ray @ (R[i] @ n))       # n . (R^-1 (ray d - t)) = c
        X = (ray * d[:, None] - t[i]) @ np.linalg.inv(R[i]).T
        a, b = X @ e1, X @ e2
        img = np.empty((h * w, 3))
        for ch in range(3):
            waves = [np.sin(2 * np.pi * (a * np.cos(np.deg2rad(ang)) + b * np.sin(np.deg2rad(ang))) / (period * foot)
                            + phase[ch, k]) for k, (period, ang) in enumerate(TEXTURE)]
            img[:, ch] = 128 + 38 * sum(waves)
        images.append(np.rint(np.clip(img, 0, 255)).astype(np.uint8).reshape(h, w, 3))
        d = d.reshape(h, w).copy()
        if blocks:
            d[ZERO_BLOCK] = 0.0
            d[OUTLIER_BLOCK] *= 1.3
        depths.append(d.astype(np.float32))
    out = np.stack(depths), K, E, np.stack(images), cams
    for a in out[:4]:
        a.setflags(write=False)
    return out


def grey_formula(images):
    c = images.astype(np.int64)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def table_of(sources, V):
    if sources is None:
        return np.array([[j for j in range(V) if j != i] for i in range(V)], np.int32).reshape(V, max(V - 1, 0))
    return np.asarray(sources, np.int32)


def pair_rows(K, E, table):
    from pointmvsnet_amd import geometric
    return geometric.source_maps(K, E, table)[:, :, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def statement(depths, grey, rows, table, radius=2, min_variance=25.0, ncc_threshold=0.6, num_consistent=2, depth_min=1e-3,
              depth_max=1e5, dtype=np.float32, diagnose=False):
    """The module docstring of photometric.py in NumPy, every floating-point operation in ``dtype``.  ``rows`` (V, M, 16)
    float32 pair rows.  Returns a dict of ncc (V, M, h, w), score, count, usable, mask, scorable and, ``diagnose``, per pair
    the quantities of this file's docstring."""
    f = dtype
    V, h, w = depths.shape
    M = table.shape[1]
    r = int(radius)
    n = (2 * r + 1) ** 2
    var_min = int(np.ceil(n * n * float(min_variance)))
    out = {"ncc": np.full((V, M, h, w), np.nan, f), "score": np.zeros((V, h, w), f), "count": np.zeros((V, h, w), np.int32),
           "usable": np.zeros((V, h, w), np.int32), "mask": np.zeros((V, h, w), bool), "scorable": np.zeros((V, h, w), bool)}
    names = ("bound", "tie", "z_behind", "off_image")
    diag = {k: np.zeros((V, M, h, w), bool if k != "bound" else np.float64) for k in names} if diagnose else None
    if h < 2 * r + 1 or w < 2 * r + 1:
        return (out, diag) if diagnose else out
    inner = (slice(r, h - r), slice(r, w - r))
    ys, xs = np.mgrid[r:h - r, r:w - r]
    one, half = f(1.0), f(0.5)
    for i in range(V):
        g = grey[i].astype(np.int64)
        c = g[inner]
        SR, SRR = np.zeros_like(c), np.zeros_like(c)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                R = g[r + dy:h - r + dy, r + dx:w - r + dx] - c
                SR += R
                SRR += R * R
        VR = n * SRR - SR * SR
        d = depths[i][inner].astype(f)
        scorable = (d > f(np.float32(depth_min))) & (d < f(np.float32(depth_max))) & (VR >= var_min)
        out["scorable"][i][inner] = scorable
        total = np.zeros(c.shape, f)
        used = np.zeros(c.shape, np.int32)
        good = np.zeros(c.shape, np.int32)
        for m in range(M):
            j = int(table[i, m])
            if j < 0 or j == i:
                continue
            row = rows[i, m].astype(f)
            gj = grey[j]
            S1, S2, SX = np.zeros(c.shape, f), np.zeros(c.shape, f), np.zeros(c.shape, f)
            inside_all = np.ones(c.shape, bool)
            if diagnose:
                E2, SAX, tie, behind = np.zeros(c.shape), np.zeros(c.shape), np.zeros(c.shape, bool), np.zeros(c.shape, bool)
            with np.errstate(all="ignore"):
                for dy in range(-r, r + 1):
                    py = (ys + dy).astype(f) + half
                    for dx in range(-r, r + 1):
                        R = g[r + dy:h - r + dy, r + dx:w - r + dx] - c
                        px = (xs + dx).astype(f) + half
                        qx = (row[0] * px + row[1] * py + row[2]) * d + row[9]
                        qy = (row[3] * px + row[4] * py + row[5]) * d + row[10]
                        z = (row[6] * px + row[7] * py + row[8]) * d + row[11]
                        rz = one / z
                        u, v = qx * rz, qy * rz
                        fx, fy = u - half, v - half
                        x0, y0 = np.floor(fx), np.floor(fy)
                        inside = (z > 0) & (x0 >= 0) & (x0 + one <= f(w - 1)) & (y0 >= 0) & (y0 + one <= f(h - 1))
                        inside_all &= inside
                        xi = np.where(inside, x0, 0).astype(np.int64)
                        yi = np.where(inside, y0, 0).astype(np.int64)
                        t00, t01 = gj[yi, xi].astype(f), gj[yi, xi + 1].astype(f)
                        t10, t11 = gj[yi + 1, xi].astype(f), gj[yi + 1, xi + 1].astype(f)
                        wx, wy = fx - x0, fy - y0
                        top = t00 * (one - wx) + t01 * wx
                        bot = t10 * (one - wx) + t11 * wx
                        s = (top * (one - wy) + bot * wy) - c.astype(f)
                        S1 = S1 + s
                        S2 = S2 + s * s
                        SX = SX + R.astype(f) * s
                        if diagnose:
                            # the running error of (m0 px + m1 py + m2) d + m9, operation by operation
                            A = []
                            for k in range(3):
                                a, b = row[3 * k] * px, row[3 * k + 1] * py
                                lin = a + b + row[3 * k + 2]
                                A.append((np.abs(a) + np.abs(b) + np.abs(a + b) + np.abs(lin)) * d + np.abs(lin * d)
                                         + np.abs(lin * d + row[9 + k]))
                            ex = U32 * (A[0] / z + np.abs(u) * (A[2] / z + 3) + 1)
                            ey = U32 * (A[1] / z + np.abs(v) * (A[2] / z + 3) + 1)
                            gx = np.maximum(np.abs(t01 - t00), np.abs(t11 - t10))
                            gy = np.maximum(np.abs(t10 - t00), np.abs(t11 - t01))
                            E2 += (gx * ex + gy * ey + 8 * U32 * 255) ** 2
                            SAX += np.abs(R * s)
                            near = (np.abs(fx - np.rint(fx)) <= TIE * ex) | (np.abs(fy - np.rint(fy)) <= TIE * ey) | \
                                   (np.abs(z) <= TIE * U32 * A[2])
                            tie |= near & scorable
                            behind |= ~(z > 0)
                nf = f(n)
                VS = nf * S2 - S1 * S1
                COV = nf * SX - SR.astype(f) * S1
                ok = scorable & inside_all & (VS >= f(var_min))
                val = np.minimum(one, np.maximum(-one, COV / np.sqrt(VR.astype(f) * VS)))
                if diagnose:
                    Eall = np.sqrt(E2)
                    sums = n * S2 + S1 * S1
                    bound = 2 * Eall * np.sqrt(n / VS) + (n + 3) * U32 * ((n * SAX + np.abs(SR * S1)) / np.sqrt(VR * VS)
                                                                         + sums / (2 * VS)) + 4 * U32
                    tie |= scorable & inside_all & (np.abs(VS - var_min) <= TIE * (2 * Eall * np.sqrt(n * np.abs(VS))
                                                                                 + (n + 2) * U32 * sums))
                    tie |= ok & (np.abs(val - ncc_threshold) <= TIE * bound)
                    diag["bound"][i, m][inner] = np.where(ok, bound, 0.0)
                    diag["tie"][i, m][inner] = tie
                    diag["z_behind"][i, m][inner] = behind & scorable
                    diag["off_image"][i, m][inner] = scorable & ~inside_all
            total = np.where(ok, total + val, total)
            used += ok
            good += ok & (val >= f(np.float32(ncc_threshold)))
            out["ncc"][i, m][inner] = np.where(ok, val, f(np.nan))
        with np.errstate(all="ignore"):
            out["score"][i][inner] = np.where(used > 0, total / used.astype(f), f(0.0))
        out["count"][i][inner] = good
        out["usable"][i][inner] = used
        out["mask"][i][inner] = scorable & (good >= num_consistent)
    return (out, diag) if diagnose else out


@functools.lru_cache(maxsize=None)
def scene_statements(h=H, w=W, radius=2):
    """The scene, its table of all pairs and both statements -- computed once, shared, never written to."""
    depths, K, E, images, _ = make_scene(V5, h, w)
    table = table_of(None, V5)
    rows = pair_rows(K, E, table)
    grey = grey_formula(images)
    kw = dict(DEFAULTS, radius=radius)
    st32 = statement(depths, grey, rows, table, dtype=np.float32, **kw)
    st64, diag = statement(depths, grey, rows, table, dtype=np.float64, diagnose=True, **kw)
    return st32, st64, diag, table


def slot_of(table, i, j):
    return int(np.nonzero(table[i] == j)[0][0])


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_pair_rows_are_the_composed_projection():
    """The float32 rows the statements read map a pixel at a depth as K_j (R_j X + t_j) does, composed here on its own."""
    depths, K, E, _, _ = make_scene()
    rows = pair_rows(K, E, table_of(None, V5)).astype(np.float64)
    for i, j in PAIRS:
        row = rows[i, slot_of(table_of(None, V5), i, j)]
        p, d = np.array([17.5, 23.5, 1.0]), 611.0
        X = np.linalg.inv(E[i, :, :3]) @ (np.linalg.inv(K[i]) @ p * d - E[i, :, 3])
        want = K[j] @ (E[j, :, :3] @ X + E[j, :, 3])
        got = (row[:9].reshape(3, 3) @ p) * d + row[9:12]
        assert np.allclose(got, want, rtol=1e-5)


def test_statements_agree_within_the_derived_bound():
    st32, st64, diag, table = scene_statements()
    both = ~np.isnan(st32["ncc"]) & ~np.isnan(st64["ncc"])
    assert both.sum() > 5000
    err = np.abs(st32["ncc"].astype(np.float64) - st64["ncc"])[both]
    bound = diag["bound"][both]
    print("pairs", int(both.sum()), "largest |ncc32 - ncc64|", err.max(), "smallest bound", bound.min(), "largest ratio",
          (err / bound).max())
    assert np.all(err <= bound)


def test_decisions_agree_outside_the_near_tie_bands():
    st32, st64, diag, table = scene_statements()
    free = ~diag["tie"]
    u32, u64 = ~np.isnan(st32["ncc"]), ~np.isnan(st64["ncc"])
    assert np.array_equal(st32["scorable"], st64["scorable"])                  # exact integers
    assert np.array_equal(u32[free], u64[free])
    with np.errstate(invalid="ignore"):
        assert np.array_equal((st32["ncc"] >= np.float32(0.6))[free], (st64["ncc"] >= np.float32(0.6))[free])
    # where no pair of a pixel is tied, the per-pixel outputs are the same decisions
    clear = free.all(axis=1)
    for k in ("count", "usable", "mask"):
        assert np.array_equal(st32[k][clear], st64[k][clear])
    for i in range(V5):
        usable, tied = int(u64[i].sum()), int((diag["tie"][i] & u64[i]).sum())
        print("view", i, "usable pairs", usable, "tied", tied)
        assert usable > 0 and tied <= 0.01 * usable


def test_true_depths_correlate_and_gross_outliers_do_not():
    """At the true depth every usable ncc is at least 0.8; in the block at depth x 1.3 no usable ncc reaches 0.8."""
    st32, _, _, table = scene_statements()
    block = np.zeros((H, W), bool)
    block[OUTLIER_BLOCK] = True
    for i, j in PAIRS:
        ncc = st32["ncc"][i, slot_of(table, i, j)]
        true, wrong = ncc[~block & ~np.isnan(ncc)], ncc[block & ~np.isnan(ncc)]
        print("pair", (i, j), "true: n", true.size, "min", true.min(), "median", np.median(true), "| x 1.3: n", wrong.size,
              "max", wrong.max() if wrong.size else None)
        assert true.size > 300 and true.min() >= 0.8
        assert not (wrong >= 0.8).any()
    # the filter's decision follows: the outlier block keeps a smaller share of its pixels than the rest of the maps
    print("kept share: x 1.3 block", st32["mask"][:, block].mean(), "elsewhere", st32["mask"][:, ~block].mean())
    assert st32["mask"][:, block].mean() < st32["mask"][:, ~block].mean()


def test_bad_arguments_raise_before_a_gpu_is_asked_for():
    from pointmvsnet_amd import photometric, scan
    depths, K, E, images, _ = make_scene()
    d, im = torch.from_numpy(depths.copy()), torch.from_numpy(images.copy())
    run = photometric.photometric_consistency
    for kw in (dict(radius=0), dict(radius=6), dict(radius=1.5), dict(min_variance=0.0), dict(min_variance=-1.0),
               dict(min_variance=1e6), dict(ncc_threshold=1.5), dict(num_consistent=0), dict(depth_min=2.0, depth_max=1.0),
               dict(depth_min=-1.0), dict(sources=np.zeros((V5, 2))), dict(sources=np.zeros((3, 2), np.int32)),
               dict(sources=np.full((V5, 1), V5, np.int32)), dict(sources=np.full((V5, 1), -2, np.int32))):
        with pytest.raises(ValueError):
            run(d, im, K, E, **kw)
        with pytest.raises(ValueError):
            photometric.photometric_filter(d, im, K, E, **kw)
    with pytest.raises(ValueError):
        run(d[0], im, K, E)
    with pytest.raises(ValueError):
        run(d, None, K, E)
    with pytest.raises(ValueError):
        run(d, im[:, :-1], K, E)
    with pytest.raises(ValueError):
        run(d, im.float(), K, E)
    with pytest.raises(ValueError):
        run(d, im, K[:3], E[:3])
    with pytest.raises(ValueError):
        run(d, im, K[:, :2], E)
    for bad in (images, im.float(), im[..., :2], im[0]):
        with pytest.raises(ValueError):
            photometric.grey_images(bad)
    with pytest.raises(TypeError):
        scan.ScanAccumulator(2).fuse(photo="radius=2")


def test_var_min_is_the_integer_of_the_docstring():
    from pointmvsnet_amd import photometric
    assert photometric._settings("t", 2, 25.0, 0.6, 2, 1e-3, 1e5) == (2, 15625)
    assert photometric._settings("t", 1, 20.0, 0.6, 2, 1e-3, 1e5) == (1, 1620)
    assert photometric._settings("t", 5, 0.001, 0.6, 2, 1e-3, 1e5) == (5, 15)           # ceil(14.641)
    assert photometric._settings("t", 5, 65025.0, 0.6, 2, 1e-3, 1e5)[1] < 2 ** 31


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _run(dev, depths, images, K, E, **kw):
    from pointmvsnet_amd import photometric
    out = photometric.photometric_consistency(torch.from_numpy(np.ascontiguousarray(depths)).to(dev),
                                              torch.from_numpy(np.ascontiguousarray(images)).to(dev), K, E, **kw)
    names = ("score", "mask", "count", "usable", "ncc")
    return {k: t.cpu().numpy() for k, t in zip(names, out)}


def _check(got, want, what=""):
    """Every output equal to the float32 statement's, bit for bit (``ncc`` with its NaNs)."""
    assert got["score"].dtype == np.float32 and got["count"].dtype == np.int32 and got["usable"].dtype == np.int32
    assert got["mask"].dtype == bool and got["ncc"].dtype == np.float32 and got["ncc"].shape == want["ncc"].shape
    assert np.array_equal(np.isnan(got["ncc"]), np.isnan(want["ncc"])), what
    live = ~np.isnan(want["ncc"])
    off = int((got["ncc"].view(np.uint32) != want["ncc"].view(np.uint32))[live].sum())
    off_score = int((got["score"].view(np.uint32) != want["score"].view(np.uint32)).sum())
    print(what, "usable pairs", int(live.sum()), "ncc off the statement", off, "scores off", off_score)
    assert off == 0 and off_score == 0, what
    for k in ("count", "usable", "mask"):
        assert np.array_equal(got[k], want[k]), (what, k)


def _case(dev, depths, images, K, E, sources, what, **kw):
    kw = dict(DEFAULTS, **kw)
    V = depths.shape[0]
    table = table_of(sources, V)
    want, diag = statement(depths, grey_formula(images), pair_rows(K, E, table), table, dtype=np.float32, diagnose=True, **kw)
    got = _run(dev, depths, images, K, E, sources=sources, return_per_source=True, **kw)
    _check(got, want, what)
    return got, want, diag


@pytest.mark.gpu
def test_grey_images_are_the_integer_formula(dev):
    from pointmvsnet_amd import photometric
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (3, 19, 23, 3), dtype=np.uint8)
    images[0, 0, :4] = [[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 0, 255]]
    grey = photometric.grey_images(torch.from_numpy(images).to(dev)).cpu().numpy()
    assert grey.dtype == np.uint8 and np.array_equal(grey, grey_formula(images))
    assert grey[0, 0, 0] == 255 and grey[0, 0, 1] == 0
    assert photometric.grey_images(torch.zeros((2, 0, 5, 3), dtype=torch.uint8).to(dev)).shape == (2, 0, 5)


@pytest.mark.gpu
def test_kernel_equals_the_float32_statement_on_the_scene(dev):
    """V = 5 at 48 x 64, r = 2, all four sources: the shared statement."""
    depths, K, E, images, _ = make_scene()
    st32 = scene_statements()[0]
    got = _run(dev, depths, images, K, E, return_per_source=True, **DEFAULTS)
    _check(got, st32, "scene")
    report("photo_ncc_scene", usable=float((~np.isnan(st32["ncc"])).sum()), kept=float(st32["mask"].sum()))


@pytest.mark.gpu
def test_two_slots_with_a_pad_and_a_row_that_names_itself(dev):
    depths, K, E, images, _ = make_scene()
    sources = np.array([[1, 4], [1, 0], [4, -1], [-1, 2], [4, 4]], np.int32)
    got, want, _ = _case(dev, depths, images, K, E, sources, "pads")
    assert np.isnan(got["ncc"][1, 0]).all() and np.isnan(got["ncc"][2, 1]).all() and np.isnan(got["ncc"][4]).all()
    assert want["usable"][0].max() == 2 and want["usable"][2].max() == 1 and not want["usable"][4].any()


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 5])
def test_partial_tiles(dev, radius):
    """37 x 53: three by four tiles, the last ones ragged; the smallest and the largest window."""
    depths, K, E, images, _ = make_scene(V5, *SMALL)
    got, want, _ = _case(dev, depths, images, K, E, None, "37x53 r%d" % radius, radius=radius)
    assert want["mask"].any() and not want["scorable"][:, :radius].any() and not want["scorable"][:, :, -radius:].any()


@pytest.mark.gpu
def test_no_sources_one_view_and_maps_smaller_than_the_window(dev):
    depths, K, E, images, _ = make_scene()
    got = _run(dev, depths, images, K, E, sources=np.zeros((V5, 0), np.int32), return_per_source=True)
    assert got["ncc"].shape == (V5, 0, H, W)
    got1 = _run(dev, depths[:1], images[:1], K[:1], E[:1], return_per_source=True)
    assert got1["ncc"].shape == (1, 0, H, W)
    for g in (got, got1):
        for k in ("score", "mask", "count", "usable"):
            assert not g[k].any()
    # h < 2 r + 1: nothing is scorable
    thin, _, _ = _case(dev, depths[:, :4], images[:, :4], K, E, None, "h 4")
    assert np.isnan(thin["ncc"]).all() and not thin["usable"].any() and not thin["score"].any()
    empty = _run(dev, depths[:, :0], images[:, :0], K, E, return_per_source=True)
    assert empty["score"].shape == (V5, 0, W) and empty["ncc"].shape == (V5, V5 - 1, 0, W)


@pytest.mark.gpu
def test_constant_image_and_the_variance_threshold_exactly(dev):
    """VR = 0 on a constant image.  View 0 as a checkerboard of grey levels 100 / 109 has, at r = 1, VR = 20 * 81 = the var_min
    of min_variance 20 exactly: scorable, and usable against the textured views 1 and 2.  One of 100 / 108 lies below it:
    nothing of view 0 is scorable, the other views stay as they were."""
    depths, K, E, textured, _ = make_scene(3, blocks=False)
    flat = np.full((3, H, W, 3), 90, np.uint8)
    got, want, _ = _case(dev, depths, flat, K, E, None, "constant")
    assert not want["scorable"].any() and not got["usable"].any() and np.isnan(got["ncc"]).all()
    ys, xs = np.mgrid[0:H, 0:W]
    runs = {}
    for high in (109, 108):
        board = np.where((xs + ys) % 2 == 0, 100, high).astype(np.uint8)
        images = textured.copy()
        images[0] = board[:, :, None]
        runs[high] = _case(dev, depths, images, K, E, None, "checkerboard %d" % high, radius=1, min_variance=20.0)
    (at, want_at, _), (below, want_below, _) = runs[109], runs[108]
    assert want_at["scorable"][0, 1:-1, 1:-1].all() and not want_below["scorable"][0].any()
    assert at["usable"][0].any() and not below["usable"][0].any() and np.isnan(below["ncc"][0]).all()
    assert below["usable"][1:].any()


@pytest.mark.gpu
def test_a_source_turned_away_and_a_window_off_the_border(dev):
    depths, K, E, images, _ = make_scene(3, blocks=False)
    turned = E.copy()
    flip = np.diag([-1.0, 1.0, -1.0])                                  # view 2 looks the other way from where it stands
    centre = -np.linalg.inv(E[2, :, :3]) @ E[2, :, 3]
    turned[2, :, :3] = flip @ E[2, :, :3]
    turned[2, :, 3] = -turned[2, :, :3] @ centre
    sources = np.array([[2, 1], [2, 0], [0, 1]], np.int32)
    got, want, diag = _case(dev, depths, images, K, turned, sources, "turned away")
    assert diag["z_behind"][0, 0].any() and diag["z_behind"][1, 0].any()
    assert np.isnan(got["ncc"][:2, 0]).all() and got["usable"][:2].max() == 1
    # twice the depth moves most windows of views 1 and 2 across view 0's border or off its image
    far = depths * np.float32(2.0)
    got, want, diag = _case(dev, far, images, K, E, None, "off the border")
    lost, live = diag["off_image"], ~np.isnan(want["ncc"])
    assert lost.any() and live.any() and not (lost & live).any()


@pytest.mark.gpu
def test_without_the_per_source_array_reproducible_and_permuted_slots(dev):
    depths, K, E, images, _ = make_scene()
    sources = np.array([[1, 2, 4], [0, 2, 3], [4, 0, 1], [1, 2, 4], [0, 2, 3]], np.int32)
    full = _run(dev, depths, images, K, E, sources=sources, return_per_source=True, **DEFAULTS)
    again = _run(dev, depths, images, K, E, sources=sources, return_per_source=True, **DEFAULTS)
    lean = _run(dev, depths, images, K, E, sources=sources, **DEFAULTS)
    assert "ncc" not in lean
    for k in ("score", "mask", "count", "usable"):
        assert full[k].tobytes() == again[k].tobytes() == lean[k].tobytes()
    assert full["ncc"].tobytes() == again["ncc"].tobytes()
    order = [2, 0, 1]
    moved = _run(dev, depths, images, K, E, sources=sources[:, order], return_per_source=True, **DEFAULTS)
    assert moved["ncc"].tobytes() == full["ncc"][:, order].tobytes()
    assert np.array_equal(moved["count"], full["count"]) and np.array_equal(moved["usable"], full["usable"])
    assert np.array_equal(moved["mask"], full["mask"])


@pytest.mark.gpu
def test_filter_zeroes_off_the_mask_and_reports(dev):
    from pointmvsnet_amd import photometric
    depths, K, E, images, _ = make_scene()
    st32 = scene_statements()[0]
    filtered, rep = photometric.photometric_filter(torch.from_numpy(depths.copy()).to(dev), torch.from_numpy(images.copy()).to(dev),
                                                   K, E, **DEFAULTS)
    assert filtered.cpu().numpy().tobytes() == np.where(st32["mask"], depths, np.float32(0)).tobytes()
    valid = depths > 0
    assert rep["views"]["valid"] == [int(v.sum()) for v in valid] and rep["total"]["valid"] == int(valid.sum())
    assert rep["views"]["scorable"] == [int(v.sum()) for v in st32["scorable"]]
    assert rep["views"]["kept"] == [int(v.sum()) for v in st32["mask"]]
    assert rep["total"]["removed"] == int((valid & ~st32["mask"]).sum()) and rep["settings"]["var_min"] == 15625


def _accumulator(dev, depths, cams, refs, **kw):
    from pointmvsnet_amd import scan
    V, h, w = depths.shape
    acc = scan.ScanAccumulator(V, mode="NEAREST", **kw)
    for v in range(V):
        preds = {"flow2": torch.from_numpy(depths[v].copy())[None, None].to(dev),
                 "flow2_prob": torch.full((1, 5, h, w), 0.2).to(dev), "coarse_prob_map": torch.ones(1, 1, h, w).to(dev)}
        cam = cams[v:v + 1][None].clone()
        cam[0, 0, 1, :2, :3] *= refs.shape[1] / float(h)                           # the cameras of the full image
        batch = {"cam_params_list": cam.to(dev), "cam_params_list_host": cam, "img_list": torch.zeros(1, 1, 3, h, w),
                 "ref_img": torch.from_numpy(refs[v:v + 1, :, :, ::-1].copy())}   # BGR, as the loader hands it
        acc.add(batch, preds, view_index=v)
    return acc


@pytest.mark.gpu
def test_through_the_scan_accumulator(dev):
    from pointmvsnet_amd import fusion, geometric, photometric
    depths, _, _, images, cams = make_scene()
    acc = _accumulator(dev, depths, cams, images)
    K, E = acc.cameras()
    settings = {"radius": 2, "ncc_threshold": 0.6, "num_consistent": 2}
    sources = np.array([[1, 2], [0, 2], [1, 3], [2, 4], [3, 2]], np.int32)
    direct = photometric.photometric_consistency(acc.filtered(), acc.images(), K, E, sources=sources, return_per_source=True,
                                                 **settings)
    through = acc.photometric(sources=sources, return_per_source=True, **settings)
    assert len(through) == 5 and all(torch.equal(a, b) for a, b in zip(through[:4], direct[:4]))
    assert through[4].cpu().numpy().tobytes() == direct[4].cpu().numpy().tobytes()
    maps, rep = photometric.photometric_filter(acc.filtered(), acc.images(), K, E, sources=sources, **settings)
    assert 0 < rep["total"]["kept"] < rep["total"]["valid"]
    photo = dict(settings, sources=sources)
    fuse = {"num_consistent": 2}
    before = fusion.fuse_depth_maps(acc.filtered(), K, E, images=acc.images(), **fuse)
    plain = acc.fuse(**fuse)
    assert acc.last_photo_report is None and all(torch.equal(a, b) for a, b in zip(plain, before))      # photo=None
    pts, col = acc.fuse(photo=photo, **fuse)
    want = fusion.fuse_depth_maps(maps, K, E, images=acc.images(), **fuse)
    assert 0 < pts.shape[0] < plain[0].shape[0] and torch.equal(pts, want[0]) and torch.equal(col, want[1])
    assert acc.last_photo_report == rep
    pts_r, col_r = acc.fuse(photo=photo, method="roundtrip", **fuse)
    want = geometric.geometric_filter(maps, K, E, images=acc.images(), depth_min=1e-3, depth_max=1e5, **fuse)[3:5]
    assert pts_r.shape[0] > 0 and torch.equal(pts_r, want[0]) and torch.equal(col_r, want[1])
    before_r = geometric.geometric_filter(acc.filtered(), K, E, images=acc.images(), depth_min=1e-3, depth_max=1e5, **fuse)[3:5]
    plain_r = acc.fuse(method="roundtrip", **fuse)
    assert acc.last_photo_report is None and all(torch.equal(a, b) for a, b in zip(plain_r, before_r))
    print("points", int(plain[0].shape[0]), "with photo", int(pts.shape[0]), "roundtrip", int(plain_r[0].shape[0]), "with photo",
          int(pts_r.shape[0]))
    with pytest.raises(TypeError):
        acc.fuse(photo="radius=2")
    blind = _accumulator(dev, depths, cams, images, keep_images=False)
    with pytest.raises(ValueError):
        blind.fuse(photo={})
    with pytest.raises(ValueError):
        blind.photometric()
