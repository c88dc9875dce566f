"""Cloud cleaning (pointmvsnet_amd/cloud_filter.py, csrc/cloud_filter.hip) against a float64 statement of its specification.

The specification is the text in pointmvsnet_amd/cloud_filter.py; the yardstick is the ``statement_*`` functions below, written
from that text with NumPy and ``scipy.spatial.cKDTree`` in float64 (no code shared with the product).

The tolerances of the GPU comparisons
-------------------------------------
* mean distances: ``|m_i - statement| <= (k + 8) * 2^-24 * R`` for EVERY point.  Each float32 distance is within
  ``4 * 2^-24`` relative of the float64 one (the bound of tests/test_evaluation.py) and at most R; the mean of the k smallest
  values capped at R is 1-Lipschitz in the sup norm of the distances, so neither ties nor the radius boundary need a band;
  the ascending float32 summation of k terms of at most R costs ``(k - 1) * 2^-24 * R``; the tail term, the last addition
  and the division cost 3.
* counts: ``count_lo <= c_i <= count_hi`` for EVERY point, the neighbours counted in float64 at ``R * (1 -+ 5 * 2^-24)``
  (float32 ``d2`` is within ``5 * 2^-24`` relative) and capped at k.
* statistical mask: equal to the statement's decision outside ``|m_i - thr| <= (2 + std_ratio) * (k + 8) * 2^-24 * R``
  (the error of ``m``, of ``mu`` and of ``std_ratio * sigma``, each 1-Lipschitz in the sup norm); the statement itself puts at
  most 0.05 % of the points into that band (asserted).
* radius mask: equal wherever ``count_lo`` and ``count_hi`` agree about the decision; at most 0.05 % of the points do not.
* voxel merge: inverse map, counts and row order EQUAL to the float32 NumPy statement; positions within
  ``2^-23 * |want| + 2^-40 * max|x|`` per coordinate (the float64 sum is far inside half a float32 ulp: only the final
  rounding can differ); colours equal; normals within ``2^-22`` per component.

The test cloud: ``RandomState(1)``, 20 000 points uniform on a 40 x 40 sheet with ``z = 0.02 x + 0.05 N(0, 1)``, 400 planted
outliers over the sheet at ``|z|`` in [1, 15], the first 200 sheet points once more as exact duplicates: 20 600 float32 points.
"""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, report
from pointmvsnet_amd import cloud_filter as CF

cKDTree = pytest.importorskip("scipy.spatial").cKDTree

EPS32 = 2.0 ** -24
N_SHEET, N_OUT, N_DUP = 20000, 400, 200


# ---------------------------------------------------------------------------------------------------------------------
# the clouds
# ---------------------------------------------------------------------------------------------------------------------
def make_cloud(n_sheet=N_SHEET, n_out=N_OUT, n_dup=N_DUP, side=40.0):
    rs = np.random.RandomState(1)
    xy = rs.uniform(0.0, side, (n_sheet, 2))
    z = 0.02 * xy[:, 0] + 0.05 * rs.normal(0.0, 1.0, n_sheet)
    sheet = np.concatenate([xy, z[:, None]], axis=1)
    oxy = rs.uniform(0.0, side, (n_out, 2))
    oz = rs.uniform(1.0, 15.0, n_out) * np.where(rs.uniform(size=n_out) < 0.5, -1.0, 1.0)
    out = np.concatenate([oxy, oz[:, None]], axis=1)
    return np.concatenate([sheet, out, sheet[:n_dup]]).astype(np.float32)


_CACHE = {}


def cloud():
    if "cloud" not in _CACHE:
        _CACHE["cloud"] = make_cloud()                  # computed once, shared, left unchanged
    return _CACHE["cloud"]


# ---------------------------------------------------------------------------------------------------------------------
# the float64 statement
# ---------------------------------------------------------------------------------------------------------------------
def statement_rows(points, R, k):
    """(n, k) float64: per point the distances to its k nearest OTHER points (by index), ``inf`` where there is none
    within ``R * (1 + 1e-6)``."""
    P = np.asarray(points, np.float64)
    n = len(P)
    if n == 0:
        return np.zeros((0, k))
    d, idx = cKDTree(P).query(P, k=k + 1, distance_upper_bound=R * (1.0 + 1e-6))
    drop = idx == np.arange(n)[:, None]
    absent = ~drop.any(axis=1)                      # more than k duplicates: the query's own index did not make the list
    drop[absent, -1] = True
    assert (drop.sum(axis=1) == 1).all()
    return d[~drop].reshape(n, k)


def statement_mean(points, max_radius, k, rows=None):
    """(m float64, count_lo, count_hi) of the text; R is the float32 value the product uses, as a float64 number."""
    R = float(np.float32(max_radius))
    rows = statement_rows(points, R, k) if rows is None else rows
    m = np.minimum(rows, R).sum(axis=1) / float(k)
    lo = (rows < R * (1.0 - 5 * EPS32)).sum(axis=1)
    hi = (rows < R * (1.0 + 5 * EPS32)).sum(axis=1)
    return m, lo, hi


def mean_tol(R, k):
    return (k + 8) * EPS32 * float(np.float32(R))


def statement_statistical(m, std_ratio):
    """(keep, thr) from float64 ``m``: population standard deviation."""
    thr = m.mean() + std_ratio * m.std()
    return m <= thr, thr


def voxel_cells32(points, voxel):
    P = np.asarray(points, np.float32)
    o = P.min(axis=0)
    inv = np.float32(1.0) / np.float32(voxel)
    q = (P - o) * inv
    assert q.dtype == np.float32
    return np.floor(q).astype(np.int64)


def voxel_cells64(points, voxel):
    P = np.asarray(points, np.float64)
    return np.floor((P - P.min(axis=0)) / float(np.float32(voxel))).astype(np.int64)


def statement_voxel(points, voxel, colors=None, normals=None):
    """The float32 cell assignment and float64 / integer reductions of the text: dict of pos (float64), col, nrm (float64),
    inverse, counts."""
    c = voxel_cells32(points, voxel)
    assert c.min() >= 0 and c.max() < (1 << 17)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    uniq, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    M = len(uniq)
    pos = np.zeros((M, 3))
    np.add.at(pos, inverse, np.asarray(points, np.float64))
    out = {"pos": pos / counts[:, None], "inverse": inverse.astype(np.int64), "counts": counts.astype(np.int32), "col": None,
           "nrm": None}
    if colors is not None:
        s = np.zeros((M, 3), np.int64)
        np.add.at(s, inverse, colors.astype(np.int64))
        out["col"] = ((2 * s + counts[:, None]) // (2 * counts[:, None])).astype(np.uint8)
    if normals is not None:
        s = np.zeros((M, 3))
        np.add.at(s, inverse, np.asarray(normals, np.float64))
        length = np.sqrt((s * s).sum(axis=1))
        out["nrm"] = np.where(length[:, None] > 0, s / np.where(length > 0, length, 1.0)[:, None], 0.0)
        out["nrm_zero"] = length == 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_statement_closed_forms():
    p = 0.25
    line = np.stack([np.arange(41) * p, np.zeros(41), np.zeros(41)], axis=1)            # exact in binary
    m, lo, hi = statement_mean(line, 10.0, 4)
    assert m[20] == (p + p + 2 * p + 2 * p) / 4.0 and m[0] == (p + 2 * p + 3 * p + 4 * p) / 4.0 and (lo == 4).all()
    m, lo, hi = statement_mean(line, 0.3, 4)                                            # only the two at distance p
    assert m[20] == (2 * p + 2 * float(np.float32(0.3))) / 4.0 and lo[20] == hi[20] == 2 and lo[0] == 1
    same = np.full((50, 3), 1.25)
    for k in (8, 32):
        m, lo, hi = statement_mean(same, 2.0, k)
        assert (m == 0).all() and (lo == k).all() and (hi == k).all()
    same = np.full((5, 3), 1.25)
    m, lo, hi = statement_mean(same, 2.0, 16)
    assert np.allclose(m, 12 * 2.0 / 16, rtol=0, atol=1e-15) and (lo == 4).all()
    m, lo, hi = statement_mean(np.array([[1.0, 2.0, 3.0]]), 0.7, 8)
    assert m[0] == float(np.float32(0.7)) and lo[0] == hi[0] == 0
    keep, thr = statement_statistical(np.array([1.0, 1.0, 1.0, 5.0]), 1.0)
    assert keep.tolist() == [True, True, True, False] and abs(thr - (2.0 + np.sqrt(3.0))) < 1e-12


def test_the_test_cloud_meets_the_statements_conditions():
    P = cloud()
    assert P.shape == (N_SHEET + N_OUT + N_DUP, 3) and P.dtype == np.float32
    assert np.array_equal(P[N_SHEET + N_OUT:], P[:N_DUP])
    for voxel in (0.2, 5.0):
        a, b = voxel_cells32(P, voxel), voxel_cells64(P, voxel)
        differ = int((a != b).any(axis=1).sum())
        st = statement_voxel(P, voxel)
        print("voxel", voxel, "cells that differ between float32 and float64", differ, "voxels", len(st["counts"]),
              "largest", int(st["counts"].max()))
        assert differ == 0
    st = statement_voxel(P, 0.2)
    assert 15000 < len(st["counts"]) < 20000 and st["counts"].max() <= 8 and st["counts"].sum() == len(P)
    assert statement_voxel(P, 5.0)["counts"].max() > 200                                # long segments
    for R, k in ((2.0, 8), (2.0, 16), (0.6, 32)):
        m, lo, hi = statement_mean(P, R, k)
        short = int((hi < k).sum())
        print("R", R, "k", k, "points with fewer than k neighbours", short, "count band", int((lo != hi).sum()))
        if R == 0.6:
            assert short == len(P)                                                      # the tail term everywhere
        else:
            assert 300 < short < 420


def test_abi_agrees_with_the_new_symbols(lib_built):
    import json
    from pointmvsnet_amd import _lib, build
    names = {"pf_cloud_knn_stats_f32", "pf_cloud_radius_count_f32", "pf_cloud_voxel_keys_f32", "pf_cloud_voxel_reduce_f32"}
    text = open(os.path.join(ROOT, "include", "pointflow_hip.h")).read()
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert names <= declared and names <= set(_lib.PROTOTYPES) and set(_lib.PROTOTYPES) == declared
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name)
    assert "cloud_filter.hip" in build.SOURCES and "cloud_eval.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "pointmvsnet_amd", "csrc", "pf_cloud_grid.h"))
    usage = json.load(open(build.USAGE_FILE))["cloud_filter.hip"]
    kernels = [k for k in usage if "cloud_" in k]
    assert len(kernels) == 6                                                            # knn<8,16,32>, count, keys, reduce
    for k in kernels:
        assert usage[k]["scratch_bytes_per_lane"] == 0, k
    assert CF.MAX_K == 32 and "#define PF_CLOUD_MAX_K 32" in text


def test_cloud_filter_has_no_cpu_path():
    pts = torch.from_numpy(cloud()[:100].copy())
    col = torch.zeros((100, 3), dtype=torch.uint8)
    for call in (lambda: CF.knn_mean_distances(pts, 1.0), lambda: CF.statistical_outlier_mask(pts, 1.0),
                 lambda: CF.radius_outlier_mask(pts, 1.0, 3), lambda: CF.voxel_downsample(pts, 0.5, colors=col),
                 lambda: CF.clean_cloud(pts, voxel=0.5), lambda: CF.clean_cloud(pts, max_radius=1.0)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_argument_errors():
    pts = torch.from_numpy(cloud()[:100].copy())
    bad = [lambda: CF.knn_mean_distances(pts, 1.0, k=0), lambda: CF.knn_mean_distances(pts, 1.0, k=33),
           lambda: CF.knn_mean_distances(pts, 0.0), lambda: CF.knn_mean_distances(pts, -1.0),
           lambda: CF.knn_mean_distances(pts, float("nan")), lambda: CF.knn_mean_distances(pts, 1.0, k=2.5),
           lambda: CF.statistical_outlier_mask(pts, 1.0, k=33), lambda: CF.statistical_outlier_mask(pts, -2.0),
           lambda: CF.radius_outlier_mask(pts, 1.0, 33), lambda: CF.radius_outlier_mask(pts, 1.0, 0),
           lambda: CF.radius_outlier_mask(pts, 0.0, 3),
           lambda: CF.voxel_downsample(pts, 0.0), lambda: CF.voxel_downsample(pts, -0.2),
           lambda: CF.voxel_downsample(pts, 0.5, colors=torch.zeros((99, 3), dtype=torch.uint8)),
           lambda: CF.voxel_downsample(pts, 0.5, normals=torch.zeros((101, 3))),
           lambda: CF.voxel_downsample(pts, 0.5, colors=torch.zeros((100, 3))),            # not uint8
           lambda: CF.voxel_downsample(pts, 1e-4),                                         # 40 / 1e-4 > 2^17 cells
           lambda: CF.clean_cloud(pts, min_neighbors=3),                                   # no radius
           lambda: CF.clean_cloud(pts, voxel=-1.0), lambda: CF.clean_cloud(pts, voxel=0.0),
           lambda: CF.clean_cloud(pts, max_radius=0.0),                                    # zero is an error, not "off"
           lambda: CF.knn_mean_distances(pts[:, :2], 1.0), lambda: CF.knn_mean_distances(pts.double(), 1.0),
           lambda: CF.knn_mean_distances(torch.tensor([[0.0, float("inf"), 0.0]]), 1.0)]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d raised nothing" % i)
    assert float(pts[:, :2].max() - pts[:, :2].min()) / 1e-4 > (1 << 17)


# ---------------------------------------------------------------------------------------------------------------------
# 2. on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _knn(dev, P, R, k):
    m, c = CF.knn_mean_distances(torch.from_numpy(np.ascontiguousarray(P)).to(dev), R, k, return_count=True)
    assert m.dtype == torch.float32 and c.dtype == torch.int32 and m.shape == c.shape == (len(P),)
    return m.cpu().numpy(), c.cpu().numpy()


def _check_knn(dev, name, P, R, k):
    want, lo, hi = statement_mean(P, R, k)
    m, c = _knn(dev, P, R, k)
    err = float(np.abs(m.astype(np.float64) - want).max()) if len(P) else 0.0
    tol = mean_tol(R, k)
    outside = int(((c < lo) | (c > hi)).sum())
    print(name, "points", len(P), "R", R, "k", k, "max |m - statement|", err, "tol", tol, "counts outside", outside,
          "count band", int((lo != hi).sum()))
    report("cloud_filter_knn_" + name, points=len(P), R=R, k=k, err_max=err, tol=tol, counts_outside=outside)
    assert err <= tol
    assert outside == 0
    return m, c


@pytest.mark.gpu
def test_the_grid_pitch_does_not_show(dev):
    """1 (the plain form: 27 cells hold the radius), 2 (the default), 3 and 4 cells to the radius give the same bytes, at
    (2.0, 8), where the sheet is final after a ring or two and the planted outliers walk every ring, and at (0.6, 32), where
    no point has 32 neighbours and every point does."""
    P = torch.from_numpy(cloud()).to(dev)
    for R, k in ((2.0, 8), (0.6, 32)):
        m, c = CF.knn_mean_distances(P, R, k, return_count=True)
        for cells in (1, 2, 3, 4):
            grid = CF._search_grid(P, np.float32(R), cells=cells)
            m1, c1 = torch.full_like(m, -1.0), torch.full_like(c, -1)
            CF._knn_stats(grid, np.float32(R), k, m1, c1)
            assert torch.equal(m1, m) and torch.equal(c1, c), (R, k, cells)


@pytest.mark.gpu
@pytest.mark.parametrize("R,k", [(2.0, 8), (2.0, 16), (0.6, 32)])
def test_mean_distances_match_the_statement(dev, R, k):
    _check_knn(dev, "cloud", cloud(), R, k)


@pytest.mark.gpu
def test_mean_distances_are_a_pure_function_of_the_input(dev):
    P = cloud()
    R, k = 2.0, 16
    m, c = _knn(dev, P, R, k)
    m2, c2 = _knn(dev, P, R, k)
    assert m.tobytes() == m2.tobytes() and c.tobytes() == c2.tobytes()                  # two runs
    perm = np.random.RandomState(2).permutation(len(P))
    mp, cp = _knn(dev, P[perm], R, k)
    assert mp.tobytes() == m[perm].tobytes() and cp.tobytes() == c[perm].tobytes()      # a permuted cloud
    far = np.array([[3.0e6, 20.0, 0.0], [-3.0e6, 20.0, 0.0]], np.float32)               # the grid's cells are widened
    assert 6.0e6 / ((1 << 17) - 4) > 10 * R
    mw, cw = _knn(dev, np.concatenate([P, far]), R, k)
    assert mw[:len(P)].tobytes() == m.tobytes() and cw[:len(P)].tobytes() == c.tobytes()
    assert (mw[len(P):] == np.float32(R)).all() and (cw[len(P):] == 0).all()
    single = CF.knn_mean_distances(torch.from_numpy(P).to(dev), R, k)                   # without the counts
    assert single.cpu().numpy().tobytes() == m.tobytes()


@pytest.mark.gpu
def test_small_and_awkward_shapes(dev):
    P = cloud()
    for n in (0, 1, 2, 63, 64, 65, 257):
        m, c = _check_knn(dev, "n%d" % n, P[:n], 2.0, 8)
        if n == 1:
            assert m[0] == np.float32(2.0) and c[0] == 0
    m, c = _knn(dev, P[:1], 0.7, 5)
    assert m[0] == np.float32(0.7) and c[0] == 0
    same = np.tile(P[7:8], (100, 1))
    for k in (8, 32):
        m, c = _check_knn(dev, "identical_k%d" % k, same, 2.0, k)
        assert (m == 0).all() and (c == k).all()
    m, c = _check_knn(dev, "five", P[:5] * np.float32(0.01), 2.0, 16)
    assert (c == 4).all()
    rs = np.random.RandomState(3)
    one_cell = (np.array([5.0, 6.0, 7.0]) + rs.uniform(0.0, 0.5, (300, 3))).astype(np.float32)   # extent < one cell
    m, c = _check_knn(dev, "one_cell", one_cell, 2.0, 16)
    assert (c == 16).all()
    _check_knn(dev, "small_cloud", make_cloud(3000, 60, 200), 2.0, 16)
    with pytest.raises(ValueError):
        CF.knn_mean_distances(torch.tensor([[0.0, float("nan"), 0.0]], device=dev), 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("R,k,std_ratio", [(2.0, 8, 2.0), (0.6, 32, 1.0)])
def test_statistical_mask_matches_the_statement(dev, R, k, std_ratio):
    P = cloud()
    want_m, _, _ = statement_mean(P, R, k)
    want, thr = statement_statistical(want_m, std_ratio)
    band = np.abs(want_m - thr) <= (2.0 + std_ratio) * mean_tol(R, k)
    assert band.sum() <= 0.0005 * len(P)                                                # the statement's own condition
    keep, m = CF.statistical_outlier_mask(torch.from_numpy(P).to(dev), R, k, std_ratio, return_distances=True)
    assert keep.dtype == torch.bool and keep.shape == (len(P),)
    keep = keep.cpu().numpy()
    planted = np.zeros(len(P), bool)
    planted[N_SHEET:N_SHEET + N_OUT] = True
    differ = int((keep != want)[~band].sum())
    print("R", R, "k", k, "std_ratio", std_ratio, "thr", thr, "in the band", int(band.sum()), "statement removes",
          int((~want).sum()), "of them planted", int((~want & planted).sum()), "product removes", int((~keep).sum()),
          "decisions that differ outside the band", differ)
    report("cloud_filter_statistical_k%d" % k, band=int(band.sum()), removed=int((~keep).sum()),
           removed_statement=int((~want).sum()), differ=differ)
    assert differ == 0
    assert np.abs(m.cpu().numpy().astype(np.float64) - want_m).max() <= mean_tol(R, k)
    plain = CF.statistical_outlier_mask(torch.from_numpy(P).to(dev), R, k, std_ratio)
    assert np.array_equal(plain.cpu().numpy(), keep)
    if k == 8:
        assert (~want & planted).sum() >= 0.95 * N_OUT and (~want & ~planted).sum() <= 5
        assert not keep[~want & planted & ~band].any()                                  # the planted outliers are removed
    assert CF.statistical_outlier_mask(torch.from_numpy(P[:0]).to(dev), R, k).shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("min_neighbors", [1, 8, 32])
def test_radius_mask_matches_the_statement(dev, min_neighbors):
    P = cloud()
    R = 2.0
    _, lo, hi = statement_mean(P, R, min_neighbors)
    sure = (lo >= min_neighbors) == (hi >= min_neighbors)
    assert (~sure).sum() <= 0.0005 * len(P)
    keep = CF.radius_outlier_mask(torch.from_numpy(P).to(dev), R, min_neighbors)
    assert keep.dtype == torch.bool and keep.shape == (len(P),)
    keep = keep.cpu().numpy()
    differ = int((keep != (lo >= min_neighbors))[sure].sum())
    print("min_neighbors", min_neighbors, "kept", int(keep.sum()), "undecided by the statement", int((~sure).sum()),
          "decisions that differ", differ)
    report("cloud_filter_radius_%d" % min_neighbors, kept=int(keep.sum()), undecided=int((~sure).sum()), differ=differ)
    assert differ == 0 and 0 < (~keep).sum() < len(P)
    again = CF.radius_outlier_mask(torch.from_numpy(P).to(dev), R, min_neighbors).cpu().numpy()
    assert np.array_equal(again, keep)
    assert CF.radius_outlier_mask(torch.from_numpy(P[:0]).to(dev), R, min_neighbors).shape == (0,)


def _voxel_inputs():
    """The cloud plus two points that share a voxel beyond its far corner and carry opposite normals."""
    rs = np.random.RandomState(5)
    P = np.concatenate([cloud(), np.array([[45.05, 45.05, 15.55], [45.07, 45.02, 15.57]], np.float32)])
    col = rs.randint(0, 256, (len(P), 3)).astype(np.uint8)
    nrm = rs.normal(size=(len(P), 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[-1] = -nrm[-2]
    return P, col, nrm


def _voxel(dev, P, voxel, col=None, nrm=None):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pos, c, n, inverse, counts = CF.voxel_downsample(t(P), voxel, colors=t(col), normals=t(nrm), return_inverse=True,
                                                     return_counts=True)
    assert pos.dtype == torch.float32 and inverse.dtype == torch.int64 and counts.dtype == torch.int32
    assert (c is None) == (col is None) and (n is None) == (nrm is None)
    f = lambda a: None if a is None else a.cpu().numpy()
    return f(pos), f(c), f(n), f(inverse), f(counts)


def _pos_tol(want, P):
    return 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * float(np.abs(P).max())


@pytest.mark.gpu
@pytest.mark.parametrize("voxel", [0.2, 5.0])
def test_voxel_merge_matches_the_statement(dev, voxel):
    P, col, nrm = _voxel_inputs()
    st = statement_voxel(P, voxel, col, nrm)
    pair = st["inverse"][-1]
    assert st["inverse"][-2] == pair and st["counts"][pair] == 2 and st["nrm_zero"][pair] and st["nrm_zero"].sum() == 1
    pos, c, n, inverse, counts = _voxel(dev, P, voxel, col, nrm)
    assert pos.shape == (len(st["counts"]), 3) and c.dtype == np.uint8 and n.dtype == np.float32
    assert np.array_equal(inverse, st["inverse"]) and np.array_equal(counts, st["counts"])          # and so the row order
    pos_err = np.abs(pos.astype(np.float64) - st["pos"])
    nrm_err = float(np.abs(n.astype(np.float64) - st["nrm"]).max())
    print("voxel", voxel, "rows", len(counts), "largest", int(counts.max()), "position error / tolerance",
          float((pos_err / _pos_tol(st["pos"], P)).max()), "colour mismatches", int((c != st["col"]).sum()), "normal error",
          nrm_err)
    report("cloud_filter_voxel_%g" % voxel, rows=len(counts), pos_err_over_tol=float((pos_err / _pos_tol(st["pos"], P)).max()),
           colour_mismatches=int((c != st["col"]).sum()), normal_err=nrm_err)
    assert (pos_err <= _pos_tol(st["pos"], P)).all()
    assert np.array_equal(c, st["col"])
    assert nrm_err <= 2.0 ** -22 and (n[pair] == 0).all()
    # two runs: identical bytes
    again = _voxel(dev, P, voxel, col, nrm)
    for a, b in zip(again, (pos, c, n, inverse, counts)):
        assert a.tobytes() == b.tobytes()
    # without colours and normals: the same positions, bit for bit
    bare = _voxel(dev, P, voxel)
    assert bare[0].tobytes() == pos.tobytes() and bare[1] is None and bare[2] is None and np.array_equal(bare[3], inverse)
    only = CF.voxel_downsample(torch.from_numpy(P).to(dev), voxel)
    assert len(only) == 3 and only[0].cpu().numpy().tobytes() == pos.tobytes() and only[1] is None and only[2] is None
    # a permuted input gives the same rows (the float64 sums change order: positions to the same tolerance)
    perm = np.random.RandomState(6).permutation(len(P))
    pp, pc, pn, pinv, pcounts = _voxel(dev, P[perm], voxel, col[perm], nrm[perm])
    assert np.array_equal(pinv, inverse[perm]) and np.array_equal(pcounts, counts) and np.array_equal(pc, c)
    assert (np.abs(pp.astype(np.float64) - st["pos"]) <= _pos_tol(st["pos"], P)).all()
    keep = ~st["nrm_zero"]
    assert np.abs(pn.astype(np.float64) - st["nrm"])[keep].max() <= 2.0 ** -22
    if voxel == 0.2:
        empty = CF.voxel_downsample(torch.from_numpy(P[:0]).to(dev), voxel, return_inverse=True, return_counts=True)
        assert empty[0].shape == (0, 3) and empty[3].shape == (0,) and empty[4].shape == (0,)
        one = _voxel(dev, P[:1], voxel, col[:1], nrm[:1])
        assert one[0].tobytes() == P[:1].tobytes() and np.array_equal(one[1], col[:1]) and one[4].tolist() == [1]


def make_plane_scan(V=5, h=96, w=128, sigma=0.3, seed=0):
    """V cameras 60 apart on a line, looking at a tilted plane 600 away; depth maps by ray-plane intersection plus Gaussian
    noise of ``sigma`` (the scan of tests/test_evaluation.py).  Returns depths, K, E (V, 4, 4)."""
    rng = np.random.default_rng(seed)
    target = np.array([0.0, 0.0, 600.0])
    n = np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    f = 2.2 * w
    K = np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
    depths, Es = [], []
    for v in range(V):
        centre = np.array([(v - (V - 1) / 2.0) * 60.0, 0.0, 0.0])
        fwd = (target - centre) / np.linalg.norm(target - centre)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        Rm = np.stack([right, np.cross(fwd, right), fwd])
        d = (n @ target - n @ centre) / (rays @ (Rm @ n))
        depths.append((d + rng.normal(0.0, sigma, d.shape)).astype(np.float32))
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = Rm, -Rm @ centre
        Es.append(E)
    return np.stack(depths), np.stack([K] * V), np.stack(Es)


@pytest.mark.gpu
def test_end_to_end_through_the_scan_accumulator(dev, tmp_path):
    from pointmvsnet_amd import geometric, scan
    from pointmvsnet_amd.utils import io as IO
    depths, K, E = make_plane_scan()
    V, h, w = depths.shape
    images = np.random.RandomState(7).randint(0, 256, (V, h, w, 3)).astype(np.uint8)
    acc = scan.ScanAccumulator(V, mode="NEAREST")
    for v in range(V):
        preds = {"flow2": torch.from_numpy(depths[v])[None, None].to(dev), "flow2_prob": torch.full((1, 5, h, w), 0.2).to(dev),
                 "coarse_prob_map": torch.ones(1, 1, h, w).to(dev)}
        cam = np.zeros((1, 1, 2, 4, 4))
        cam[0, 0, 0], cam[0, 0, 1, :3, :3] = E[v], K[v]
        cam = torch.from_numpy(cam)
        batch = {"cam_params_list": cam.to(dev), "cam_params_list_host": cam, "img_list": torch.zeros(1, 1, 3, h, w),
                 "ref_img": torch.from_numpy(images[v:v + 1, :, :, ::-1].copy())}
        acc.add(batch, preds, view_index=v)
    fuse = dict(method="roundtrip", with_normals=True, pix_threshold=2.0, rel_depth_threshold=0.01)
    Ka, Ea = acc.cameras()
    parent = geometric.geometric_filter(acc.filtered(), Ka, Ea, images=acc.images(), with_normals=True, pix_threshold=2.0,
                                        rel_depth_threshold=0.01)[3:6]
    raw = acc.fuse(clean=None, **fuse)
    default = acc.fuse(**fuse)
    assert len(raw) == 3 and raw[0].shape[0] > 2000 and raw[1] is not None
    for a, b, c in zip(raw, default, parent):                                           # clean=None: the parent's bytes
        assert torch.equal(a, b) and a.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()
    clean = dict(voxel=1.0, max_radius=3.0, k=8, std_ratio=2.0, min_neighbors=2)
    got = acc.fuse(clean=clean, **fuse)
    want = CF.clean_cloud(raw[0], raw[1], raw[2], **clean)
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want[:3]))
    rep = want[3]
    assert acc.last_clean_report == rep and rep["input"] == raw[0].shape[0] and rep["output"] == got[0].shape[0]
    assert rep["input"] > rep["voxel"] >= rep["radius"] >= rep["statistical"] == rep["output"] > 100
    print("end to end", rep)
    report("cloud_filter_end_to_end", **rep)
    assert got[1].dtype == torch.uint8 and got[2].dtype == torch.float32 and got[1].shape == got[2].shape == got[0].shape
    # after voxel= no two output points share a voxel, and the count drops
    merged = acc.fuse(clean=dict(voxel=1.0, std_ratio=None), **fuse)
    assert acc.last_clean_report == {"input": rep["input"], "voxel": rep["voxel"], "output": rep["voxel"]}
    mp = merged[0].cpu().numpy()
    cells = voxel_cells32(raw[0].cpu().numpy(), 1.0)
    o = raw[0].cpu().numpy().min(axis=0)
    own = np.floor((mp - o) * (np.float32(1.0) / np.float32(1.0))).astype(np.int64)     # a mean stays inside its voxel, up to
    assert len(np.unique(cells, axis=0)) == len(mp) < len(cells)                        # rounding on a face: compare loosely
    assert len(np.unique(own, axis=0)) >= len(mp) - 2
    assert cKDTree(mp.astype(np.float64)).query(mp.astype(np.float64), k=2)[0][:, 1].min() > 0
    # the disparity fuser and write_ply pass the option through as well
    path = str(tmp_path / "clean.ply")
    two = acc.write_ply(path, clean=dict(voxel=1.0, std_ratio=None), num_consistent=2)
    assert acc.last_clean_report["output"] == two[0].shape[0]
    plain = acc.fuse(num_consistent=2)
    assert acc.last_clean_report is None                                                # it describes the last call
    assert len(two) == 2 and two[0].shape[0] < plain[0].shape[0]
    assert IO.load_ply_points(path).tobytes() == two[0].cpu().numpy().tobytes()
    with pytest.raises(TypeError):
        acc.fuse(clean=[("voxel", 1.0)], **fuse)
