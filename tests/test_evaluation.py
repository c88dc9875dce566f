"""Point-cloud evaluation (pointmvsnet_amd/evaluation.py, csrc/cloud_eval.hip) against a float64 statement of its specification.

DTU's evaluation is a MATLAB program that exists neither here nor for ROCm: the specification is the text in
pointmvsnet_amd/evaluation.py and the yardstick is the ``statement_*`` functions below, written from that text (the greedy
walk in key order in plain Python, the distances by ``scipy.spatial.cKDTree`` in float64; no code shared with the product).

The tolerances of the GPU comparisons
-------------------------------------
* thinning: EQUAL index sets.  ``near`` compares a float32 sum of three squares (within 5 * 2^-24 relative of the true
  d^2) against t, so the kernel and the statement can only disagree on a pair whose distance is that close to min_dist.
  The inputs are built, with the float64 statement alone, to contain NO pair within relative 1e-5 of min_dist (one point of
  each such pair is dropped first); the test asserts that.  Exact duplicates stay in.
* distances: |d_gpu - d_f64| <= 4 * 2^-24 * d_f64 (three differences, three squares, two sums and a root, each 2^-24
  relative: 5 on d^2, 2.5 + 1 on d, rounded up) for queries inside the cap; the inputs hold no query whose float64 distance
  is within relative 1e-5 of max_dist (asserted), beyond it the result is exactly max_dist and the index -1.
* filters: EQUAL for points no closer than 1e-4 * res to a voxel boundary / 1e-4 relative to the plane (asserted).
* scores: counts equal; means and medians within the distance bound relative to the value.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, report
from pointmvsnet_amd import evaluation as EV
from pointmvsnet_amd.utils import io as IO

cKDTree = pytest.importorskip("scipy.spatial").cKDTree

EPS32 = 2.0 ** -24
DIST_TOL = 4 * EPS32
BAND = 1e-5
MIN_DIST, MAX_DIST = 0.2, 20.0


# ---------------------------------------------------------------------------------------------------------------------
# the float64 statement
# ---------------------------------------------------------------------------------------------------------------------
def prio(i):
    x = i & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def keys_of(n):
    return np.array([(prio(i) << 32) | i for i in range(n)], dtype=np.uint64)


def near_pairs(points, min_dist, slack=0.0):
    """(i, j, d) of every pair with d < min_dist * (1 + slack), d in float64."""
    P = np.asarray(points, np.float64)
    if len(P) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    pairs = cKDTree(P).query_pairs(min_dist * (1.0 + slack) * (1.0 + 1e-9), output_type="ndarray")
    d = np.sqrt(((P[pairs[:, 0]] - P[pairs[:, 1]]) ** 2).sum(axis=1))
    ok = d < min_dist * (1.0 + slack)
    return pairs[ok, 0], pairs[ok, 1], d[ok]


def _lower_neighbours(n, i, j, key):
    """CSR lists: for every point its near neighbours of LOWER key."""
    hi = np.where(key[i] > key[j], i, j)
    lo = np.where(key[i] > key[j], j, i)
    order = np.argsort(hi, kind="stable")
    start = np.searchsorted(hi[order], np.arange(n + 1))
    return start, lo[order]


def statement_thin(points, min_dist=MIN_DIST, key=None):
    """The sequential greedy walk in key order; returns the sorted indices of the kept points."""
    n = len(points)
    t = float(np.float32(min_dist))
    i, j, _ = near_pairs(points, t)
    key = keys_of(n) if key is None else key
    start, lo = _lower_neighbours(n, i, j, key)
    kept = np.zeros(n, bool)
    for p in np.argsort(key):
        kept[p] = not kept[lo[start[p]:start[p + 1]]].any()
    return np.nonzero(kept)[0]


def statement_thin_rounds(points, min_dist=MIN_DIST, key=None):
    """The round-parallel form: (sorted kept indices, rounds)."""
    n = len(points)
    i, j, _ = near_pairs(points, float(np.float32(min_dist)))
    key = keys_of(n) if key is None else key
    hi = np.where(key[i] > key[j], i, j)
    lo = np.where(key[i] > key[j], j, i)
    state = np.zeros(n, np.int8)                    # 0 undecided, 1 kept, 2 removed
    rounds = 0
    while (state == 0).any():
        has_kept = np.zeros(n, bool)
        has_undecided = np.zeros(n, bool)
        has_kept[hi[state[lo] == 1]] = True
        has_undecided[hi[state[lo] == 0]] = True
        new = np.where(has_kept, 2, np.where(has_undecided, 0, 1)).astype(np.int8)
        state = np.where(state == 0, new, state)
        rounds += 1
    return np.nonzero(state == 1)[0], rounds


def drop_band_pairs(points, min_dist=MIN_DIST):
    """Drop one point of every pair whose distance is within relative BAND of min_dist; assert none is left."""
    t = float(np.float32(min_dist))
    i, j, d = near_pairs(points, t, slack=10 * BAND)
    bad = np.abs(d / t - 1.0) <= BAND
    keep = np.ones(len(points), bool)
    keep[np.maximum(i[bad], j[bad])] = False
    out = np.ascontiguousarray(points[keep])
    _, _, d = near_pairs(out, t, slack=10 * BAND)
    assert not (np.abs(d / t - 1.0) <= BAND).any()
    return out, int(bad.sum())


def statement_distances(query, target, max_dist=MAX_DIST):
    """(uncapped float64 nearest distance (inf for an empty target), index)."""
    if len(target) == 0 or len(query) == 0:
        return np.full(len(query), np.inf), np.full(len(query), -1, np.int64)
    d, idx = cKDTree(np.asarray(target, np.float64)).query(np.asarray(query, np.float64))
    return d, idx


def statement_obs_mask(points, mask, bb_min, res):
    u = (np.asarray(points, np.float64) - np.asarray(bb_min, np.float64)) / float(res) + 0.5
    idx = np.floor(u).astype(np.int64)
    inside = ((idx >= 0) & (idx < np.array(mask.shape))).all(axis=1)
    out = np.zeros(len(points), bool)
    out[inside] = mask[idx[inside, 0], idx[inside, 1], idx[inside, 2]]
    return out, np.abs(u - np.rint(u)).min(axis=1) if len(points) else np.zeros(0)


def statement_plane(points, plane):
    P = np.asarray(points, np.float64)
    terms = np.concatenate([P * np.asarray(plane[:3], np.float64), np.full((len(P), 1), float(plane[3]))], axis=1)
    s = terms.sum(axis=1)
    return s > 0, np.abs(s) / np.abs(terms).sum(axis=1)


def lower_median(d):
    return float(np.sort(d)[(len(d) - 1) // 2]) if len(d) else float("nan")


def statement_scores(data, gt, min_dist=MIN_DIST, max_dist=MAX_DIST, obs_mask=None, bb_min=None, res=None, plane=None,
                     thin=True, kept=None):
    """The dict of evaluate_point_cloud in float64 (``kept``: use this thinned index set instead of computing it)."""
    data = np.asarray(data, np.float64)
    gt = np.asarray(gt, np.float64)
    if thin and kept is None:
        kept = statement_thin(data, min_dist)
    thinned = data[kept] if thin else data
    d_acc, _ = statement_distances(thinned, gt)
    d_comp, _ = statement_distances(gt, thinned)
    acc_used = d_acc < max_dist
    if obs_mask is not None:
        acc_used &= statement_obs_mask(thinned, obs_mask, bb_min, res)[0]
    comp_used = d_comp < max_dist
    if plane is not None:
        comp_used &= statement_plane(gt, plane)[0]
    a, c = d_acc[acc_used], d_comp[comp_used]
    am = float(a.mean()) if len(a) else float("nan")
    cm = float(c.mean()) if len(c) else float("nan")
    return {"accuracy_mean": am, "accuracy_median": lower_median(a), "completeness_mean": cm,
            "completeness_median": lower_median(c), "overall": (am + cm) / 2.0, "n_data": len(data),
            "n_data_thinned": len(thinned), "n_data_used": int(acc_used.sum()), "n_gt": len(gt),
            "n_gt_used": int(comp_used.sum())}, d_acc, d_comp


# ---------------------------------------------------------------------------------------------------------------------
# the clouds
# ---------------------------------------------------------------------------------------------------------------------
def noisy_sheet(n, side, seed, noise=0.05, offset=0.0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, side, (n, 2))
    z = 0.02 * xy[:, 0] + rng.normal(0.0, noise, n)
    return (np.concatenate([xy, z[:, None]], axis=1) + offset).astype(np.float32)


def grid_cloud(rows=300, cols=400, pitch=0.11):
    ys, xs = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    z = 0.05 * np.sin(xs * 0.05) + 0.03 * np.cos(ys * 0.07)
    return np.stack([xs * pitch, ys * pitch, z], -1).reshape(-1, 3).astype(np.float32)       # row-major


def sampled_plane(nx, ny, pitch, z):
    ys, xs = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([xs * pitch, ys * pitch, np.full(xs.shape, z)], -1).reshape(-1, 3).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_prio_against_values_computed_by_hand():
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on 32 bits, step by step in Python ints."""
    def by_hand(i):
        M = 1 << 32
        a = i ^ (i >> 16)
        b = (a * 2146121005) % M
        c = b ^ (b >> 15)
        d = (c * 2221713035) % M
        return d ^ (d >> 16)

    cases = [0, 1, 2, 3, 255, 65536, 123456, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    assert len(cases) == 10 and prio(0) == 0
    for i in cases:
        assert prio(i) == by_hand(i) and 0 <= prio(i) < 2 ** 32
    assert 0x7feb352d == 2146121005 and 0x846ca68b == 2221713035
    assert len({prio(i) for i in range(100000)}) == 100000                 # injective where it can be checked
    k = keys_of(5)
    assert [int(v) >> 32 for v in k] == [prio(i) for i in range(5)] and [int(v) & 0xffffffff for v in k] == list(range(5))


def test_statement_thinning_is_independent_maximal_and_equals_its_parallel_form():
    for name, cloud in (("sheet", noisy_sheet(20000, 30.0, 1)), ("grid", grid_cloud(60, 80))):
        cloud = np.concatenate([cloud, cloud[:50]])                          # exact duplicates
        kept = statement_thin(cloud)
        n = len(cloud)
        key = keys_of(n)
        i, j, _ = near_pairs(cloud, float(np.float32(MIN_DIST)))
        is_kept = np.zeros(n, bool)
        is_kept[kept] = True
        assert not (is_kept[i] & is_kept[j]).any()                           # independent
        covered = np.zeros(n, bool)                                          # maximal: a kept near neighbour of LOWER key
        a = is_kept[i] & (key[i] < key[j])
        covered[j[a]] = True
        b = is_kept[j] & (key[j] < key[i])
        covered[i[b]] = True
        assert (covered | is_kept).all() and not (covered & is_kept).any()
        assert not is_kept[n - 50:].all() and 0 < len(kept) < n
        par, rounds = statement_thin_rounds(cloud)
        print(name, "points", n, "kept", len(kept), "rounds", rounds)
        assert np.array_equal(par, kept) and rounds < 40
    # the hashed keys are what keeps the rounds few: plain index order on the same grid needs many more
    g = grid_cloud(60, 80)
    _, hashed = statement_thin_rounds(g)
    plain, slow = statement_thin_rounds(g, key=np.arange(len(g), dtype=np.uint64))
    assert slow > 4 * hashed and np.array_equal(plain, statement_thin(g, key=np.arange(len(g), dtype=np.uint64)))


def test_statement_scores_closed_forms():
    delta = 0.75
    a = sampled_plane(120, 90, 0.25, 0.0)
    b = sampled_plane(120, 90, 0.25, delta)                                  # the same lattice, delta above
    s, _, _ = statement_scores(a, b)
    assert s["n_data_thinned"] == s["n_data"] == len(a)                      # pitch 0.25 > min_dist: nothing thinned
    for k in ("accuracy_mean", "accuracy_median", "completeness_mean", "completeness_median", "overall"):
        assert abs(s[k] - delta) < 1e-12, k
    s, _, _ = statement_scores(a, a)
    assert s["accuracy_mean"] == 0.0 and s["completeness_mean"] == 0.0 and s["overall"] == 0.0
    mask = np.zeros((4, 4, 4), bool)
    s, _, _ = statement_scores(a, b, obs_mask=mask, bb_min=[0.0, 0.0, 0.0], res=10.0, plane=[0.0, 0.0, -1.0, -5.0])
    assert s["n_data_used"] == 0 and s["n_gt_used"] == 0 and s["n_data_thinned"] == len(a)
    assert all(np.isnan(s[k]) for k in ("accuracy_mean", "accuracy_median", "completeness_mean", "completeness_median",
                                        "overall"))
    far, _, _ = statement_scores(a, b + np.float32(100.0))                   # everything beyond max_dist
    assert far["n_data_used"] == 0 and far["n_gt_used"] == 0 and np.isnan(far["overall"])
    assert lower_median(np.array([4.0, 1.0, 3.0, 2.0])) == 2.0               # torch.median's convention
    assert float(torch.median(torch.tensor([4.0, 1.0, 3.0, 2.0]))) == 2.0


def _write_rich_ply(path, pts, n_faces=3):
    """x y z float, normals, a double property BEFORE y to break any fixed layout, colours, then a face element."""
    rng = np.random.default_rng(5)
    dt = np.dtype([("x", "<f4"), ("q", "<f8"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                   ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("s", "<i2")])
    v = np.zeros(len(pts), dt)
    for c, n in enumerate("xyz"):
        v[n] = pts[:, c]
    v["q"] = rng.normal(size=len(pts))
    v["nx"] = 1.0
    v["red"] = 200
    head = "ply\nformat binary_little_endian 1.0\ncomment made by a test\nelement vertex %d\nproperty float x\n" \
           "property double q\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n" \
           "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty short s\nelement face %d\n" \
           "property list uchar int vertex_indices\nend_header\n" % (len(pts), n_faces)
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(v.tobytes())
        for k in range(n_faces):
            f.write(np.uint8(3).tobytes() + np.array([k, k + 1, k + 2], "<i4").tobytes())


def test_load_ply_points_and_the_dtu_mat_files(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(41, 3)).astype(np.float32)
    _write_rich_ply(str(tmp_path / "rich.ply"), pts)
    got = IO.load_ply_points(str(tmp_path / "rich.ply"))
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, pts)
    with pytest.raises(Exception):
        IO.load_ply(str(tmp_path / "rich.ply"))                              # load_ply stays strict
    IO.write_ply(str(tmp_path / "plain.ply"), pts, rng.integers(0, 256, (41, 3), dtype=np.uint8))
    assert np.array_equal(IO.load_ply_points(str(tmp_path / "plain.ply")), pts)
    IO.write_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.float32))
    assert IO.load_ply_points(str(tmp_path / "empty.ply")).shape == (0, 3)
    with open(str(tmp_path / "ascii.ply"), "wb") as f:
        f.write(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(Exception):
        IO.load_ply_points(str(tmp_path / "ascii.ply"))
    sio = pytest.importorskip("scipy.io")
    mask = rng.random((5, 6, 7)) < 0.4
    sio.savemat(str(tmp_path / "ObsMask9_10.mat"), {"ObsMask": mask, "BB": np.array([[-1.5, 2.0, 3.0], [10.0, 11.0, 12.0]]),
                                                    "Res": 0.25, "MaskName": "x"})
    m, bb, res = IO.load_dtu_obs_mask(str(tmp_path / "ObsMask9_10.mat"))
    assert m.dtype == bool and m.shape == (5, 6, 7) and m.flags["C_CONTIGUOUS"] and np.array_equal(m, mask)
    assert np.array_equal(bb, [-1.5, 2.0, 3.0]) and res == 0.25
    sio.savemat(str(tmp_path / "Plane9.mat"), {"P": np.array([[0.1], [-0.2], [0.97], [-3.5]])})
    assert np.array_equal(IO.load_dtu_plane(str(tmp_path / "Plane9.mat")), [0.1, -0.2, 0.97, -3.5])
    sio.savemat(str(tmp_path / "other.mat"), {"Mask": mask.astype(np.uint8), "Box": np.zeros((2, 3)), "R": 2.0, "Q": np.ones(4)})
    m, bb, res = IO.load_dtu_obs_mask(str(tmp_path / "other.mat"), mask_name="Mask", bb_name="Box", res_name="R")
    assert np.array_equal(m, mask) and res == 2.0
    assert np.array_equal(IO.load_dtu_plane(str(tmp_path / "other.mat"), plane_name="Q"), np.ones(4))
    with pytest.raises(KeyError):
        IO.load_dtu_obs_mask(str(tmp_path / "Plane9.mat"))


def test_abi_still_agrees_with_the_new_symbols(lib_built):
    import test_abi
    test_abi.test_header_library_and_bindings_agree(lib_built)
    from pointmvsnet_amd import _lib, build
    names = {"pf_cloud_cell_keys_f32", "pf_cloud_pack_f32", "pf_cloud_thin_round", "pf_cloud_nn_cells_f32",
             "pf_cloud_nn_wave_f32", "pf_cloud_obs_mask_f32", "pf_cloud_above_plane_f32"}
    assert names <= set(_lib.PROTOTYPES) and "cloud_eval.hip" in build.SOURCES
    usage = json.load(open(build.USAGE_FILE))["cloud_eval.hip"]
    kernels = [k for k in usage if "cloud_" in k]
    assert len(kernels) == 7
    for k in kernels:
        assert usage[k]["scratch_bytes_per_lane"] == 0, k
    assert EV.MAX_CELLS == 131072 and "#define PF_CLOUD_MAX_CELLS 131072" in open(
        os.path.join(ROOT, "include", "pointflow_hip.h")).read()


def test_evaluation_has_no_cpu_path():
    pts = torch.from_numpy(noisy_sheet(100, 5.0, 0))
    for call in (lambda: EV.thin_points(pts), lambda: EV.nearest_distances(pts, pts),
                 lambda: EV.in_obs_mask(pts, torch.ones(2, 2, 2, dtype=torch.bool), [0.0, 0.0, 0.0], 1.0),
                 lambda: EV.above_plane(pts, [0.0, 0.0, 1.0, 0.0]), lambda: EV.evaluate_point_cloud(pts, pts)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


# ---------------------------------------------------------------------------------------------------------------------
# 2. on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _thin(dev, cloud):
    kept, idx = EV.thin_points(torch.from_numpy(cloud).to(dev), MIN_DIST, return_index=True)
    return kept.cpu(), idx.cpu(), EV.last_thinning_rounds()


@pytest.mark.gpu
def test_thinning_equals_the_statement_exactly(dev):
    sheet = noisy_sheet(220000, 100.0, 7)
    sheet = np.concatenate([sheet, sheet[1000:1100]])                        # exact duplicates must be thinned
    for name, raw in (("sheet", sheet), ("grid", grid_cloud())):
        cloud, dropped = drop_band_pairs(raw)
        assert len(cloud) >= 100000 and (name != "sheet" or len(cloud) >= 200000)
        want = statement_thin(cloud)
        _, want_rounds = statement_thin_rounds(cloud)
        kept, idx, rounds = _thin(dev, cloud)
        print(name, "points", len(cloud), "band pairs dropped", dropped, "kept", len(want), "rounds", rounds, want_rounds)
        report("evaluation_thinning_" + name, points=len(cloud), band_pairs_dropped=dropped, kept=len(want),
               kept_gpu=int(idx.numel()), rounds=rounds, rounds_statement=want_rounds,
               index_sets_differ=int(len(np.setxor1d(idx.numpy(), want))))
        assert idx.dtype == torch.int64 and np.array_equal(idx.numpy(), want)
        assert torch.equal(kept, torch.from_numpy(cloud)[idx])                # input order, the points themselves
        assert rounds == want_rounds                                          # the double-buffered rounds ARE the parallel form
        kept2, idx2, _ = _thin(dev, cloud)
        assert torch.equal(idx2, idx) and kept2.numpy().tobytes() == kept.numpy().tobytes()
    assert (np.diff(np.sort(idx.numpy())) > 0).all()
    few = torch.from_numpy(sheet[:3]).to(dev)
    assert EV.thin_points(few[:0]).shape == (0, 3) and EV.thin_points(few[:1]).shape == (1, 3)
    assert torch.equal(EV.thin_points(torch.cat([few[:1], few[:1]]), return_index=True)[1].cpu(),
                       torch.tensor([0 if keys_of(2)[0] < keys_of(2)[1] else 1]))
    with pytest.raises(ValueError):
        EV.thin_points(torch.tensor([[0.0, float("nan"), 0.0]], device=dev))


def _check_distances(dev, name, query, target, max_dist=MAX_DIST):
    d64, _ = statement_distances(query, target)
    assert not (np.abs(d64 / max_dist - 1.0) <= BAND).any()                  # no query near the cap
    q, t = torch.from_numpy(query).to(dev), torch.from_numpy(target).to(dev)
    d, idx = EV.nearest_distances(q, t, max_dist, return_index=True)
    unfinished = EV.last_unfinished_queries()
    d2 = EV.nearest_distances(q, t, max_dist)
    d, idx = d.cpu().numpy(), idx.cpu().numpy()
    assert d.dtype == np.float32 and idx.dtype == np.int64 and d.shape == (len(query),)
    assert d2.cpu().numpy().tobytes() == d.tobytes()                          # two runs: identical bytes
    inside = d64 < max_dist
    cap = np.float32(max_dist)
    assert (d[~inside] == cap).all() and (idx[~inside] == -1).all()
    err = np.abs(d[inside].astype(np.float64) - d64[inside]) / np.maximum(d64[inside], 1e-300)
    err[d64[inside] == 0] = np.abs(d[inside][d64[inside] == 0])
    worst = float(err.max()) if err.size else 0.0
    assert (idx[inside] >= 0).all() and (idx[inside] < len(target)).all()
    back = np.sqrt(((query[inside].astype(np.float64) - target[idx[inside]].astype(np.float64)) ** 2).sum(axis=1))
    err_back = np.abs(d[inside].astype(np.float64) - back) / np.maximum(back, 1e-300)
    err_back[back == 0] = np.abs(d[inside][back == 0])
    worst_back = float(err_back.max()) if err_back.size else 0.0
    print(name, "queries", len(query), "targets", len(target), "inside", int(inside.sum()), "unfinished after the cell pass",
          unfinished, "rel err", worst, "rel err from the index", worst_back)
    report("evaluation_distances_" + name, queries=len(query), targets=len(target), inside=int(inside.sum()),
           unfinished=unfinished, rel_err_max=worst, rel_err_from_index_max=worst_back, tol=DIST_TOL)
    assert worst <= DIST_TOL and worst_back <= DIST_TOL
    return unfinished


def _drop_near_cap(query, target, max_dist=MAX_DIST):
    d64, _ = statement_distances(query, target)
    return np.ascontiguousarray(query[np.abs(d64 / max_dist - 1.0) > BAND])


@pytest.mark.gpu
def test_distances_match_the_float64_statement(dev):
    rng = np.random.default_rng(11)
    for name, offset in (("origin", 0.0), ("offset_1e4", 1.0e4)):
        target = noisy_sheet(150001, 120.0, 3, offset=offset)                # not a multiple of the block size
        inliers = target[rng.integers(0, len(target), 100003)] + rng.normal(0.0, 0.08, (100003, 3)).astype(np.float32)
        middle = target[rng.integers(0, len(target), 3001)] + np.array([0.0, 0.0, 1.0], np.float32) * \
            rng.uniform(1.0, 25.0, (3001, 1)).astype(np.float32)             # 1 .. 25 off the sheet: both sides of the cap
        lo, hi = target.min(axis=0), target.max(axis=0)
        far = rng.uniform(lo - 150.0, hi + 150.0, (5000, 3)).astype(np.float32)
        block = (np.array([60.0, 60.0, 300.0]) + offset + rng.uniform(0.0, 5.0, (1999, 3))).astype(np.float32)
        query = _drop_near_cap(np.concatenate([inliers, target[:500], middle, far, block]), target)
        unfinished = _check_distances(dev, name, query, target)
        assert 0 < unfinished < len(query) // 4                              # both passes ran
    one = target[:1]
    _check_distances(dev, "single_target", _drop_near_cap(np.concatenate([inliers[:2000], far[:300]]), one), one)
    q = torch.from_numpy(inliers[:777]).to(dev)
    d, idx = EV.nearest_distances(q, q[:0], MAX_DIST, return_index=True)
    assert (d.cpu() == MAX_DIST).all() and (idx.cpu() == -1).all() and d.shape == (777,)
    d, idx = EV.nearest_distances(q[:0], q, MAX_DIST, return_index=True)
    assert d.shape == (0,) and idx.shape == (0,)
    # a small cap: the fine pass alone covers it; and a larger one
    small = _drop_near_cap(np.concatenate([inliers[:5000], middle]), target, 0.3)
    _check_distances(dev, "cap_0.3", small, target, 0.3)
    with pytest.raises(ValueError):
        EV.nearest_distances(torch.tensor([[0.0, float("inf"), 0.0]], device=dev), q)


@pytest.mark.gpu
def test_filters_match_the_statement(dev):
    rng = np.random.default_rng(2)
    mask = rng.random((23, 17, 31)) < 0.5
    bb_min, res = np.array([-3.0, 4.0, 100.0]), 0.7
    size = np.array(mask.shape) * res
    pts = rng.uniform(bb_min - 0.3 * size, bb_min + 1.3 * size, (200003, 3)).astype(np.float32)    # outside on every side
    want, margin = statement_obs_mask(pts, mask, bb_min, res)
    ok = margin >= 1e-4
    pts, want = np.ascontiguousarray(pts[ok]), want[ok]
    assert statement_obs_mask(pts, mask, bb_min, res)[1].min() >= 1e-4 and 0.05 < want.mean() < 0.6
    for axis in range(3):
        assert (pts[:, axis] < bb_min[axis] - res).any() and (pts[:, axis] > bb_min[axis] + size[axis] + res).any()
    got = EV.in_obs_mask(torch.from_numpy(pts).to(dev), torch.from_numpy(mask), bb_min, res).cpu().numpy()
    assert got.dtype == bool and np.array_equal(got, want)
    plane = np.array([0.2, -0.3, 0.9, -95.0])
    want_p, rel = statement_plane(pts, plane)
    okp = rel >= 1e-4
    got_p = EV.above_plane(torch.from_numpy(np.ascontiguousarray(pts[okp])).to(dev), plane).cpu().numpy()
    assert np.array_equal(got_p, want_p[okp]) and 0.1 < want_p[okp].mean() < 0.9
    report("evaluation_filters", points=len(pts), mask_mismatches=int((got != want).sum()),
           plane_mismatches=int((got_p != want_p[okp]).sum()))


def _assert_scores(got, want, tol=DIST_TOL):
    for k in ("n_data", "n_data_thinned", "n_data_used", "n_gt", "n_gt_used"):
        assert got[k] == want[k] and isinstance(got[k], int), k
    worst = 0.0
    for k in ("accuracy_mean", "accuracy_median", "completeness_mean", "completeness_median", "overall"):
        assert isinstance(got[k], float), k
        if np.isnan(want[k]):
            assert np.isnan(got[k]), k
            continue
        rel = abs(got[k] - want[k]) / want[k] if want[k] else abs(got[k])
        worst = max(worst, rel)
        assert rel <= tol, (k, got[k], want[k])
    return worst


@pytest.mark.gpu
def test_scores_match_the_statement(dev):
    rng = np.random.default_rng(4)
    data = noisy_sheet(60000, 50.0, 21, noise=0.3)
    data = np.concatenate([data, rng.uniform([-40.0, -40.0, -60.0], [90.0, 90.0, 60.0], (1200, 3)).astype(np.float32)])
    gt = sampled_plane(300, 300, 0.2, 0.0)
    gt[:, 2] = 0.02 * gt[:, 0]
    mask = np.zeros((30, 30, 8), bool)
    mask[2:27, 3:28, 1:7] = True
    bb_min, res, plane = np.array([-5.0, -5.0, -8.0]), 2.0, np.array([0.0, 1.0, 0.0, -12.3456])
    # keep the yardstick's own decisions away from its bands (cap, voxel boundaries, plane) for EVERY point, so that
    # whatever the thinning keeps is clear of them
    data = data[statement_obs_mask(data, mask, bb_min, res)[1] >= 1e-4]
    data = np.ascontiguousarray(data[np.abs(statement_distances(data, gt)[0] / MAX_DIST - 1) > BAND])
    gt = np.ascontiguousarray(gt[statement_plane(gt, plane)[1] >= 1e-4])
    data, _ = drop_band_pairs(data)
    kept = statement_thin(data)
    d_comp, _ = statement_distances(gt, data[kept])
    assert not (np.abs(d_comp / MAX_DIST - 1) <= BAND).any()
    assert not (np.abs(statement_distances(gt, data)[0] / MAX_DIST - 1) <= BAND).any()      # (thin=False)
    for kw in ({}, {"obs_mask": mask, "bb_min": bb_min, "res": res, "plane": plane}, {"thin": False}):
        want, w_acc, w_comp = statement_scores(data, gt, kept=kept, **kw)
        got = EV.evaluate_point_cloud(torch.from_numpy(data).to(dev), torch.from_numpy(gt).to(dev), return_distances=True,
                                      **{k: (torch.from_numpy(v) if k == "obs_mask" else v) for k, v in kw.items()})
        tensors = {k: got.pop(k) for k in ("data_thinned", "d_acc", "d_comp", "acc_used", "comp_used")}
        worst = _assert_scores(got, want)
        print(sorted(kw), "gpu", got, "statement", want, "worst rel", worst)
        report("evaluation_scores_" + ("_".join(sorted(kw)) or "default"), worst_rel=worst, tol=DIST_TOL,
               accuracy_mean=got["accuracy_mean"], completeness_mean=got["completeness_mean"])
        assert 0 < want["n_data_used"] < want["n_data_thinned"] and 0 < want["n_gt_used"] <= want["n_gt"]
        if kw.get("thin", True):
            assert torch.equal(tensors["data_thinned"].cpu(), torch.from_numpy(data[kept]))
        assert int(tensors["acc_used"].sum()) == want["n_data_used"] and tensors["acc_used"].dtype == torch.bool
        again = EV.evaluate_point_cloud(torch.from_numpy(data).to(dev), torch.from_numpy(gt).to(dev), return_distances=True,
                                        **{k: (torch.from_numpy(v) if k == "obs_mask" else v) for k, v in kw.items()})
        for k, v in tensors.items():
            assert again[k].cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), k
        assert all(again[k] == got[k] or (np.isnan(again[k]) and np.isnan(got[k])) for k in got)
    # closed forms on the GPU: two lattices delta apart, a cloud against itself, filters that exclude everything
    a, b = sampled_plane(120, 90, 0.25, 0.0), sampled_plane(120, 90, 0.25, 0.75)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    s = EV.evaluate_point_cloud(ta, tb)
    assert s["n_data_thinned"] == len(a) and s["accuracy_mean"] == 0.75 and s["completeness_median"] == 0.75
    assert EV.evaluate_point_cloud(ta, ta)["overall"] == 0.0
    s = EV.evaluate_point_cloud(ta, tb, obs_mask=torch.zeros(4, 4, 4, dtype=torch.bool), bb_min=[0.0, 0.0, 0.0], res=10.0,
                                plane=[0.0, 0.0, -1.0, -5.0])
    assert s["n_data_used"] == 0 and s["n_gt_used"] == 0 and np.isnan(s["accuracy_mean"]) and np.isnan(s["overall"])
    s = EV.evaluate_point_cloud(ta[:0], tb)
    assert s["n_data"] == 0 and s["n_gt_used"] == 0 and np.isnan(s["completeness_mean"])


def make_plane_scan(V=5, h=96, w=128, sigma=0.3, seed=0):
    """V cameras 60 apart on a line, looking at a tilted plane 600 away; depth maps by ray-plane intersection plus Gaussian
    noise of ``sigma``.  Returns depths, K, E, the plane (n, c with n . X = c) and the world size of a pixel on the plane."""
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
        R = np.stack([right, np.cross(fwd, right), fwd])
        d = (n @ target - n @ centre) / (rays @ (R @ n))
        depths.append((d + rng.normal(0.0, sigma, d.shape)).astype(np.float32))
        Es.append(np.concatenate([R, (-R @ centre)[:, None]], 1))
    return np.stack(depths), np.stack([K] * V), np.stack(Es), (n, float(n @ target)), 600.0 / f


@pytest.mark.gpu
def test_end_to_end_fused_scan_scored_from_ply_files(dev, tmp_path):
    from pointmvsnet_amd import fusion
    sigma = 0.3
    depths, K, E, (n, c), pixel = make_plane_scan(sigma=sigma)
    pts, _ = fusion.fuse_depth_maps(torch.from_numpy(depths).to(dev), K, E)
    assert pts.shape[0] > 5000
    IO.write_ply(str(tmp_path / "final3d_model.ply"), pts.cpu().numpy())
    # ground truth: the plane sampled at 0.2 pitch over the footprint of the fused cloud plus a margin, so that every
    # fused point has the plane below it; completeness is judged in the middle, which the central view covers
    data = pts.cpu().numpy()
    u = np.cross(n, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    centre = np.array([0.0, 0.0, 600.0])
    cu, cv = (data - centre) @ u, (data - centre) @ v
    gu, gv = np.meshgrid(np.arange(cu.min() - 2.0, cu.max() + 2.0, 0.2), np.arange(cv.min() - 2.0, cv.max() + 2.0, 0.2),
                         indexing="ij")
    gt = (centre + gu[..., None] * u + gv[..., None] * v).reshape(-1, 3).astype(np.float32)
    half_u, half_v = 0.3 * depths.shape[2] * pixel, 0.3 * depths.shape[1] * pixel
    middle = (np.abs(gu) < half_u).reshape(-1) & (np.abs(gv) < half_v).reshape(-1)
    assert 1000 < middle.sum() < len(gt)
    IO.write_ply(str(tmp_path / "gt.ply"), gt)
    got = EV.evaluate_ply(str(tmp_path / "final3d_model.ply"), str(tmp_path / "gt.ply"), device=dev, return_distances=True)
    thinned = got.pop("data_thinned").cpu().numpy()
    d_comp = got.pop("d_comp").cpu().numpy()
    for k in ("d_acc", "acc_used", "comp_used"):
        got.pop(k)
    # the thinned set, checked with float64 alone: a subset of the cloud in input order, independent inside the band,
    # and every removed point has a kept one within the band's outer edge
    t = float(np.float32(MIN_DIST))
    tree = cKDTree(thinned.astype(np.float64))
    assert len(tree.query_pairs(t * (1 - BAND))) == 0
    assert (tree.query(data.astype(np.float64))[0] < t * (1 + BAND)).all()
    pos = cKDTree(data.astype(np.float64)).query(thinned.astype(np.float64))
    assert (pos[0] == 0).all()
    want, _, _ = statement_scores(thinned, gt, thin=False)
    want["n_data"], want["n_data_thinned"] = len(data), len(thinned)
    worst = _assert_scores(got, want)
    print("end to end: gpu", got, "statement", want, "pixel on the plane", pixel, "worst rel", worst)
    report("evaluation_end_to_end", points=len(data), thinned=len(thinned), accuracy_mean=got["accuracy_mean"],
           completeness_mean=got["completeness_mean"], completeness_mean_middle=float(d_comp[middle].mean()),
           worst_rel=worst, tol=DIST_TOL)
    assert 0.02 * sigma < got["accuracy_mean"] < 3.0 * sigma                  # of the order of the depth noise put in
    assert float(d_comp[middle].mean()) < 2.0 * pixel and got["n_gt_used"] == len(gt)   # covered: a point within ~a pixel
    assert got["n_data_used"] <= got["n_data_thinned"] <= got["n_data"] == len(data)
    # the command-line tool prints the same dict as one JSON line
    import subprocess
    import sys
    if dev.type == "cuda":
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "evaluate_dtu.py"), "--data",
                                       str(tmp_path / "final3d_model.ply"), "--gt", str(tmp_path / "gt.ply")])
        line = json.loads(out.decode().strip().splitlines()[-1])
        assert line == {k: v for k, v in got.items()}
