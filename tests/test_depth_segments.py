"""Depth-map segments, speckle removal and gap filling (pointmvsnet_amd/depth_segments.py, csrc/depth_segments.hip) against a
NumPy float32 statement written here from the module's docstring alone: link masks from shifted slices, components from a
plain union-find (cross-checked with scipy.sparse.csgraph where SciPy is importable), labels as the smallest flat index per
component, the gap fill as a literal loop.  Every comparison is exact: torch.equal, no pixel excused, no tolerance."""
import numpy as np
import pytest
import torch

from pointmvsnet_amd import depth_segments as DS
from pointmvsnet_amd import scan as S

REL, DMIN, DMAX = 0.01, 1e-3, 1e5


# ---- the statement ------------------------------------------------------------------------------------------------------
def ref_valid(d, dmin=DMIN, dmax=DMAX):
    with np.errstate(invalid="ignore"):
        return (d > np.float32(dmin)) & (d < np.float32(dmax))


def ref_links(d, rel=REL, dmin=DMIN, dmax=DMAX):
    """(right (V, h, w-1), down (V, h-1, w)) link masks."""
    ok, rel = ref_valid(d, dmin, dmax), np.float32(rel)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = d[:, :, :-1], d[:, :, 1:]
        right = ok[:, :, :-1] & ok[:, :, 1:] & (np.abs(a - b) <= rel * np.minimum(a, b))
        a, b = d[:, :-1, :], d[:, 1:, :]
        down = ok[:, :-1, :] & ok[:, 1:, :] & (np.abs(a - b) <= rel * np.minimum(a, b))
    return right, down


def ref_segments(d, rel=REL, dmin=DMIN, dmax=DMAX):
    """(labels, sizes) int32 (V, h, w)."""
    V, h, w = d.shape
    n = V * h * w
    ok = ref_valid(d, dmin, dmax).reshape(-1)
    right, down = ref_links(d, rel, dmin, dmax)
    index = np.arange(n, dtype=np.int64).reshape(V, h, w)
    pairs = np.concatenate([np.stack([index[:, :, :-1][right], index[:, :, 1:][right]], 1),
                            np.stack([index[:, :-1, :][down], index[:, 1:, :][down]], 1)])
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)                  # the root is the smallest index of its component
    labels = np.array([find(x) for x in range(n)], dtype=np.int64)
    labels[~ok] = -1
    sizes = np.zeros(n, dtype=np.int64)
    if ok.any():
        counts = np.bincount(labels[ok], minlength=n)
        sizes[ok] = counts[labels[ok]]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        pass
    else:
        if n:
            graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
            comp = connected_components(graph, directed=False)[1]
            first = np.full(comp.max() + 1, n, dtype=np.int64)
            np.minimum.at(first, comp, np.arange(n))
            assert np.array_equal(np.where(ok, first[comp], -1), labels)
    return labels.reshape(V, h, w).astype(np.int32), sizes.reshape(V, h, w).astype(np.int32)


def ref_speckles(d, sizes, min_size, dmin=DMIN, dmax=DMAX):
    ok = ref_valid(d, dmin, dmax)
    keep = ok & (sizes >= min_size)
    return np.where(keep, d, np.float32(0)).astype(np.float32), (ok & ~keep).astype(np.uint8)


def _candidate(line, ok, pos, max_gap, rel):
    lo = pos - 1
    while lo >= 0 and not ok[lo]:
        lo -= 1
    hi = pos + 1
    while hi < len(line) and not ok[hi]:
        hi += 1
    if lo < 0 or hi >= len(line) or hi - lo - 1 > max_gap:
        return None
    dl, dr = line[lo], line[hi]
    if not np.abs(dl - dr) <= (np.float32(rel) * np.float32(hi - lo)) * min(dl, dr):
        return None
    return dl + (np.float32(pos - lo) / np.float32(hi - lo)) * (dr - dl)


def ref_fill(d, max_gap, rel=REL, dmin=DMIN, dmax=DMAX):
    ok = ref_valid(d, dmin, dmax)
    out = np.where(ok, d, np.float32(0)).astype(np.float32)
    filled = np.zeros(d.shape, dtype=np.uint8)
    for v, y, x in zip(*np.nonzero(~ok)):
        dh = _candidate(d[v, y, :], ok[v, y, :], x, max_gap, rel)
        dv = _candidate(d[v, :, x], ok[v, :, x], y, max_gap, rel)
        if dh is not None and dv is not None:
            out[v, y, x] = np.float32(0.5) * (dh + dv)
        elif dh is not None or dv is not None:
            out[v, y, x] = dh if dh is not None else dv
        filled[v, y, x] = dh is not None or dv is not None
    assert out.dtype == np.float32
    return out, filled


# ---- helpers --------------------------------------------------------------------------------------------------------------
def same(got, want):
    """Bit for bit (floats compared as their int32 bits: a NaN would otherwise never be equal, and -0 always)."""
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == torch.float32:
        got, want = got.view(torch.int32), want.view(torch.int32)
    return torch.equal(got, want)


def check_segments(dev, d, rel=REL, dmin=DMIN, dmax=DMAX):
    """labels and sizes of ``d`` against the statement; returns the statement's ``(labels, sizes)``."""
    labels, sizes = ref_segments(d, rel, dmin, dmax)
    t = torch.from_numpy(d).to(dev)
    got_l, got_s = DS.depth_segments(t, rel, dmin, dmax, return_sizes=True)
    assert same(got_l, labels)
    assert same(got_s, sizes)
    assert same(DS.depth_segments(t, rel, dmin, dmax), labels)
    return labels, sizes


def random_scene(seed=0):
    """Piecewise-smooth depths around 500 with steps, noise that puts many neighbours near the rel_jump threshold (5 at
    depth 500), 20 % holes and a few values that are not depths at all."""
    tw, th = DS.tile_size()
    V, h, w = 3, 2 * th + 5, 2 * tw + 3
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.empty((V, h, w), dtype=np.float32)
    for v in range(V):
        plane = 500.0 + 0.5 * xx + 0.3 * yy + 7.0 * v
        for _ in range(6):
            y0, x0 = rng.randint(0, h), rng.randint(0, w)
            plane[y0:y0 + rng.randint(3, h), x0:x0 + rng.randint(3, w)] += rng.choice([-60.0, 40.0, 90.0])
        d[v] = plane + rng.uniform(-3.6, 3.6, size=(h, w))
    d[rng.rand(V, h, w) < 0.2] = 0.0
    flat = d.reshape(-1)
    for value in (np.nan, np.inf, -np.inf, -500.0, 1e5, 2e5, 1e-3, 5e-4):
        flat[rng.choice(flat.size, 4, replace=False)] = value
    return d


@pytest.fixture(scope="module")
def scene():
    d = random_scene()
    labels, sizes = ref_segments(d)
    return d, labels, sizes


def percolation(shape, seed=1, p=0.59):
    rng = np.random.RandomState(seed)
    return np.where(rng.rand(*shape) < p, np.float32(500), np.float32(0)).astype(np.float32)


def spiral(h, w):
    m = np.zeros((h, w), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        for _ in range(2):                                      # straight on if the way is free, else one turn to the right
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            free = 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ay < h and 0 <= ax < w and m[ay, ax])
            if free:
                break
            dy, dx = dx, -dy
        if not free:
            return m
        y, x = ny, nx
        m[y, x] = True


def serpentine(h, w):
    m = np.zeros((h, w), dtype=bool)
    m[0::2] = True
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = True
    return m


def comb(h, w):
    m = np.zeros((h, w), dtype=bool)
    m[0] = True
    m[:, 0::2] = True
    return m


def as_depth(mask, depth=500.0):
    return np.where(mask, np.float32(depth), np.float32(0)).astype(np.float32)[None]


# ---- 1. random scene ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_random_scene_labels_and_sizes(dev, scene):
    d, labels, sizes = scene
    t = torch.from_numpy(d).to(dev)
    got_l, got_s = DS.depth_segments(t, return_sizes=True)
    assert same(got_l, labels) and same(got_s, sizes)
    assert same(DS.depth_segments(t), labels)
    stats = DS.last_segment_stats()
    assert stats["rounds"] >= 2 and stats["border_unions"] >= 1
    assert labels.max() > 0 and len(np.unique(sizes)) > 5       # the scene is neither one segment nor all singletons


@pytest.mark.gpu
@pytest.mark.parametrize("min_size", [2, 9, 100])
def test_random_scene_speckles(dev, scene, min_size):
    d, _, sizes = scene
    want, want_removed = ref_speckles(d, sizes, min_size)
    assert want_removed.any() and (want != 0).any()
    t = torch.from_numpy(d).to(dev)
    out, removed = DS.remove_speckles(t, min_size, return_removed=True)
    assert same(out, want) and same(removed, want_removed)
    assert same(DS.remove_speckles(t, min_size), want)


@pytest.mark.gpu
def test_min_size_of_one_or_less_removes_nothing(dev, scene):
    d, _, sizes = scene
    want, want_removed = ref_speckles(d, sizes, 1)
    assert not want_removed.any()
    t = torch.from_numpy(d).to(dev)
    for min_size in (0, 1):
        out, removed = DS.remove_speckles(t, min_size, return_removed=True)
        assert same(out, want) and same(removed, want_removed)  # NaN, inf and the other non-depths come out as 0


@pytest.mark.gpu
@pytest.mark.parametrize("max_gap", [1, 3, 7])
def test_random_scene_gaps(dev, scene, max_gap):
    d = scene[0]
    want, want_filled = ref_fill(d, max_gap)
    assert want_filled.any() and not want_filled[ref_valid(d)].any()
    t = torch.from_numpy(d).to(dev)
    out, filled = DS.fill_gaps(t, max_gap, return_filled=True)
    assert same(out, want) and same(filled, want_filled)
    assert same(DS.fill_gaps(t, max_gap), want)


@pytest.mark.gpu
def test_max_gap_of_zero_fills_nothing(dev, scene):
    d = scene[0]
    out, filled = DS.fill_gaps(torch.from_numpy(d).to(dev), 0, return_filled=True)
    assert same(out, np.where(ref_valid(d), d, np.float32(0)).astype(np.float32)) and not bool(filled.any())


def ref_clean(d, min_size, max_gap):
    report = {"valid_in": int(ref_valid(d).sum()), "segments": 0, "removed_segments": 0, "removed_pixels": 0,
              "filled_pixels": 0}
    out = np.where(ref_valid(d), d, np.float32(0)).astype(np.float32)
    if min_size > 1:
        labels, sizes = ref_segments(d)
        roots = labels.reshape(-1) == np.arange(labels.size)
        out, removed = ref_speckles(d, sizes, min_size)
        report.update(segments=int(roots.sum()), removed_segments=int((roots & (sizes.reshape(-1) < min_size)).sum()),
                      removed_pixels=int(removed.sum()))
    if max_gap > 0:
        out, filled = ref_fill(out, max_gap)
        report["filled_pixels"] = int(filled.sum())
    report["valid_out"] = int(ref_valid(out).sum())
    return out, report


@pytest.mark.gpu
@pytest.mark.parametrize("min_size,max_gap", [(9, 3), (1, 3), (9, 0), (0, 0)])
def test_random_scene_clean_and_its_report(dev, scene, min_size, max_gap):
    d = scene[0]
    want, want_report = ref_clean(d, min_size, max_gap)
    out, report = DS.clean_depth_maps(torch.from_numpy(d).to(dev), min_size=min_size, max_gap=max_gap)
    assert same(out, want)
    assert all(type(v) is int for v in report.values())
    assert {k: report[k] for k in want_report} == want_report
    if min_size > 1 and max_gap > 0:
        assert report["removed_pixels"] > 0 and report["filled_pixels"] > 0
        assert report["valid_out"] == report["valid_in"] - report["removed_pixels"] + report["filled_pixels"]


# ---- 2. percolation -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_percolation_mask_winds_through_many_tiles(dev):
    tw, th = DS.tile_size()
    d = percolation((3, 2 * th + 5, 2 * tw + 3))
    labels, sizes = check_segments(dev, d)
    assert DS.last_segment_stats()["border_unions"] >= 1
    out, report = DS.clean_depth_maps(torch.from_numpy(d).to(dev), min_size=9, max_gap=0)
    assert report["border_unions"] >= 1 and report["rounds"] >= 2             # the merge path, not only the tile kernel
    assert same(out, ref_speckles(d, sizes, 9)[0])
    assert report["segments"] == int((labels.reshape(-1) == np.arange(labels.size)).sum())


# ---- 3. shapes built to break a union-find --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["spiral", "serpentine", "comb"])
def test_one_segment_that_crosses_every_tile_border(dev, shape):
    tw, th = DS.tile_size()
    h, w = 3 * th + 1, 3 * tw + 1
    mask = {"spiral": spiral, "serpentine": serpentine, "comb": comb}[shape](h, w)
    labels, sizes = check_segments(dev, as_depth(mask))
    assert set(np.unique(labels)) == {-1, 0} and sizes.max() == mask.sum()    # the shape is what it was built to be
    assert DS.last_segment_stats()["border_unions"] >= 4


@pytest.mark.gpu
def test_checkerboard_every_pixel_its_own_segment(dev):
    tw, th = DS.tile_size()
    h, w = 2 * th + 1, 2 * tw + 1
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.stack([as_depth((yy + xx) % 2 == 0)[0], as_depth((yy + xx) % 2 == 1)[0]])
    labels, sizes = check_segments(dev, d)
    assert sizes.max() == 1 and DS.last_segment_stats()["border_unions"] == 0
    ok = labels >= 0
    assert np.array_equal(labels[ok], np.arange(labels.size).reshape(labels.shape)[ok])


@pytest.mark.gpu
def test_full_plane_is_one_segment_per_view(dev):
    tw, th = DS.tile_size()
    V, h, w = 2, 2 * th + 3, 2 * tw + 5
    d = np.full((V, h, w), 700.0, dtype=np.float32)
    labels, sizes = check_segments(dev, d)
    assert (sizes == h * w).all()
    assert np.array_equal(labels, np.broadcast_to((np.arange(V) * h * w).reshape(V, 1, 1), (V, h, w)))


# ---- 4. edges of the map --------------------------------------------------------------------------------------------------
def _edge_shapes():
    return ["small", "one_row", "one_column", "tile_multiple", "one_tile"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _edge_shapes())
def test_map_shapes(dev, name):
    tw, th = DS.tile_size()
    V, h, w = {"small": (2, 5, 7), "one_row": (2, 1, 2 * tw + 3), "one_column": (2, 2 * th + 3, 1),
               "tile_multiple": (2, 2 * th, 2 * tw), "one_tile": (1, th, tw)}[name]
    rng = np.random.RandomState(4)
    d = (500.0 + rng.uniform(-3.0, 3.0, size=(V, h, w))).astype(np.float32)
    d[rng.rand(V, h, w) < 0.15] = 0.0
    _, sizes = check_segments(dev, d)
    t = torch.from_numpy(d).to(dev)
    assert same(DS.remove_speckles(t, 4), ref_speckles(d, sizes, 4)[0])
    want, want_filled = ref_fill(d, 3)
    out, filled = DS.fill_gaps(t, 3, return_filled=True)
    assert same(out, want) and same(filled, want_filled)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(0, 5, 7), (2, 0, 7), (2, 5, 0)])
def test_empty_inputs_return_empty_outputs(dev, shape):
    t = torch.zeros(shape, dtype=torch.float32, device=dev)
    labels, sizes = DS.depth_segments(t, return_sizes=True)
    assert labels.shape == shape and labels.dtype == torch.int32 and sizes.shape == shape and sizes.dtype == torch.int32
    out, removed = DS.remove_speckles(t, return_removed=True)
    assert out.shape == shape and out.dtype == torch.float32 and removed.shape == shape and removed.dtype == torch.uint8
    out, filled = DS.fill_gaps(t, return_filled=True)
    assert out.shape == shape and out.dtype == torch.float32 and filled.shape == shape and filled.dtype == torch.uint8
    out, report = DS.clean_depth_maps(t)
    assert out.shape == shape and report["valid_in"] == report["valid_out"] == report["segments"] == 0
    assert DS.last_segment_stats()["rounds"] == 0


@pytest.mark.gpu
def test_no_links_around_the_end_of_a_row_or_of_a_view(dev):
    tw, th = DS.tile_size()
    h, w = 4, tw + 2
    rows = np.zeros((1, h, w), dtype=np.float32)                # the last pixel of a row equals the first of the next one
    for y in range(h):
        rows[0, y, 0], rows[0, y, w - 1] = 100.0 * 1.5 ** y, 100.0 * 1.5 ** (y + 1)
    assert all(rows[0, y, w - 1] == rows[0, y + 1, 0] for y in range(h - 1))
    labels, sizes = check_segments(dev, rows)
    assert sizes.max() == 1 and (labels >= 0).sum() == 2 * h
    views = np.full((2, th, w), 500.0, dtype=np.float32)        # the last row of view 0 equals the first row of view 1
    labels, sizes = check_segments(dev, views)
    assert (labels[0] == 0).all() and (labels[1] == th * w).all() and (sizes == th * w).all()
    holes = views.copy()
    holes[0, th - 1] = 0.0                                      # ... and a gap is not filled across views either
    out, filled = DS.fill_gaps(torch.from_numpy(holes).to(dev), 3, return_filled=True)
    assert same(out, holes) and not bool(filled.any())


# ---- 5. thresholds, exactly -----------------------------------------------------------------------------------------------
def _row(values):
    return np.array(values, dtype=np.float32).reshape(1, 1, -1)


@pytest.mark.gpu
def test_link_threshold_is_exact_and_uses_the_smaller_depth(dev):
    above = np.nextafter(np.float32(1.5), np.float32(2))
    for values, linked in (([1.0, 1.5], True), ([1.5, 1.0], True), ([1.0, above], False), ([above, 1.0], False),
                           ([1.0, 1.75], False), ([1.75, 1.0], False)):         # 0.75 <= 0.5 * 1.75, but not <= 0.5 * 1.0
        for d in (_row(values), _row(values).reshape(1, 2, 1)):                 # along a row and along a column
            labels, _ = check_segments(dev, d, rel=0.5, dmin=0.0, dmax=10.0)
            assert labels.reshape(-1).tolist() == ([0, 0] if linked else [0, 1])
    labels, _ = check_segments(dev, _row([1.0, 1.0, 2.0]), rel=0.0)             # rel_jump 0 links equal depths only
    assert labels.reshape(-1).tolist() == [0, 0, 2]


@pytest.mark.gpu
def test_validity_bounds_are_strict(dev):
    d = _row([1.0, 2.0, 4.0, np.nan, 3.0, np.inf, 0.0, -1.0])
    labels, _ = check_segments(dev, d, rel=0.0, dmin=1.0, dmax=4.0)
    assert labels.reshape(-1).tolist() == [-1, 1, -1, -1, 4, -1, -1, -1]


@pytest.mark.gpu
def test_a_segment_of_exactly_min_size_is_kept(dev):
    d = _row([500.0] * 5 + [0.0] + [600.0] * 4 + [0.0] + [700.0] * 6)
    t = torch.from_numpy(d).to(dev)
    out, removed = DS.remove_speckles(t, 5, return_removed=True)
    assert out.cpu().reshape(-1).tolist() == [500.0] * 5 + [0.0] * 6 + [700.0] * 6
    assert removed.cpu().reshape(-1).tolist() == [0] * 6 + [1] * 4 + [0] * 7
    _, sizes = ref_segments(d)
    assert same(out, ref_speckles(d, sizes, 5)[0])


@pytest.mark.gpu
def test_gap_rules_exactly(dev):
    def fill(values, max_gap, rel=0.01, column=False):
        d = _row(values)
        d = d.reshape(1, -1, 1) if column else d
        want, want_filled = ref_fill(d, max_gap, rel)
        out, filled = DS.fill_gaps(torch.from_numpy(d).to(dev), max_gap, rel, return_filled=True)
        assert same(out, want) and same(filled, want_filled)
        return out.cpu().reshape(-1).tolist()

    for column in (False, True):
        assert fill([8.0, 0.0, 0.0, 0.0, 8.0], 3, column=column) == [8.0] * 5              # a gap of exactly max_gap
        assert fill([8.0, 0.0, 0.0, 0.0, 0.0, 8.0], 3, column=column) == [8.0] + [0.0] * 4 + [8.0]
        # the ends agree at the gap's length: |8 - 9| <= (0.0625 * 2) * 8 holds, (0.03125 * 2) * 8 does not
        assert fill([8.0, 0.0, 9.0], 1, rel=0.0625, column=column) == [8.0, 8.5, 9.0]
        assert fill([9.0, 0.0, 8.0], 1, rel=0.0625, column=column) == [9.0, 8.5, 8.0]
        assert fill([8.0, 0.0, 9.0], 1, rel=0.03125, column=column) == [8.0, 0.0, 9.0]
        assert fill([0.0, 0.0, 8.0, 8.0], 3, column=column) == [0.0, 0.0, 8.0, 8.0]        # a gap at the border stays open
        assert fill([8.0, 8.0, 0.0], 3, column=column) == [8.0, 8.0, 0.0]
        assert fill([8.0, 0.0, 0.0, 0.0, 12.0], 3, rel=0.5, column=column) == [8.0, 9.0, 10.0, 11.0, 12.0]
        assert fill([8.0, np.nan, np.inf, -3.0, 12.0], 3, rel=0.5, column=column) == [8.0, 9.0, 10.0, 11.0, 12.0]


@pytest.mark.gpu
def test_a_hole_with_both_candidates_takes_their_mean_and_fills_do_not_cascade(dev):
    d = np.array([[0.0, 16.0, 0.0],
                  [8.0, 0.0, 8.0],
                  [0.0, 32.0, 0.0]], dtype=np.float32)[None]
    out = DS.fill_gaps(torch.from_numpy(d).to(dev), 1, rel_jump=0.5)
    assert float(out[0, 1, 1]) == 0.5 * (8.0 + 24.0)
    assert same(out, ref_fill(d, 1, 0.5)[0])
    # the hole at x = 2 has the end 8 at x = 1 and, at x = 4, nothing within max_gap = 1 ... unless it saw x = 3 filled
    d = _row([8.0, 8.0, 0.0, 0.0, 0.0, 8.0])
    d2 = np.concatenate([_row([0.0] * 6), d, _row([0.0] * 6)], axis=1)
    d2[0, 0, 3], d2[0, 2, 3] = 8.0, 8.0                        # x = 3 is filled along its column
    want, want_filled = ref_fill(d2, 1)
    out, filled = DS.fill_gaps(torch.from_numpy(d2).to(dev), 1, return_filled=True)
    assert same(out, want) and same(filled, want_filled)
    assert out[0, 1].cpu().tolist() == [8.0, 8.0, 0.0, 8.0, 0.0, 8.0]


# ---- 6. tile independence -------------------------------------------------------------------------------------------------
def _paddings():
    return [(a, b) for a in ("1", "th-1") for b in ("1", "tw-1")]


@pytest.mark.gpu
@pytest.mark.parametrize("pad", _paddings())
def test_results_do_not_depend_on_where_the_tiles_fall(dev, scene, pad):
    tw, th = DS.tile_size()
    dy = 1 if pad[0] == "1" else th - 1
    dx = 1 if pad[1] == "1" else tw - 1
    d, labels, sizes = scene
    V, h, w = d.shape
    H, W = h + dy, w + dx
    padded = np.zeros((V, H, W), dtype=np.float32)
    padded[:, dy:, dx:] = d
    v, y, x = np.unravel_index(np.maximum(labels, 0), (V, h, w))
    want_l = np.full((V, H, W), -1, dtype=np.int32)
    want_l[:, dy:, dx:] = np.where(labels >= 0, (v * H + y + dy) * W + x + dx, -1)
    want_s = np.zeros((V, H, W), dtype=np.int32)
    want_s[:, dy:, dx:] = sizes
    t = torch.from_numpy(padded).to(dev)
    got_l, got_s = DS.depth_segments(t, return_sizes=True)
    assert same(got_l, want_l) and same(got_s, want_s)
    want_o = np.zeros((V, H, W), dtype=np.float32)
    want_o[:, dy:, dx:] = ref_speckles(d, sizes, 9)[0]
    assert same(DS.remove_speckles(t, 9), want_o)
    # (the padding is holes at the border: it opens no gap that the unpadded map would not have)
    want_o[:, dy:, dx:] = ref_clean(d, 9, 3)[0]
    first, report = DS.clean_depth_maps(t, min_size=9, max_gap=3)
    assert same(first, want_o)
    second, again = DS.clean_depth_maps(t, min_size=9, max_gap=3)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    pure = [k for k in report if k not in ("rounds", "border_unions")]      # (those two are diagnostics of the run's schedule)
    assert len(pure) == 7 and [report[k] for k in pure] == [again[k] for k in pure]
    assert torch.equal(got_l, DS.depth_segments(t))


# ---- 7. arguments (no GPU) ------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_a_gpu_is_needed(lib_built):
    good = torch.full((1, 4, 4), 5.0)
    calls = (DS.depth_segments, DS.remove_speckles, DS.fill_gaps, DS.clean_depth_maps)
    for call in calls:
        for bad in (good.double(), good.int(), good[0], good[None], good.numpy(), None):
            with pytest.raises(ValueError):
                call(bad)
        for rel_jump in (-0.01, 0.51, float("nan")):
            with pytest.raises(ValueError, match="rel_jump"):
                call(good, rel_jump=rel_jump)
        for kwargs in ({"depth_min": -1.0}, {"depth_min": 2.0, "depth_max": 2.0}, {"depth_max": float("nan")}):
            with pytest.raises(ValueError, match="depth_min"):
                call(good, **kwargs)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(good)
    for call in (DS.fill_gaps, DS.clean_depth_maps):
        for max_gap in (-1, 33, 2.5, True):
            with pytest.raises(ValueError, match="max_gap"):
                call(good, max_gap=max_gap)
    for call in (DS.remove_speckles, DS.clean_depth_maps):
        for min_size in (-1, 2.5, False):
            with pytest.raises(ValueError, match="min_size"):
                call(good, min_size=min_size)
    with pytest.raises(ValueError, match="2\\^31"):                        # (a stride-0 view: no memory behind it)
        DS.depth_segments(torch.zeros((1,), dtype=torch.float32).expand(1, 2 ** 16, 2 ** 15))
    for bad in ([], "min_size", 3, ("min_size", 3)):
        with pytest.raises(ValueError, match="clean_depth"):
            S.ScanAccumulator(2, clean_depth=bad)
    for bad in ({"min_size": -1}, {"max_gap": 40}, {"rel_jump": 0.6}, {"speckle": 3}):
        with pytest.raises(ValueError):
            S.ScanAccumulator(2, clean_depth=bad)
    assert S.ScanAccumulator(2, clean_depth={}).clean_depth == {}
    assert S.ScanAccumulator(2).clean_depth is None
    assert DS.TILE_W == DS.tile_size()[0] and DS.TILE_H == DS.tile_size()[1] and DS.TILE_W * DS.TILE_H % 256 == 0


# ---- 8. the accumulator ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.isolated
def test_accumulator_cleans_what_filtered_returns(dev):
    from test_scan import FUSE, NAME, _model, scan_batches
    from pointmvsnet_amd.fusion import fuse_depth_maps
    batches, img_scales, inter_scales = scan_batches(dev)
    net = _model(dev)
    settings = {"min_size": 6, "max_gap": 2, "rel_jump": 0.02}
    thresholds = {"init_prob_threshold": 0.0, "flow_prob_threshold": 0.21}
    plain, twin = (S.ScanAccumulator(len(batches), name=NAME, **thresholds) for _ in range(2))
    cleaning = S.ScanAccumulator(len(batches), name=NAME, clean_depth=settings, **thresholds)
    with torch.no_grad():
        for batch, _ in batches:
            out = net(batch, img_scales, inter_scales, isFlow=True, isTest=True)
            for acc in (plain, twin, cleaning):
                acc.add(batch, out)

    def bits(t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t

    # without the option: what it returned before
    want, want_kept = S.filter_depth_maps(*plain.predictions(), mode=plain.mode, return_kept=True, **thresholds)
    assert torch.equal(bits(plain.filtered()), bits(want)) and torch.equal(bits(twin.filtered()), bits(want))
    assert plain.last_depth_report is None
    for a, b in zip(plain.fuse(**FUSE), twin.fuse(**FUSE)):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(plain.normals()), bits(twin.normals()))
    # with it: filtered() is the cleaned map, kept the confidence filter's own count
    cleaned, report = DS.clean_depth_maps(want, **settings)
    got, kept = cleaning.filtered(return_kept=True)
    assert torch.equal(bits(got), bits(cleaned)) and torch.equal(kept, want_kept)
    pure = [k for k in report if k not in ("rounds", "border_unions")]
    assert len(pure) == 7 and [cleaning.last_depth_report[k] for k in pure] == [report[k] for k in pure]
    print("depth report of the accumulator's scan:", report)
    assert 0 < report["valid_in"] < want.numel()                 # the thresholds leave something to segment, and holes
    K, E = cleaning.cameras()
    fused = fuse_depth_maps(cleaned, K, E, images=cleaning.images(), **FUSE)
    for a, b in zip(cleaning.fuse(**FUSE), fused):
        assert torch.equal(bits(a), bits(b))
