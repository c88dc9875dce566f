"""Guided depth upsampling (pointmvsnet_amd/refine.py, csrc/depth_refine.hip) against two NumPy statements of its
specification, written from the module's docstring (plain loops over the taps, no code shared with the product):

* ``statement(...)["out32"]``: every operation in float32 in the stated order -- what the kernel must return bit for bit;
* ``statement(...)["out64"]``: the same float32 tables and the same float32 decisions (anchor, links), the weights' products,
  the two sums and the quotient in float64 -- what the rounding bound below is measured against.

The bound (test_statement_pair_agrees_within_the_derived_bound)
---------------------------------------------------------------
``u = 2^-24``, ``T = (2 radius + 1)^2`` taps, ``J`` the largest ``|d - d0|`` among the pixel's linked taps; ``d - d0`` is exact
(Sterbenz: ``rel_jump <= 0.5``).  Per linked tap the float32 weight is ``w (1 + e1)(1 + e2)``: two rounded products, 2 u.
``W32``: T positive terms, each 2 u off, summed one after another with at most (T - 1) u relative to the sum:
``W32 = W (1 + th)``, ``|th| <= (T + 1) u``.  ``S32``: each term ``w * diff`` carries the weight's 2 u and its own product's u,
3 u of ``|w diff| <= w J``; the T - 1 additions each round relative to a partial sum no larger than ``J W``:
``|S32 - S| <= (T + 2) u J W``.  The quotient: ``|S32 / W32 - S / W| <= (T + 2) u J + |S / W| (T + 1) u + u |S / W|``, and
``|S / W| <= J``: ``(2 T + 4) u J``.  The last addition rounds once, ``u |out|``.  All of that is to first order in ``u``; the
terms of second order are smaller than ``(2 T + 4) u J`` by a factor ``(T + 2) u < 2e-5`` and are covered by one more ``u J``:

    ``|out32 - out64| <= u |out64| + (2 T + 5) u J``.

The issue that asked for this module states the bound with the constant ``2 T + 6``; the derivation gives ``2 T + 5``, which
is the smaller, and that is what is asserted.  Measured with the statements alone (this file, CPU): the largest
``|out32 - out64| / bound`` over the runs of the scene is 0.63 to 0.82 (0.41 to 0.60 with ``J`` replaced by ``rel_jump d0``);
most of it is the last addition's half ulp of a depth near 600 against ``u |out|``.  On an MI355X the kernel equals the
float32 statement bit for bit in every case of this file (parity_report.jsonl, "depth_upsample_*": 0 differing pixels,
largest error / bound 0.08 to 0.88).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import report

U32 = 2.0 ** -24
DEFAULTS = dict(sigma_space=1.0, sigma_colour=12.0, rel_jump=0.02, depth_min=1e-3, depth_max=1e5)


# ---------------------------------------------------------------------------------------------------------------------
# the two statements
# ---------------------------------------------------------------------------------------------------------------------
def tables(s, radius, sigma_space, sigma_colour):
    """ws (s, 2 radius + 1) and wc (766,) of the docstring: float64 on the host, entries below 2^-24 zeroed, then float32."""
    ws = np.zeros((s, 2 * radius + 1))
    for p in range(s):
        for j in range(-radius, radius + 1):
            delta = j + 0.5 - (p + 0.5) / s
            ws[p, j + radius] = np.exp(-delta ** 2 / (2.0 * sigma_space ** 2))
    wc = np.exp(-(np.arange(766) / 3.0) ** 2 / (2.0 * sigma_colour ** 2))
    ws[ws < U32] = 0.0
    wc[wc < U32] = 0.0
    return ws.astype(np.float32), wc.astype(np.float32)


def statement(depth, guide, radius, anchor_radius, sigma_space=1.0, sigma_colour=12.0, rel_jump=0.02, depth_min=1e-3,
              depth_max=1e5):
    """One view: ``depth`` (h, w) float32, ``guide`` (s h, s w, 3) uint8 -> dict of out32, out64 (float64), count, J, d0."""
    depth = np.asarray(depth, np.float32)
    h, w = depth.shape
    H, W = guide.shape[:2]
    s = H // h if h else 1
    assert (H, W) == (s * h, s * w)
    ws, wc = tables(s, radius, sigma_space, sigma_colour)
    f32 = np.float32
    rel_jump, depth_min, depth_max = f32(rel_jump), f32(depth_min), f32(depth_max)     # the kernel's arguments are floats
    Y, X = np.mgrid[0:H, 0:W]
    cy, cx, py, px = Y // s, X // s, Y % s, X % s
    own = guide.astype(np.int64)

    def tap(tx, ty):
        qx, qy = cx + tx, cy + ty
        inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
        qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
        d = depth[qy, qx]
        a = np.abs(guide[qy * s + s // 2, qx * s + s // 2].astype(np.int64) - own).sum(-1)
        wsp = ws[py, ty + radius] * ws[px, tx + radius]                            # float32 product
        wt = wsp * wc[a]                                                           # float32 product
        wt64 = ws[py, ty + radius].astype(np.float64) * ws[px, tx + radius].astype(np.float64) * wc[a].astype(np.float64)
        with np.errstate(invalid="ignore"):
            valid = inside & (d > depth_min) & (d < depth_max)
        return d, valid, wt, wt64

    dc, centre_valid, w_best, _ = tap(0, 0)
    d0 = dc.copy()
    w_best = w_best.copy()
    for ty in range(-anchor_radius, anchor_radius + 1):
        for tx in range(-anchor_radius, anchor_radius + 1):
            d, valid, wt, _ = tap(tx, ty)
            better = valid & (wt > w_best)
            w_best = np.where(better, wt, w_best)
            d0 = np.where(better, d, d0)
    with np.errstate(invalid="ignore", over="ignore"):
        jump = rel_jump * d0                                                       # float32
    W32, S32 = np.zeros((H, W), f32), np.zeros((H, W), f32)
    W64, S64 = np.zeros((H, W)), np.zeros((H, W))
    count = np.zeros((H, W), np.int32)
    J = np.zeros((H, W))
    for ty in range(-radius, radius + 1):
        for tx in range(-radius, radius + 1):
            d, valid, wt, wt64 = tap(tx, ty)
            with np.errstate(invalid="ignore", over="ignore"):
                diff = d - d0                                                      # float32
                linked = valid & (np.abs(diff) <= jump)
                W32 = W32 + np.where(linked, wt, f32(0))
                S32 = S32 + np.where(linked, wt * diff, f32(0))
                W64 = W64 + np.where(linked, wt64, 0.0)
                S64 = S64 + np.where(linked, wt64 * diff.astype(np.float64), 0.0)
            count += linked
            J = np.maximum(J, np.where(linked, np.abs(diff.astype(np.float64)), 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        out32 = np.where(W32 > 0, d0 + S32 / W32, d0).astype(f32)
        out64 = np.where(W64 > 0, d0.astype(np.float64) + S64 / W64, d0.astype(np.float64))
    assert out32.dtype == f32 and W32.dtype == f32 and S32.dtype == f32
    hole = ~centre_valid
    return dict(out32=np.where(hole, f32(0), out32), out64=np.where(hole, 0.0, out64), count=np.where(hole, 0, count),
                J=np.where(hole, 0.0, J), d0=np.where(hole, f32(0), d0), hole=hole)


def bound(st, radius):
    """The module docstring's bound per pixel."""
    T = (2 * radius + 1) ** 2
    return U32 * np.abs(st["out64"]) + (2 * T + 5) * U32 * st["J"]


# ---------------------------------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------------------------------
def make_scene(s, h=48, w=64, seed=0):
    """A tilted background plane 600 + 1.5 u + 0.8 v (u, v in low-resolution pixels), a disc 60 units nearer (radius 14.2,
    centre (32.3, 24.4) on the 48 x 64 map, scaled with the map), depth noise of sigma 0.3, a 4 x 5 block of zeros; the
    guide has two flat colours about 400 apart in summed channel difference that switch at the disc's TRUE edge at full
    resolution, with +-6 of noise.  Returns depth (h, w) float32, guide (s h, s w, 3) uint8, the true depth (s h, s w)."""
    rng = np.random.default_rng(100 + seed)
    k = h / 48.0
    r, ux, vy = 14.2 * k, 32.3 * k, 24.4 * k

    def truth(u, v):
        d = 600.0 + 1.5 * u + 0.8 * v
        inside = (u - ux) ** 2 + (v - vy) ** 2 < r * r
        return np.where(inside, d - 60.0, d), inside

    v, u = np.mgrid[0:h, 0:w] + 0.5
    depth = truth(u, v)[0] + rng.normal(0.0, 0.3, (h, w))
    depth[5:9, 50:55] = 0.0
    V, U = (np.mgrid[0:h * s, 0:w * s] + 0.5) / s
    true_hi, inside = truth(U, V)
    colours = np.array([[60, 70, 80], [200, 190, 220]], np.int64)              # |d| = 140 + 120 + 140 = 400
    guide = colours[inside.astype(np.int64)] + rng.integers(-6, 7, (h * s, w * s, 3))
    return depth.astype(np.float32), np.clip(guide, 0, 255).astype(np.uint8), true_hi


@functools.lru_cache(maxsize=None)
def scene_run(s, radius, anchor_radius):
    depth, guide, truth = make_scene(s)
    return depth, guide, truth, statement(depth, guide, radius, anchor_radius, **DEFAULTS)


SCENE_RUNS = [(2, 2), (3, 2), (3, 1), (4, 2)]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the statements themselves, and the arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_module_tables_are_the_statements():
    from pointmvsnet_amd import refine
    for s, radius, sigma in ((1, 0, 1.0), (2, 2, 1.0), (3, 8, 0.7), (8, 8, 2.5)):
        ws, wc = tables(s, radius, sigma, 12.0)
        assert refine.spatial_table(s, radius, sigma).tobytes() == ws.tobytes()
        assert refine.colour_table(12.0).tobytes() == wc.tobytes()
    ws, wc = tables(3, 8, 0.7, 4.0)
    assert (ws == 0).any() and (wc == 0).any() and ws[ws > 0].min() >= U32 and wc[wc > 0].min() >= U32


def test_exact_cases_of_the_float32_statement():
    rng = np.random.default_rng(1)
    h, w, s = 9, 11, 3
    guide = rng.integers(0, 256, (h * s, w * s, 3), dtype=np.uint8)
    # a constant map returns the constant, bit for bit, wherever it is valid; 0 exactly where the containing pixel is not
    const = np.full((h, w), np.float32(612.3456), np.float32)
    const[2:4, 5:8] = 0.0
    const[7, 1] = np.float32(2e5)                                                 # beyond depth_max: not valid either
    st = statement(const, guide, 2, 1)
    hole = np.repeat(np.repeat((const == 0) | (const > 1e5), s, 0), s, 1)
    assert np.array_equal(st["hole"], hole) and np.array_equal(st["out32"] == 0, hole) and np.array_equal(st["count"] == 0, hole)
    assert np.all(st["out32"][~hole].view(np.uint32) == np.float32(612.3456).view(np.uint32))
    # s = 1, radius = 0 is the identity
    depth = (600 + rng.normal(0, 20, (h, w))).astype(np.float32)
    depth[0, 0] = 0.0
    st = statement(depth, guide[::s, ::s], 0, 0)
    assert st["out32"].tobytes() == depth.tobytes() and np.array_equal(st["count"], (depth != 0).astype(np.int32))
    # uniform colours: a depth step larger than rel_jump is not bridged
    step = np.full((h, w), np.float32(500.0), np.float32)
    step[:, 6:] = np.float32(500.0 * 1.05)
    step += rng.normal(0, 0.2, (h, w)).astype(np.float32)
    flat = np.full((h * s, w * s, 3), 128, np.uint8)
    st = statement(step, flat, 2, 1)
    left = np.zeros((h * s, w * s), bool)
    left[:, :6 * s] = True
    assert st["out32"][left].max() < 502 and st["out32"][~left].min() > 523       # the values stay on their own side
    # with one colour the containing pixel has the largest weight, so it is the anchor, and the count is that of its side:
    # all 25 taps away from the step, 20 and 15 in the two columns on either side of it
    low = st["count"][::s, ::s]
    assert np.array_equal(st["count"], np.repeat(np.repeat(low, s, 0), s, 1))
    assert np.all(low[2:7, [2, 3, 8]] == 25)
    assert np.all(low[2:7, 4] == 20) and np.all(low[2:7, 5] == 15) and np.all(low[2:7, 6] == 15) and np.all(low[2:7, 7] == 20)


def test_upsampled_intrinsics_map_pixel_centres_exactly():
    from pointmvsnet_amd import refine
    K = np.array([[361.5, 0.0, 81.25], [0.0, 360.75, 64.5], [0.0, 0.0, 1.0]])
    for s in (1, 2, 3, 4, 8):
        Ks = refine.upsampled_intrinsics(K, s)
        assert Ks.dtype == np.float64 and np.array_equal(Ks, np.diag([s, s, 1.0]) @ K)
        assert np.array_equal(refine.upsampled_intrinsics(np.stack([K, 2 * K]), s)[1], np.diag([s, s, 1.0]) @ (2 * K))
        # the ray through output pixel (X, Y)'s centre is the low-resolution ray through ((X + .5) / s, (Y + .5) / s)
        X, Y = np.meshgrid(np.arange(0, 12 * s, 5), np.arange(0, 10 * s, 3))
        hi = np.stack([X + 0.5, Y + 0.5, np.ones_like(X, float)], -1)
        lo = np.stack([(X + 0.5) / s, (Y + 0.5) / s, np.ones_like(X, float)], -1)
        assert np.allclose(hi @ np.linalg.inv(Ks).T, lo @ np.linalg.inv(K).T, rtol=1e-13, atol=1e-15)
        if s in (1, 2, 4, 8):                                                     # powers of two: not one bit is lost
            P = np.array([12.25, -7.5, 600.0])
            assert np.array_equal((Ks @ P)[:2], s * (K @ P)[:2])
    for bad in (0, 1.5, True):
        with pytest.raises(ValueError):
            refine.upsampled_intrinsics(K, bad)


def test_bad_arguments_raise_before_a_gpu_is_asked_for():
    from pointmvsnet_amd import refine, scan
    d = torch.zeros((2, 4, 6))
    g = torch.zeros((2, 8, 12, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):                         # sound arguments: only the GPU is missing
        refine.upsample_depth_maps(d, g)
    with pytest.raises(RuntimeError, match="no CPU path"):
        refine.upsample_depth_maps([d[0], d[1]], g, radius=8, anchor_radius=2, rel_jump=0.5)
    for guides in (torch.zeros((2, 8, 13, 3), dtype=torch.uint8), torch.zeros((2, 8, 18, 3), dtype=torch.uint8),
                   torch.zeros((2, 9, 12, 3), dtype=torch.uint8), torch.zeros((2, 36, 54, 3), dtype=torch.uint8),
                   torch.zeros((2, 2, 3, 3), dtype=torch.uint8), torch.zeros((3, 8, 12, 3), dtype=torch.uint8),
                   torch.zeros((2, 8, 12, 4), dtype=torch.uint8), torch.zeros((2, 8, 12), dtype=torch.uint8),
                   torch.zeros((2, 8, 12, 3), dtype=torch.float32)):
        with pytest.raises(ValueError):
            refine.upsample_depth_maps(d, guides)
    for depths in (d.double(), d.to(torch.int32), d[0], [d[0], d[1, :3]]):
        with pytest.raises(ValueError):
            refine.upsample_depth_maps(depths, g)
    for kw in (dict(radius=9), dict(radius=-1), dict(radius=1.5), dict(radius=1, anchor_radius=2), dict(radius=8, anchor_radius=3),
               dict(anchor_radius=-1), dict(rel_jump=-0.01), dict(rel_jump=0.51), dict(rel_jump=float("nan")),
               dict(sigma_space=0.0), dict(sigma_colour=0.0), dict(sigma_space=-1.0), dict(sigma_colour=float("nan"))):
        with pytest.raises(ValueError):
            refine.upsample_depth_maps(d, g, **kw)
    # the accumulator's two refusals need neither views nor a GPU
    with pytest.raises(TypeError):
        scan.ScanAccumulator(2, keep_guides=True).fuse(upsample=[("radius", 2)])
    with pytest.raises(ValueError, match="keep_guides"):
        scan.ScanAccumulator(2).fuse(upsample={})
    with pytest.raises(ValueError, match="have not been added"):
        scan.ScanAccumulator(2, keep_guides=True).upsampled()


@pytest.mark.parametrize("anchor_radius", [0, 1])
@pytest.mark.parametrize("s,radius", SCENE_RUNS)
def test_statement_pair_agrees_within_the_derived_bound(s, radius, anchor_radius):
    """Holes and counts are one computation's decisions, shared; the values agree within the module docstring's bound."""
    depth, guide, _, st = scene_run(s, radius, anchor_radius)
    hole = np.repeat(np.repeat(~((depth > 1e-3) & (depth < 1e5)), s, 0), s, 1)
    assert np.array_equal(st["out32"] == 0, hole) and np.array_equal(st["out64"] == 0, hole)
    assert np.array_equal(st["count"] == 0, hole) and st["count"].max() <= (2 * radius + 1) ** 2
    err = np.abs(st["out32"].astype(np.float64) - st["out64"])
    ratio = float((err[~hole] / bound(st, radius)[~hole]).max())
    loose = float((err[~hole] / (U32 * np.abs(st["out64"]) + (2 * (2 * radius + 1) ** 2 + 5) * U32 * 0.02 * st["d0"])[~hole]).max())
    print("s", s, "radius", radius, "anchor", anchor_radius, "error / bound", ratio, "with J = rel_jump d0", loose)
    assert np.all(err <= bound(st, radius))
    assert np.all(st["J"] <= 0.02 * st["d0"].astype(np.float64) * (1 + 2 * U32))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_the_anchor_moves_the_depth_edge_to_the_guides(s):
    """Against nearest replication, over the valid pixels: fewer than half as many pixels more than 5 units from the true
    full-resolution depth, and a smaller RMS error.  Without the anchor the edge stays where replication puts it."""
    depth, guide, truth, st = scene_run(s, 2, 1)
    nearest = np.repeat(np.repeat(depth, s, 0), s, 1)
    ok = ~st["hole"]
    far_nearest = int((np.abs(nearest - truth) > 5)[ok].sum())
    far = int((np.abs(st["out32"] - truth) > 5)[ok].sum())
    far_no_anchor = int((np.abs(scene_run(s, 2, 0)[3]["out32"] - truth) > 5)[ok].sum())
    rms = float(np.sqrt(np.mean((st["out32"] - truth)[ok] ** 2)))
    rms_nearest = float(np.sqrt(np.mean((nearest - truth)[ok] ** 2)))
    print("s", s, "far", far, "nearest", far_nearest, "no anchor", far_no_anchor, "rms", rms, "nearest", rms_nearest)
    assert far_nearest > 0 and 2 * far < far_nearest
    assert far_no_anchor == far_nearest
    assert rms < rms_nearest


def test_scale_one_smooths_the_map():
    depth, guide, truth = make_scene(1)
    st = statement(depth, guide, 2, 1, **DEFAULTS)
    ok = ~st["hole"]
    rms = float(np.sqrt(np.mean((st["out32"] - truth)[ok] ** 2)))
    rms_nearest = float(np.sqrt(np.mean((depth - truth)[ok] ** 2)))
    print("s 1 rms", rms, "the map's own", rms_nearest)
    assert rms < rms_nearest


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
GPU_CASES = [(2, 2, 1), (3, 1, 1), (4, 2, 0), (1, 3, 2), (8, 8, 2)]


@functools.lru_cache(maxsize=None)
def gpu_case(s):
    """Three views of the scene at 24 x 32 low resolution."""
    scenes = [make_scene(s, 24, 32, seed=v) for v in range(3)]
    return np.stack([d for d, _, _ in scenes]), np.stack([g for _, g, _ in scenes])


def _run(dev, depths, guides, **kw):
    from pointmvsnet_amd import refine
    out = refine.upsample_depth_maps(torch.from_numpy(depths).to(dev), torch.from_numpy(guides).to(dev), **kw)
    if isinstance(out, tuple):
        return tuple(t.cpu().numpy() for t in out)
    return out.cpu().numpy()


def _statements(depths, guides, radius, anchor_radius, **kw):
    sts = [statement(d, g, radius, anchor_radius, **kw) for d, g in zip(depths, guides)]
    return {k: np.stack([st[k] for st in sts]) for k in sts[0]}


@pytest.mark.gpu
@pytest.mark.parametrize("s,radius,anchor_radius", GPU_CASES)
def test_kernel_matches_the_statements(dev, s, radius, anchor_radius):
    """Holes and counts equal to the statement's on every pixel; values within the derived bound of the float64 statement,
    and equal to the float32 statement bit for bit."""
    depths, guides = gpu_case(s)
    st = _statements(depths, guides, radius, anchor_radius, **DEFAULTS)
    out, count = _run(dev, depths, guides, radius=radius, anchor_radius=anchor_radius, return_count=True, **DEFAULTS)
    assert out.dtype == np.float32 and count.dtype == np.int32 and out.shape == count.shape == st["out32"].shape
    assert np.array_equal(out == 0, st["hole"]) and np.array_equal(count, st["count"])
    b = np.stack([bound({k: st[k][v] for k in st}, radius) for v in range(len(depths))])
    err = np.abs(out.astype(np.float64) - st["out64"])
    ok = ~st["hole"]
    ratio = float((err[ok] / b[ok]).max())
    differing = int((out.view(np.uint32) != st["out32"].view(np.uint32)).sum())
    print("s", s, "radius", radius, "anchor", anchor_radius, "largest error / bound", ratio, "pixels off the float32 statement",
          differing)
    report("depth_upsample_s%d_r%d_a%d" % (s, radius, anchor_radius), ratio=ratio, differing=differing)
    assert np.all(err <= b)
    assert differing == 0


EDGE_SHAPES = [((1, 20), 2, 2), ((20, 1), 2, 2), ((8, 8), 2, 2), ((9, 13), 2, 2), ((6, 5), 3, 2), ((5, 5), 2, 8),
               ((5, 5), 1, 8), ((17, 33), 1, 2), ((7, 6), 5, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,s,radius", EDGE_SHAPES)
def test_edge_shapes(dev, shape, s, radius):
    """Maps of one row, one column, exactly one tile, ragged tiles, a halo larger than the map."""
    h, w = shape
    rng = np.random.default_rng(h * 100 + w)
    depths = (600 + rng.normal(0, 3, (2, h, w))).astype(np.float32)
    depths[rng.random((2, h, w)) < 0.1] = 0.0
    depths[1].flat[::7] *= np.float32(1.1)
    guides = (rng.integers(0, 2, (2, h * s, w * s, 1)) * 90 + rng.integers(0, 30, (2, h * s, w * s, 3))).astype(np.uint8)
    anchor = min(radius, 2)
    st = _statements(depths, guides, radius, anchor, **DEFAULTS)
    out, count = _run(dev, depths, guides, radius=radius, anchor_radius=anchor, return_count=True, **DEFAULTS)
    assert np.array_equal(count, st["count"]) and out.tobytes() == st["out32"].tobytes()


@pytest.mark.gpu
def test_empty_maps(dev):
    zeros = np.zeros((2, 9, 13), np.float32)
    guides = np.random.default_rng(0).integers(0, 256, (2, 18, 26, 3), dtype=np.uint8)
    out, count = _run(dev, zeros, guides, return_count=True)
    assert out.shape == (2, 18, 26) and not out.any() and not count.any()
    out, count = _run(dev, np.zeros((2, 0, 13), np.float32), np.zeros((2, 0, 26, 3), np.uint8), return_count=True)
    assert out.shape == (2, 0, 26) and count.shape == (2, 0, 26) and out.dtype == np.float32 and count.dtype == np.int32
    assert _run(dev, np.zeros((1, 4, 0), np.float32), np.zeros((1, 4, 0, 3), np.uint8)).shape == (1, 4, 0)


@pytest.mark.gpu
def test_reproducible_and_independent_of_the_view_order(dev):
    depths, guides = gpu_case(3)
    kw = dict(radius=2, anchor_radius=1)
    out, count = _run(dev, depths, guides, return_count=True, **kw)
    again, count2 = _run(dev, depths, guides, return_count=True, **kw)
    assert out.tobytes() == again.tobytes() and count.tobytes() == count2.tobytes()
    order = [2, 0, 1]
    permuted = _run(dev, depths[order], guides[order], **kw)
    assert permuted.tobytes() == out[order].tobytes()                # and the arm without the count map gives the same depths
    assert _run(dev, depths, guides, **kw).tobytes() == out.tobytes()
    sequence = _run(dev, depths, guides, **kw)
    from pointmvsnet_amd import refine
    stacked = refine.upsample_depth_maps([torch.from_numpy(d).to(dev) for d in depths], torch.from_numpy(guides).to(dev), **kw)
    assert stacked.cpu().numpy().tobytes() == sequence.tobytes()


def _accumulator(dev, depths, cams, refs, **kw):
    from pointmvsnet_amd import scan
    V, h, w = depths.shape
    acc = scan.ScanAccumulator(V, mode="NEAREST", **kw)
    for v in range(V):
        preds = {"flow2": torch.from_numpy(depths[v])[None, None].to(dev), "flow2_prob": torch.full((1, 5, h, w), 0.2).to(dev),
                 "coarse_prob_map": torch.ones(1, 1, h, w).to(dev)}
        cam = cams[v:v + 1][None].clone()
        cam[0, 0, 1, :2, :3] *= refs.shape[1] / float(h)                           # the cameras of the full image
        batch = {"cam_params_list": cam.to(dev), "cam_params_list_host": cam, "img_list": torch.zeros(1, 1, 3, h, w),
                 "ref_img": torch.from_numpy(refs[v:v + 1, :, :, ::-1].copy())}   # BGR, as the loader hands it
        acc.add(batch, preds, view_index=v)
    return acc


@pytest.mark.gpu
def test_through_the_scan_accumulator(dev):
    """Five views of test_fusion's plane scene as predictions, the ``ref_img`` at twice the map's size."""
    from test_fusion import make_plane_scene
    from pointmvsnet_amd import fusion, geometric, refine
    depths, K, E, images, cams = make_plane_scene(5, sigma=0.3)
    V, h, w = depths.shape
    rng = np.random.default_rng(3)
    smooth = rng.integers(0, 256, (V, h // 8, w // 8, 3)).repeat(16, 1).repeat(16, 2)
    refs = np.clip(smooth + rng.integers(-5, 6, smooth.shape), 0, 255).astype(np.uint8)      # (V, 2 h, 2 w, 3) RGB
    acc = _accumulator(dev, depths, cams, refs, keep_guides=True)
    plain = _accumulator(dev, depths, cams, refs)
    assert plain.guides() is None and torch.equal(acc.guides().cpu(), torch.from_numpy(refs))
    settings = {"radius": 2, "anchor_radius": 1, "rel_jump": 0.01}
    fuse = {"num_consistent": 2}
    d_hi, K_hi, E_hi, guides = acc.upsampled(**settings)
    K_lo, E_lo = acc.cameras()
    assert np.array_equal(K_hi, refine.upsampled_intrinsics(K_lo, 2)) and np.array_equal(E_hi, E_lo) and guides is acc.guides()
    assert np.allclose(K_lo, K, rtol=1e-12)
    want_hi = refine.upsample_depth_maps(acc.filtered(), guides, **settings)
    assert d_hi.shape == (V, 2 * h, 2 * w) and torch.equal(d_hi, want_hi)
    # both methods: the fusers on the upsampled maps, with the guides as the images
    pts, col = acc.fuse(upsample=settings, **fuse)
    want = fusion.fuse_depth_maps(want_hi, K_hi, E_lo, images=guides, **fuse)
    assert pts.shape[0] > 0 and torch.equal(pts, want[0]) and torch.equal(col, want[1])
    pts_r, col_r, nrm_r = acc.fuse(upsample=settings, method="roundtrip", with_normals=True, **fuse)
    want = geometric.geometric_filter(want_hi, K_hi, E_lo, images=guides, with_normals=True, depth_min=1e-3, depth_max=1e5,
                                      **fuse)[3:6]
    assert pts_r.shape[0] > 0 and torch.equal(pts_r, want[0]) and torch.equal(col_r, want[1]) and torch.equal(nrm_r, want[2])
    # without `upsample` nothing changes: the bytes of an accumulator that keeps no guides
    low = plain.fuse(**fuse)
    assert all(torch.equal(a, b) for a, b in zip(acc.fuse(**fuse), low)) and low[0].shape[0] > 0
    assert all(torch.equal(a, b) for a, b in zip(acc.fuse(method="roundtrip", **fuse), plain.fuse(method="roundtrip", **fuse)))
    print("points", int(low[0].shape[0]), "upsampled", int(pts.shape[0]), "roundtrip upsampled", int(pts_r.shape[0]))
    report("upsample_accumulator", points_low=int(low[0].shape[0]), points_high=int(pts.shape[0]))
    with pytest.raises(ValueError, match="keep_guides"):
        plain.fuse(upsample=settings)
    with pytest.raises(TypeError):
        acc.fuse(upsample="radius=2")
    with pytest.raises(ValueError):
        plain.upsampled()
    odd = _accumulator(dev, depths[:, :, :-1].copy(), cams, refs, keep_guides=True)       # 2 w is no multiple of w - 1
    with pytest.raises(ValueError):
        odd.upsampled()
