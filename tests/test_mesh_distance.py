"""Exact point-to-mesh distances and the scores built on them (pointmvsnet_amd/mesh_distance.py, csrc/mesh_distance.hip)
against a NumPy float64 statement written from the module's docstring: a brute-force minimum over all faces that shares no
code with the product.  Meshes come from the CPU statements of tests/test_tsdf.py (the sphere volumes, the plane scene) and
from a few lines of NumPy.

The bound
---------
U = 2^-53, the unit roundoff of float64.  Statement and kernel perform the same float64 additions, subtractions and
products in the same order (the library is built without contraction), so every quantity that involves no division and no
square root has the same bits on both sides: the edge vectors, ``ee``, ``w.e``, ``n``, ``nn``, the three inside tests and
``h = (p - a).n``.  They can differ only through the device's division and square root, each taken to be within one ulp
(2 U relative) of the correctly rounded host result.  With L the largest distance from the query to the face's vertices
(``|w| <= L``, ``|e| <= 2 L``, ``|r| <= L``):

* ``seg``: ``t`` differs by at most 2 U (it is clamped to [0, 1]).  Per component ``r = w - t e`` then differs by
  ``2 U |e|`` from ``t``, ``U |t e|`` from the product's rounding and ``U |r|`` from the difference's: at most ``7 U L``.
  ``r.r`` differs by ``2 sum |r_i| |dr_i| <= 2 sqrt(3) L * 7 U L < 25 U L^2`` plus its own roundings (three products, two
  sums: ``< 3 U L^2``): at most ``28 U L^2``.
* the plane: ``h h`` and ``nn`` are the same bits, so ``d2_plane`` differs by the one division: ``2 U d2 <= 2 U L^2``.
* the minimum of values that each differ by at most ``B`` differs by at most ``B``.

``B(L) = 32 U L^2`` is used (C = 32).  For the minimum over the faces, ``d2*_gpu <= d2_gpu(f*_stmt) <= d2*_stmt + B`` and the
other way round with the kernel's face, so L is taken over both faces.  Through the square root ``|sqrt x - sqrt y| <=
min(sqrt |x - y|, |x - y| / sqrt y)``: for an on-surface query that is ``sqrt(B)``.  The device's ``sqrt`` adds ``2 U d`` and
the two float32 roundings one float32 ulp, ``2^-23 d`` (plus the smallest float32 denormal)::

    tol(d, L) = min(sqrt(B), B / d) + 4 U d + 2^-23 d + 2^-149,    B = 32 * 2^-53 * L^2

The returned face must attain the statement's minimum within the same B: ``d2_stmt(p, face) <= d2*_stmt + B``.  The cap set
equals the statement's except where ``|d_stmt - max_dist| <= tol``; the statement alone keeps that band below 0.1 % of the
queries (asserted).  On the spheres additionally ``|d - | |p - centre| - r| | <= L^2 / (8 (r - L))``, ``L = sqrt(3)`` voxels, the
chord sag ``check_sphere_mesh`` uses.

Purity is asserted bit for bit.  ``conftest.report`` carries the figures as ``mesh_distance``.

Measured on an MI355X: of the 3 x 4 096 + 2 600 queries none differs from the statement in distance or face (the bound is
not used up), no query lies in the cap band, the spheres' distances are at most 0.77 (r = 8.3) and 0.62 (r = 5) of the sag;
the budget mesh exceeds its 107 040 pairs at edge 0.5 (247 406, counted with the per-face clamp), ends at edge 4 after three
widenings with 39 254, and hands 401 of 2 600 queries to the second pass.
"""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, report
from test_mesh_ops import plane_mesh
from test_tsdf import SPHERES, check_sphere_mesh, sphere_volume, statement_extract
from pointmvsnet_amd.utils import io as IO

U = 2.0 ** -53
C_BOUND = 32.0
N_QUERIES = 4096

DYADIC_TRIANGLE = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
DYADIC_QUERIES = np.array([[1, 1, 3], [-3, -4, 0], [2, -2, 0], [3, 3, 0], [7, 0, 4], [0, 8, -3], [-1, 2, 0], [4, 4, 0]], np.float32)
DYADIC_D2 = np.array([9, 25, 4, 2, 25, 25, 1, 8], np.float64)
# the same queries against the segment (0,0,0)-(4,0,0), which the face (a, b, b) is
SEGMENT_D2 = np.array([10, 25, 4, 9, 25, 73, 5, 16], np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _seg(p, u, v):
    e, w = v - u, p - u
    ee = np.broadcast_to(_dot(e, e), w.shape[:-1])
    we = _dot(w, e)
    with np.errstate(all="ignore"):
        t = np.where(ee > 0, np.clip(we / np.where(ee > 0, ee, 1.0), 0.0, 1.0), 0.0)
    r = w - t[..., None] * e
    return _dot(r, r)


def statement_d2(points, a, b, c):
    """(Q, F) float64 squared distances of the docstring: points (Q, 3), a, b, c (F, 3), float32 values."""
    p = np.asarray(points, np.float32).astype(np.float64)[:, None, :]
    a, b, c = (np.asarray(x, np.float32).astype(np.float64)[None, :, :] for x in (a, b, c))
    d2 = np.minimum(np.minimum(_seg(p, a, b), _seg(p, b, c)), _seg(p, c, a))
    n = _cross(b - a, c - a)
    nn = _dot(n, n)
    inside = (nn > 0) & (_dot(_cross(b - a, p - a), n) >= 0) & (_dot(_cross(c - b, p - b), n) >= 0) & \
        (_dot(_cross(a - c, p - c), n) >= 0)
    h = _dot(p - a, n)
    with np.errstate(all="ignore"):
        plane = (h * h) / np.where(nn > 0, nn, 1.0)
    return np.where(inside, np.minimum(plane, d2), d2)


def statement_distances(points, vertices, faces, max_dist, chunk=256):
    """``(dist float32, face int64, d2* float64)`` by brute force; faces with a non-finite vertex are skipped."""
    vertices = np.asarray(vertices, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    points = np.asarray(points, np.float32)
    keep = np.flatnonzero(np.isfinite(vertices[faces]).all(axis=(1, 2))) if len(faces) else np.zeros((0,), np.int64)
    best = np.full(len(points), np.inf)
    arg = np.full(len(points), -1, np.int64)
    if len(keep):
        a, b, c = (vertices[faces[keep, k]] for k in range(3))
        for s in range(0, len(points), chunk):
            d2 = statement_d2(points[s:s + chunk], a, b, c)
            j = np.argmin(d2, axis=1)                                      # the first minimum: the smallest face index
            best[s:s + chunk] = d2[np.arange(len(j)), j]
            arg[s:s + chunk] = keep[j]
    cap = np.float32(max_dist)
    with np.errstate(all="ignore"):
        d = np.sqrt(best).astype(np.float32)
    capped = ~(d < cap)
    return np.where(capped, cap, d).astype(np.float32), np.where(capped, -1, arg), best


def face_d2(points, vertices, faces, index):
    """The statement's d2 of query i against face index[i] (inf where the index is -1)."""
    vertices, faces = np.asarray(vertices, np.float32), np.asarray(faces, np.int64)
    out = np.full(len(points), np.inf)
    ok = np.flatnonzero(index >= 0)
    for s in range(0, len(ok), 512):
        i = ok[s:s + 512]
        f = faces[index[i]]
        d2 = statement_d2(points[i], vertices[f[:, 0]], vertices[f[:, 1]], vertices[f[:, 2]])
        out[i] = d2[np.arange(len(i)), np.arange(len(i))]
    return out


def reach(points, vertices, faces, index):
    """L: the largest distance from query i to the vertices of face index[i] (0 where the index is -1)."""
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)[np.maximum(index, 0)]]
    L = np.sqrt(((v - np.asarray(points, np.float64)[:, None, :]) ** 2).sum(-1)).max(axis=1)
    return np.where(index >= 0, L, 0.0)


def tolerance(d, L):
    B = C_BOUND * U * L * L
    d = np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        root = np.minimum(np.sqrt(B), np.where(d > 0, B / np.where(d > 0, d, 1.0), np.inf))
    return root + 4 * U * d + 2.0 ** -23 * d + 2.0 ** -149, B


def check_against_statement(points, vertices, faces, max_dist, got_d, got_f, want):
    """The conditions of the module docstring; returns the figures for the report."""
    want_d, want_f, want_d2 = want
    points = np.asarray(points, np.float32)
    d64 = np.sqrt(want_d2)
    cap = float(np.float32(max_dist))
    # L over the kernel's face and the statement's (where the statement is capped, its argmin before the cap)
    unc = statement_unclamped_face(points, vertices, faces, want_d2, want_f)
    L = np.maximum(reach(points, vertices, faces, got_f), reach(points, vertices, faces, unc))
    tol, B = tolerance(d64, L)
    band = np.abs(d64 - cap) <= tol
    assert band.mean() < 1e-3, band.mean()
    got_cap, want_cap = got_f < 0, want_f < 0
    assert ((got_d == np.float32(cap)) == got_cap).all()
    assert (got_cap == want_cap)[~band].all(), np.flatnonzero((got_cap != want_cap) & ~band)[:10]
    live = ~got_cap & ~want_cap
    err = np.abs(got_d.astype(np.float64) - want_d.astype(np.float64))
    assert (err[live] <= tol[live]).all(), (err[live] / tol[live]).max()
    own = face_d2(points, vertices, faces, got_f)
    assert (own[live] <= want_d2[live] + B[live]).all()
    return {"queries": len(points), "capped": int(got_cap.sum()), "band": int(band.sum()),
            "differing": int((got_d != want_d).sum()), "other_face": int((got_f != want_f).sum()),
            "worst_err_over_tol": float((err[live] / tol[live]).max()) if live.any() else 0.0}


def statement_unclamped_face(points, vertices, faces, want_d2, want_f):
    """The statement's argmin also where its result is capped (-1 only where no face has a surface)."""
    out = want_f.copy()
    miss = np.flatnonzero((want_f < 0) & np.isfinite(want_d2))
    if len(miss):
        out[miss] = statement_distances(points[miss], vertices, faces, np.float32(3e38))[1]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the meshes and the queries
# ---------------------------------------------------------------------------------------------------------------------
def sphere_mesh(name):
    n, centre, r = SPHERES[name]
    f, wgt = sphere_volume(n, centre, r)
    _, faces, vertices, _, _ = statement_extract(f, wgt, (0.0, 0.0, 0.0), 1.0)
    return vertices.astype(np.float32), faces.astype(np.int64)


def make_queries(vertices, faces, seed, n=N_QUERIES):
    """``(points (n, 3) float32, max_dist)``: a third within 0.01 of the surface, a third within a tenth of the mesh's
    diagonal (a few units), a third beyond ``max_dist`` = a quarter of the diagonal from every point of the mesh's box."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, np.float64)
    v = v[np.isfinite(v).all(axis=1)]
    lo, hi = v.min(axis=0), v.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    max_dist = float(np.float32(0.25 * diag))
    tri = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    tri = tri[np.isfinite(tri).all(axis=(1, 2))]

    def on_surface(m):
        t = tri[rng.integers(0, len(tri), m)]
        w = rng.dirichlet(np.ones(3), m)
        return (t * w[:, :, None]).sum(axis=1)

    def offset(m, length):
        d = rng.normal(size=(m, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True) * (rng.random((m, 1)) * length)

    third = n // 3
    near = on_surface(third) + offset(third, 0.01)
    near[: third // 8] = on_surface(third // 8)                                # and some as close as float32 puts them
    mid = on_surface(third) + offset(third, 0.1 * diag)
    far_n = n - 2 * third
    d = rng.normal(size=(far_n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = (lo + hi) / 2.0 + d * (0.5 * diag + max_dist * (1.1 + rng.random((far_n, 1))))
    points = np.concatenate([near, mid, far]).astype(np.float32)
    return points[rng.permutation(n)], max_dist


def budget_mesh():
    """Two triangles spanning a 600 x 450 plane at z = 0 and the small sphere mesh moved above it: vertices, faces, and
    queries of which some are 15 above the plane, away from the sphere."""
    sv, sf = sphere_mesh("on_sample_17")
    sv = sv + np.array([300.0, 200.0, 30.0], np.float32)
    plane = np.array([[0, 0, 0], [600, 0, 0], [600, 450, 0], [0, 450, 0]], np.float32)
    vertices = np.concatenate([plane, sv]).astype(np.float32)
    faces = np.concatenate([[[0, 1, 2], [0, 2, 3]], sf + 4]).astype(np.int64)
    rng = np.random.default_rng(11)
    over = np.stack([rng.uniform(-10, 610, 1500), rng.uniform(-10, 460, 1500), rng.uniform(-6, 6, 1500)], axis=1)
    high = np.stack([rng.uniform(0, 250, 300), rng.uniform(0, 450, 300), rng.uniform(13, 19, 300)], axis=1)
    ball = np.array([308.0, 208.0, 38.0]) + rng.normal(size=(700, 3)) * 4.0
    away = np.stack([rng.uniform(0, 600, 100), rng.uniform(0, 450, 100), rng.uniform(60, 90, 100)], axis=1)
    return vertices, faces, np.concatenate([over, high, ball, away]).astype(np.float32)


@pytest.fixture(scope="module")
def cases():
    """Per mesh: vertices, faces, queries, max_dist and the statement's answer, computed once."""
    out = {}
    for seed, (name, (v, f)) in enumerate([("sphere24", sphere_mesh("off_lattice_24")), ("sphere17", sphere_mesh("on_sample_17")),
                                           ("plane", plane_mesh()[:2])]):
        assert 1000 < len(f) < 20000, (name, len(f))
        q, max_dist = make_queries(v, f, seed)
        out[name] = (v, f, q, max_dist, statement_distances(q, v, f, max_dist))
    v, f, q = budget_mesh()
    out["budget"] = (v, f, q, 20.0, statement_distances(q, v, f, 20.0))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused_before_a_device_is_needed():
    from pointmvsnet_amd import mesh_distance as D
    p = torch.zeros((5, 3))
    v = torch.zeros((4, 3))
    f = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    calls = (lambda p, v, f, **kw: D.point_mesh_distances(p, v, f, **kw), lambda p, v, f, **kw: D.evaluate_mesh(v, f, p, **kw),
             lambda p, v, f, **kw: D.evaluate_point_cloud_on_mesh(p, v, f, **kw))
    for call in calls:
        for bad in (p.double(), p[:, :2], p[0]):
            with pytest.raises(ValueError, match="points must be"):
                call(bad, v, f)
        with pytest.raises(TypeError):
            call(None, v, f)
        nan = p.clone()
        nan[2, 1] = float("nan")
        with pytest.raises(ValueError, match="non-finite"):
            call(nan, v, f)
        for bad in (v.double(), v[:, :2], v[0], None):
            with pytest.raises(ValueError, match="vertices must be"):
                call(p, bad, f)
        for bad in (f.float(), f[:, :2], f[0], None, f.to(torch.int16)):
            with pytest.raises(ValueError, match="faces must be"):
                call(p, v, bad)
        for bad in (0.0, -1.0, float("nan"), float("inf"), "x", None):
            with pytest.raises(ValueError, match="max_dist"):
                call(p, v, f, max_dist=bad)
        with pytest.raises(RuntimeError, match="no CPU path"):                 # well-formed: only the device is missing
            call(p, v, f)
    with pytest.raises(ValueError, match="obs_mask needs"):
        D.evaluate_mesh(v, f, p, obs_mask=torch.ones((2, 2, 2)))
    with pytest.raises(ValueError, match="obs_mask needs"):
        D.evaluate_point_cloud_on_mesh(p, v, f, obs_mask=torch.ones((2, 2, 2)))
    assert D.pair_budget(1000) == 16 * 1000 + 2 ** 16 and D.pair_budget(D.MAX_FACES) < 2 ** 31
    assert isinstance(D.last_grid_report(), dict)


def test_kernels_are_built_and_bound(lib_built):
    from pointmvsnet_amd import _lib, build
    names = {"pf_mesh_dist_count_f32", "pf_mesh_dist_emit_f32", "pf_mesh_dist_pack_f32", "pf_mesh_dist_cells_f64",
             "pf_mesh_dist_wave_f64"}
    assert "mesh_distance.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "pointflow_hip.h")).read()
    exported = set(re.findall(r" T (pf_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", lib_built]).decode()))
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header) and name in exported and name in _lib.PROTOTYPES, name
    assert {n for n in exported if n.startswith("pf_mesh_dist_")} == names
    lib = _lib.load()
    # pointers and counts are required before anything is launched
    assert lib.pf_mesh_dist_count_f32(None, 3, None, 1, 0, 0, 0, 1.0, 2, 2, 2, 10, None, None) == -1
    assert lib.pf_mesh_dist_count_f32(None, 3, None, 0, 0, 0, 0, 1.0, 2, 2, 2, 10, None, None) == 0
    assert lib.pf_mesh_dist_count_f32(None, 3, None, 1, 0, 0, 0, 0.0, 2, 2, 2, 10, None, None) == -1
    assert lib.pf_mesh_dist_emit_f32(None, 3, None, 1, 0, 0, 0, 1.0, 2, 2, 2, None, 5, None, None, None) == -1
    assert lib.pf_mesh_dist_emit_f32(None, 3, None, 1, 0, 0, 0, 1.0, 2, 2, 2, None, 2 ** 31, None, None, None) == -1
    assert lib.pf_mesh_dist_pack_f32(None, 3, None, 1, None, None, 5, None, None) == -1
    assert lib.pf_mesh_dist_cells_f64(None, 5, None, None, 5, 0, 0, 0, 1.0, 2, 2, 2, 3, 20.0, None, None, None, None) == -1
    assert lib.pf_mesh_dist_cells_f64(None, 5, None, None, 0, 0, 0, 0, 1.0, 2, 2, 2, 3, 20.0, None, None, None, None) == -1
    assert lib.pf_mesh_dist_wave_f64(None, None, 5, 5, None, None, 5, 0, 0, 0, 30.0, 2, 2, 2, 20.0, None, None, None) == -1
    assert lib.pf_mesh_dist_wave_f64(None, None, 0, 5, None, None, 5, 0, 0, 0, 10.0, 2, 2, 2, 20.0, None, None, None) == -1


def test_statement_gives_the_dyadic_cases_exactly():
    a, b, c = DYADIC_TRIANGLE[None, 0], DYADIC_TRIANGLE[None, 1], DYADIC_TRIANGLE[None, 2]
    assert np.array_equal(statement_d2(DYADIC_QUERIES, a, b, c)[:, 0], DYADIC_D2)
    assert np.array_equal(statement_d2(DYADIC_QUERIES, a, b, b)[:, 0], SEGMENT_D2)
    assert np.array_equal(statement_d2(DYADIC_QUERIES, b, b, b)[:, 0], ((DYADIC_QUERIES - DYADIC_TRIANGLE[1]) ** 2).sum(1))
    d, f, d2 = statement_distances(DYADIC_QUERIES, DYADIC_TRIANGLE, [[0, 1, 2]] * 3, 4.5)
    assert f.tolist() == [0, -1, 0, 0, -1, -1, 0, 0] and np.array_equal(d2, DYADIC_D2)
    assert np.array_equal(d, np.where(f < 0, np.float32(4.5), np.sqrt(DYADIC_D2).astype(np.float32)))


def test_statement_against_dense_sampling_of_the_triangles():
    """On random triangles, slivers and degenerate faces among them, the statement's distance is <= the minimum over a
    201 x 201 barycentric lattice of the triangle and >= that minimum minus the lattice spacing.  The lattice is the
    yardstick here and has a rounding of its own: a lattice point ``a + wi (b - a) + wj (c - a)`` and its difference from
    the query carry a few U of the coordinates' magnitude M (where the nearest point is the vertex b the statement forms
    ``(p - a) - 1 (b - a)`` and the lattice ``p - (a + 1 (b - a))``), so both comparisons allow ``16 U M``."""
    rng = np.random.default_rng(7)
    T, Q, n = 60, 80, 200
    tri = rng.normal(size=(T, 3, 3)) * 3.0
    tri[10:20, 2] = tri[10:20, 0] + (tri[10:20, 1] - tri[10:20, 0]) * rng.random((10, 1)) + rng.normal(size=(10, 3)) * 1e-6
    tri[20:25, 2] = tri[20:25, 1]                                            # (a, b, b)
    tri[25:28, 1] = tri[25:28, 0]
    tri[25:28, 2] = tri[25:28, 0]                                            # a point
    tri[28:32, 2] = (tri[28:32, 0] + tri[28:32, 1]) / 2                      # collinear
    tri = tri.astype(np.float32)
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    ok = (i + j) <= n
    wi, wj = (i[ok] / float(n))[:, None], (j[ok] / float(n))[:, None]
    worst = 0.0
    for t in range(T):
        a, b, c = tri[t].astype(np.float64)
        q = (tri[t].astype(np.float64)[rng.integers(0, 3, Q)] + rng.normal(size=(Q, 3)) * rng.choice([0.01, 1.0, 10.0], (Q, 1)))
        q = q.astype(np.float32)
        lattice = a + wi * (b - a) + wj * (c - a)
        diff = q.astype(np.float64)[:, None, :] - lattice[None, :, :]
        dense = np.sqrt(_dot(diff, diff).min(axis=1))
        d = np.sqrt(statement_d2(q, tri[t, 0][None], tri[t, 1][None], tri[t, 2][None])[:, 0])
        spacing = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b)) / n
        own = 16 * U * max(np.abs(tri[t]).max(), np.abs(q).max())
        assert (d <= dense + own).all(), (t, (d - dense).max())
        assert (d >= dense - spacing - own).all(), (t, (dense - spacing - d).max())
        worst = max(worst, float((dense - d).max() / max(spacing, 1e-300)))
    assert 0.0 < worst <= 1.0


def test_sphere_statement_lies_within_the_chord_sag(cases):
    """The statement alone: on the sphere meshes the distance to the mesh is the distance to the sphere within the sag."""
    for name, key in (("sphere24", "off_lattice_24"), ("sphere17", "on_sample_17")):
        v, f, q, max_dist, (d, face, d2) = cases[name]
        _, centre, r = SPHERES[key]
        check_sphere_mesh(v, f, centre, r)
        L = np.sqrt(3.0)
        live = face >= 0
        assert live.sum() > 2000 and (~live).sum() > 1000
        off = np.abs(np.sqrt(d2) - np.abs(np.linalg.norm(q.astype(np.float64) - np.asarray(centre), axis=1) - r))
        assert off[live].max() <= L * L / (8.0 * (r - L)), (name, off[live].max())


def test_query_groups_are_populated(cases):
    for name in ("sphere24", "sphere17", "plane"):
        v, f, q, max_dist, (d, face, d2) = cases[name]
        root = np.sqrt(d2)
        assert (root <= 0.0101).sum() >= N_QUERIES // 3 - 8, name
        assert ((root > 0.0101) & (face >= 0)).sum() >= N_QUERIES // 4, name
        assert (face < 0).sum() >= N_QUERIES // 3, name
        L = reach(q, v, f, statement_unclamped_face(q, v, f, d2, face))
        assert (np.abs(root - max_dist) <= tolerance(root, L)[0]).mean() < 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 2. GPU
# ---------------------------------------------------------------------------------------------------------------------
def _run(dev, points, vertices, faces, max_dist, dtype=torch.int64):
    from pointmvsnet_amd import mesh_distance as D
    d, f = D.point_mesh_distances(torch.from_numpy(np.asarray(points, np.float32)).to(dev),
                                  torch.from_numpy(np.asarray(vertices, np.float32)).to(dev),
                                  torch.from_numpy(np.asarray(faces, np.int64).reshape(-1, 3)).to(dev).to(dtype), max_dist,
                                  return_face=True)
    assert d.dtype == torch.float32 and f.dtype == torch.int64 and d.shape == f.shape == (len(points),)
    return d.cpu().numpy(), f.cpu().numpy(), D.last_grid_report()


@pytest.mark.gpu
def test_dyadic_cases_bit_for_bit(dev):
    want = np.sqrt(DYADIC_D2).astype(np.float32)
    d, f, _ = _run(dev, DYADIC_QUERIES, DYADIC_TRIANGLE, [[0, 1, 2]], 20.0)
    assert np.array_equal(d, want) and (f == 0).all()
    d, f, _ = _run(dev, DYADIC_QUERIES, DYADIC_TRIANGLE, [[0, 1, 2]] * 3, 20.0, dtype=torch.int32)
    assert np.array_equal(d, want) and (f == 0).all()                       # the tie goes to the smallest face index
    d, f, _ = _run(dev, DYADIC_QUERIES, DYADIC_TRIANGLE, [[0, 1, 1]], 20.0)
    assert np.array_equal(d, np.sqrt(SEGMENT_D2).astype(np.float32)) and (f == 0).all()
    # the point (b, b, b) listed before the triangle: query 4 is 5 from both, and the tie goes to face 0
    d, f, _ = _run(dev, DYADIC_QUERIES, DYADIC_TRIANGLE, [[1, 1, 1], [0, 1, 2]], 20.0)
    assert f.tolist() == [1, 1, 1, 1, 0, 1, 1, 1] and np.array_equal(d, want)
    d, f, _ = _run(dev, DYADIC_QUERIES, DYADIC_TRIANGLE, [[1, 1, 1], [0, 1, 2]], 4.5)       # the cap rule: 5 >= 4.5
    assert f.tolist() == [1, -1, 1, 1, -1, -1, 1, 1] and np.array_equal(d, np.where(f < 0, np.float32(4.5), want))
    d, f, _ = _run(dev, DYADIC_QUERIES, DYADIC_TRIANGLE, [[0, 1, 2]], 5.0)                  # d == max_dist is the cap
    assert f.tolist() == [0, -1, 0, 0, -1, -1, 0, 0] and np.array_equal(d, np.where(f < 0, np.float32(5.0), want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere24", "sphere17", "plane"])
def test_random_queries_against_brute_force(dev, cases, name):
    v, f, q, max_dist, want = cases[name]
    d, face, grid = _run(dev, q, v, f, max_dist)
    figures = check_against_statement(q, v, f, max_dist, d, face, want)
    if name != "plane":
        _, centre, r = SPHERES[{"sphere24": "off_lattice_24", "sphere17": "on_sample_17"}[name]]
        live = face >= 0
        off = np.abs(d.astype(np.float64) - np.abs(np.linalg.norm(q.astype(np.float64) - np.asarray(centre), axis=1) - r))
        L = np.sqrt(3.0)
        assert off[live].max() <= L * L / (8.0 * (r - L)), off[live].max()
        figures["sphere_off_over_sag"] = float(off[live].max() / (L * L / (8.0 * (r - L))))
    assert grid["queries"] == len(q) and grid["faces"] == len(f) and 0 < grid["fine_pairs"] <= grid["budget"]
    print(name, figures, grid)
    report("mesh_distance", **dict(figures, second_pass=grid["second_pass_queries"], fine_pairs=grid["fine_pairs"],
                                   fine_edge=grid["fine_edge"]))


@pytest.mark.gpu
def test_both_passes_and_the_pair_budget(dev, cases):
    from pointmvsnet_amd import mesh_distance as D
    v, f, q, max_dist, want = cases["budget"]
    d, face, grid = _run(dev, q, v, f, max_dist)
    budget = D.pair_budget(len(f))
    assert grid["budget"] == budget and grid["fine_edge_first"] == pytest.approx(0.5)
    assert grid["fine_pairs_first"] > budget                                # the plane's two faces alone exceed it
    assert grid["fine_widenings"] >= 1 and grid["fine_edge"] == grid["fine_edge_first"] * 2 ** grid["fine_widenings"]
    assert 0 < grid["fine_pairs"] <= budget and 0 < grid["coarse_pairs"] <= budget
    assert grid["coarse_edge"] >= max_dist
    # some queries can only finish in the second pass: farther from every face than the fine rings reach, inside max_dist
    far = (np.sqrt(want[2]) > D.FINE_RINGS * grid["fine_edge"]) & (want[1] >= 0)
    assert far.sum() >= 100 and grid["second_pass_queries"] >= far.sum() > 0
    assert grid["second_pass_queries"] < len(q)                              # and the first pass finished the others
    figures = check_against_statement(q, v, f, max_dist, d, face, want)
    assert (face[far] >= 0).all() and (face == 0).sum() > 100 and (face == 1).sum() > 100 and (face > 1).sum() > 100
    print("budget", figures, grid)
    report("mesh_distance", **dict(figures, second_pass=grid["second_pass_queries"], fine_pairs=grid["fine_pairs"],
                                   fine_edge=grid["fine_edge"]))
    # a call that the first pass finishes alone builds no coarse grid
    _, _, grid = _run(dev, q[np.sqrt(want[2]) < 0.5], v, f, max_dist)
    assert grid["second_pass_queries"] == 0 and "coarse_pairs" not in grid


@pytest.mark.gpu
def test_results_are_a_pure_function_of_the_input(dev, cases):
    v, f, q, max_dist, want = cases["sphere17"]
    d, face, _ = _run(dev, q, v, f, max_dist)
    d2, face2, _ = _run(dev, q, v, f, max_dist)
    assert d.tobytes() == d2.tobytes() and face.tobytes() == face2.tobytes()
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(f))
    dp, facep, _ = _run(dev, q, v, f[perm], max_dist)
    assert dp.tobytes() == d.tobytes()
    back = np.where(facep >= 0, perm[np.maximum(facep, 0)], -1)
    assert np.array_equal(back < 0, face < 0)
    assert np.array_equal(face_d2(q, v, f, back), face_d2(q, v, f, face))
    order = rng.permutation(len(q))
    dq, faceq, _ = _run(dev, q[order], v, f, max_dist)
    assert dq.tobytes() == d[order].tobytes() and faceq.tobytes() == face[order].tobytes()


@pytest.mark.gpu
def test_edge_cases(dev):
    from pointmvsnet_amd import mesh_distance as D
    v, f = sphere_mesh("on_sample_17")
    q = np.concatenate([v[::7] + np.float32(0.25), v[f[5]] + np.float32(0.125)]).astype(np.float32)   # some at face 5 itself
    d, face, _ = _run(dev, q[:0], v, f, 3.0)
    assert d.shape == (0,) and face.shape == (0,)
    for vv, ff in ((v, f[:0]), (v[:0], f[:0])):
        d, face, grid = _run(dev, q, vv, ff, 3.0)
        assert (d == np.float32(3.0)).all() and (face == -1).all() and grid == {}
    # one NaN vertex: its faces are skipped, the others are still found
    bad = v.copy()
    bad[f[5, 0], 1] = np.nan
    skipped = (f == f[5, 0]).any(axis=1)
    assert 1 <= skipped.sum() < 40
    d, face, _ = _run(dev, q, bad, f, 3.0)
    want = statement_distances(q, bad, f, 3.0)
    check_against_statement(q, bad, f, 3.0, d, face, want)
    assert not np.isin(face, np.flatnonzero(skipped)).any() and (face >= 0).sum() > len(q) // 2
    full = statement_distances(q, v, f, 3.0)
    assert (full[1] != want[1]).any()                                       # and the skipped faces mattered
    allnan = np.full_like(v, np.nan)
    d, face, _ = _run(dev, q, allnan, f, 3.0)
    assert (d == np.float32(3.0)).all() and (face == -1).all()
    tq, tv, tf = (torch.from_numpy(x) for x in (q, v, f))
    for wrong in (np.int64(len(v)), np.int64(-1)):
        broken = tf.clone()
        broken[3, 2] = int(wrong)
        with pytest.raises(ValueError, match="face indices run from"):
            D.point_mesh_distances(tq.to(dev), tv.to(dev), broken.to(dev))
    if dev.type == "cuda":
        for args in ((tq, tv.to(dev), tf.to(dev)), (tq.to(dev), tv, tf.to(dev)), (tq.to(dev), tv.to(dev), tf)):
            with pytest.raises(RuntimeError, match="no CPU path"):
                D.point_mesh_distances(*args)


def _scene(dev):
    """A mesh (the plane scene's), a ground-truth cloud on and around it, and a noisy cloud of it."""
    v, f = plane_mesh()[:2]
    rng = np.random.default_rng(5)
    tri = v.astype(np.float64)[f]
    w = rng.dirichlet(np.ones(3), 6000)
    on = (tri[rng.integers(0, len(tri), 6000)] * w[:, :, None]).sum(axis=1)
    diag = np.linalg.norm(v.max(axis=0) - v.min(axis=0))
    gt = np.concatenate([on + rng.normal(size=on.shape) * 1e-4 * diag, on[:200] + diag]).astype(np.float32)
    return (torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(gt).to(dev))


@pytest.mark.gpu
def test_scores_equal_their_composition(dev):
    from pointmvsnet_amd import evaluation as EV
    from pointmvsnet_amd import mesh_distance as D
    from pointmvsnet_amd import mesh_ops as M
    v, f, gt = _scene(dev)
    diag = float((v.amax(0) - v.amin(0)).norm())
    pitch, cap = float(np.float32(diag / 150.0)), float(np.float32(diag / 4.0))
    lo = gt[:6000].amin(0)
    plane = [0.0, 0.0, 1.0, -float(gt[:6000, 2].median())]
    mask = torch.zeros((9, 72, 72), dtype=torch.bool)                        # the lower half of the cloud's x range
    mask[:4] = True
    res = float(gt[:6000, 0].max() - lo[0]) / 8.0
    kw = {"obs_mask": mask, "bb_min": lo.cpu().numpy(), "res": res, "plane": plane}

    def mm(d):
        return EV._mean_median(d)

    # a mesh against a cloud
    got = D.evaluate_mesh(v, f, gt, pitch=pitch, max_dist=cap, seed=4, return_distances=True, **kw)
    samples = M.sample_surface(v, f, pitch, seed=4)[0]
    d_acc = EV.nearest_distances(samples, gt, cap)
    d_comp = D.point_mesh_distances(gt, v, f, cap)
    acc_used = (d_acc < cap) & EV.in_obs_mask(samples, mask, kw["bb_min"], res)
    comp_used = (d_comp < cap) & EV.above_plane(gt, plane)
    assert torch.equal(got["samples"], samples) and torch.equal(got["d_acc"], d_acc) and torch.equal(got["d_comp"], d_comp)
    assert torch.equal(got["acc_used"], acc_used) and torch.equal(got["comp_used"], comp_used)
    assert 0 < int(acc_used.sum()) < len(samples) and 0 < int(comp_used.sum()) < len(gt) - 200
    want = {"accuracy_mean": mm(d_acc[acc_used])[0], "accuracy_median": mm(d_acc[acc_used])[1],
            "completeness_mean": mm(d_comp[comp_used])[0], "completeness_median": mm(d_comp[comp_used])[1],
            "n_data": len(samples), "n_data_thinned": len(samples), "n_samples": len(samples), "n_data_used": int(acc_used.sum()),
            "n_gt": len(gt), "n_gt_used": int(comp_used.sum())}
    want["overall"] = (want["accuracy_mean"] + want["completeness_mean"]) / 2.0
    plain = D.evaluate_mesh(v, f, gt, pitch=pitch, max_dist=cap, seed=4, **kw)
    assert plain == want and {k: got[k] for k in want} == want
    assert set(EV.evaluate_point_cloud(gt[:50], gt[:50])) | {"n_samples"} == set(plain)
    # exact against sampled, per ground-truth point: the surface is never farther than a sample of it
    d_sampled = EV.nearest_distances(gt, samples, cap)
    assert bool((d_comp.double() <= d_sampled.double() * (1.0 + 4.0 * 2.0 ** -24)).all())
    both = (d_comp < cap) & (d_sampled < cap)
    gap = float(d_sampled[both].double().mean() - d_comp[both].double().mean())
    assert int(both.sum()) >= 6000 and abs(gap) < pitch
    # a cloud against a surface
    data = gt[:6000]
    got = D.evaluate_point_cloud_on_mesh(data, v, f, gt_pitch=pitch, min_dist=pitch, max_dist=cap, seed=9,
                                         return_distances=True, **kw)
    thinned = EV.thin_points(data, pitch)
    samples = M.sample_surface(v, f, pitch, seed=9)[0]
    d_acc = D.point_mesh_distances(thinned, v, f, cap)
    d_comp = EV.nearest_distances(samples, thinned, cap)
    acc_used = (d_acc < cap) & EV.in_obs_mask(thinned, mask, kw["bb_min"], res)
    comp_used = (d_comp < cap) & EV.above_plane(samples, plane)
    for key, t in (("data_thinned", thinned), ("samples", samples), ("d_acc", d_acc), ("d_comp", d_comp), ("acc_used", acc_used),
                   ("comp_used", comp_used)):
        assert torch.equal(got[key], t), key
    want = {"accuracy_mean": mm(d_acc[acc_used])[0], "accuracy_median": mm(d_acc[acc_used])[1],
            "completeness_mean": mm(d_comp[comp_used])[0], "completeness_median": mm(d_comp[comp_used])[1],
            "n_data": len(data), "n_data_thinned": len(thinned), "n_samples": len(samples), "n_data_used": int(acc_used.sum()),
            "n_gt": len(samples), "n_gt_used": int(comp_used.sum())}
    want["overall"] = (want["accuracy_mean"] + want["completeness_mean"]) / 2.0
    assert {k: got[k] for k in want} == want and 0 < want["n_data_used"] < want["n_data_thinned"] < want["n_data"]
    unthinned = D.evaluate_point_cloud_on_mesh(data, v, f, gt_pitch=pitch, max_dist=cap, thin=False)
    assert unthinned["n_data_thinned"] == len(data) and unthinned["n_data_used"] == len(data)
    # an empty mesh scores nothing
    empty = D.evaluate_mesh(v, f[:0], gt, pitch=pitch, max_dist=cap)
    assert empty["n_samples"] == 0 and empty["n_gt_used"] == 0 and np.isnan(empty["completeness_mean"])
    report("mesh_distance", completeness_exact=plain["completeness_mean"], sampled_minus_exact=gap, pitch=pitch,
           samples=len(samples))


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_ply_route(dev, tmp_path):
    from pointmvsnet_amd import mesh_distance as D
    v, f, gt = _scene(dev)
    gt = gt[:6000]
    diag = float((v.amax(0) - v.amin(0)).norm())
    pitch, cap = float(np.float32(diag / 150.0)), float(np.float32(diag / 4.0))
    mesh_ply, cloud_ply = str(tmp_path / "mesh.ply"), str(tmp_path / "cloud.ply")
    IO.write_ply(mesh_ply, v.cpu().numpy(), faces=f.cpu().numpy())
    IO.write_ply(cloud_ply, gt.cpu().numpy())
    tool = _load_tool("evaluate_dtu")
    # --data-mesh: the data file is a mesh, the ground truth a cloud
    want = D.evaluate_mesh(v, f, gt, pitch=pitch, max_dist=cap)
    assert D.evaluate_mesh_ply(mesh_ply, cloud_ply, pitch=pitch, max_dist=cap, device=dev) == want
    args = tool.parse_args(["--data", mesh_ply, "--gt", cloud_ply, "--data-mesh", "--pitch", repr(pitch), "--max-dist", repr(cap)])
    assert tool.score(args, device=dev) == want and want["n_gt_used"] == 6000
    # --gt-mesh: the data file is a cloud, the ground truth a surface
    want = D.evaluate_point_cloud_on_mesh(gt, v, f, gt_pitch=pitch, min_dist=pitch, max_dist=cap)
    assert D.evaluate_ply_on_mesh(cloud_ply, mesh_ply, gt_pitch=pitch, min_dist=pitch, max_dist=cap, device=dev) == want
    args = tool.parse_args(["--data", cloud_ply, "--gt-mesh", mesh_ply, "--pitch", repr(pitch), "--min-dist", repr(pitch),
                            "--max-dist", repr(cap)])
    assert tool.score(args, device=dev) == want and want["n_data_used"] == want["n_data_thinned"] > 100
    # a cloud where a mesh is needed is an error, not a score
    with pytest.raises(ValueError, match="has no faces"):
        D.evaluate_mesh_ply(cloud_ply, cloud_ply, device=dev)
    with pytest.raises(SystemExit):
        tool.parse_args(["--data", cloud_ply])                                # neither --gt nor --gt-mesh
    with pytest.raises(SystemExit):
        tool.parse_args(["--data", mesh_ply, "--data-mesh", "--gt-mesh", mesh_ply])      # mesh against mesh is out of scope
