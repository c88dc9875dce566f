"""TSDF integration and marching tetrahedra (pointmvsnet_amd/tsdf.py, csrc/tsdf.hip) against NumPy statements of the
specification, and the layers above: PLY faces, ``ScanAccumulator.mesh``.

The reference has no such step: the specification is the docstring of pointmvsnet_amd/tsdf.py, and the yardsticks are
``statement_integrate`` (float64) and ``statement_extract`` below, written from that text with no code shared with the
product.  Both are fed what the kernels are fed: the float32 ``proj``, depth maps, origin, voxel and ``trunc``, and sample
positions evaluated as ``o + float(i) * voxel`` in NumPy float32 (which is the kernel's arithmetic bit for bit), so input
rounding is not part of any error.

The integration bound (test_integration_matches_the_float64_statement)
---------------------------------------------------------------------
eps = 2^-24 per float32 rounding.  ``test_render.project64`` gives u, w_, z in float64 with the derived ``eps_u``,
``eps_v``, ``eps_z``.  A (sample, view) is *ambiguous* when a decision of the statement is within the kernel's rounding of
flipping: ``z`` within ``eps_z`` of a depth bound; ``u`` or ``w_`` within ``eps_u`` / ``eps_v`` of an integer (pixel and map
borders are integers); ``sdf = d - z`` within ``eps_z + eps |sdf|`` (z's error and the subtraction's rounding) of
``+-trunc``.  A sample is ambiguous if any of its views is; at most 0.5 % of the samples may be, and the comparison is
made on all the others.  There the kernel takes the statement's decisions, so ``W``, ``CW``, ``CS`` and ``colour()`` are
equal, and a term ``fminf(sdf, trunc) / trunc`` differs from the statement's by at most ``(eps_z + eps |sdf|) / trunc``
(the subtraction) plus ``eps`` (the quotient, a number of at most 1 in magnitude; one more ``eps`` covers the second
order).  ``S`` adds ``W`` such terms with ``W - 1`` roundings of partial sums; ``tsdf = S / W`` is one more rounding.  A
mean of perturbed terms is perturbed by at most their largest perturbation, and every partial sum is at most ``W`` in
magnitude, i.e. at most 1 after the division, so
``|tsdf - tsdf64| <= max_v((eps_z + eps |sdf|) / trunc + 2 eps) + (W + 1) eps``.  Nothing is tuned.

The extraction (teacher-forced)
-------------------------------
``statement_extract`` is fed the GPU's own ``tsdf`` and ``weight``, so ``tsdf < 0`` is exact and there is no tie band:
keys are equal, faces are equal after rotating each face's smallest index to the front, positions are within
``6 eps (|p_a| + |p_b|)`` per coordinate of the float64 interpolation (``t``: a difference and a quotient; then a
difference, a product and a sum, each at most that size), colours within one level.

The spheres.  ``tsdf = clip((|p - c| - r) / trunc, -1, 1)``, voxel 1, trunc 3.  The distance function restricted to an edge
of length at most ``L = sqrt(3) voxel`` is convex with curvature at most ``1 / (r - L)``, so its chord sags by at most
``L^2 / (8 (r - L))``: that bounds how far a vertex lies from the sphere.  The mesh must be a closed 2-manifold of Euler
characteristic 2 with every non-degenerate face outward, and its signed volume must lie between the balls of radius
``r -+`` that bound.  The 17^3 case has its centre on a sample and 30 samples exactly 0 (outside by definition); its
zero-area faces are kept and the surface stays closed.

Measured on an MI355X, and the same on tests/hipemu (the kernel source compiled for the host): ambiguous share 0.074 % and
0.134 % of the samples, no ``W``, ``CW``, ``CS`` or colour differs outside it, largest ``|tsdf - tsdf64|`` 0.38 and 0.39 of
the bound; closed form: 0.45 eps, every vertex on ``z = D`` exactly; extraction: keys and faces equal in all eight cases,
positions at most 0.29 of the bound on the scene and 0.09 on the spheres, colours equal.  ``conftest.report`` carries the
figures (``tsdf_integration``, ``tsdf_closed_form``, ``tsdf_extraction``).
"""

import numpy as np
import pytest
import torch

from conftest import report
from test_fusion import _back_project, _pixel_centres, make_plane_scene
from test_render import EPS32, project64
from pointmvsnet_amd import render
from pointmvsnet_amd.utils import io as IO

DEPTH_MIN, DEPTH_MAX = 1e-3, 1e5
GRIDS = ((21, 19, 17), (33, 29, 25))                   # no multiple of a block dimension
TETS = ((0, 1, 3, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 6, 4, 7), (0, 4, 5, 7), (0, 5, 1, 7))


# ---------------------------------------------------------------------------------------------------------------------
# the statements
# ---------------------------------------------------------------------------------------------------------------------
def sample_positions(origin, voxel, dims):
    """(nz, ny, nx, 3) float32: ``o + float(i) * voxel`` per coordinate in float32, as the kernels evaluate it."""
    o, vx = np.asarray(origin, np.float32), np.float32(voxel)
    axes = [o[a] + np.arange(dims[a]).astype(np.float32) * vx for a in range(3)]
    assert all(a.dtype == np.float32 for a in axes)
    Z, Y, X = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([X, Y, Z], axis=-1)


def statement_integrate(depths, images, proj, origin, voxel, dims, trunc, depth_min=DEPTH_MIN, depth_max=DEPTH_MAX):
    """The integration of the docstring in float64.  Returns a dict: W, S, tsdf (float64), CS, CW, colour, the per-sample
    error bound ``bound`` and ``ambiguous``, and the two non-vacuity masks."""
    V, h, w = depths.shape
    nx, ny, nz = dims
    pts = sample_positions(origin, voxel, dims).reshape(-1, 3)
    g = project64(pts, proj)
    lo, hi, tr = float(np.float32(depth_min)), float(np.float32(depth_max)), float(np.float32(trunc))
    N = len(pts)
    W, S = np.zeros(N, np.int64), np.zeros(N)
    CS, CW = np.zeros((N, 3), np.int64), np.zeros(N, np.int64)
    ambiguous, near = np.zeros(N, bool), np.zeros(N, bool)
    term_err = np.zeros(N)
    for v in range(V):
        z, ez, u, eu, y_, ev = g["z"][v], g["eps_z"][v], g["u"][v], g["eps_u"][v], g["v"][v], g["eps_v"][v]
        ambiguous |= (np.abs(z - lo) <= ez) | (np.abs(z - hi) <= ez)
        ok = (z > lo) & (z < hi)
        with np.errstate(invalid="ignore"):
            ambiguous |= ok & ((np.abs(u - np.round(u)) <= eu) | (np.abs(y_ - np.round(y_)) <= ev))
            ok &= (u >= 0) & (u < w) & (y_ >= 0) & (y_ < h)
        x = np.where(ok, np.floor(u), 0).astype(np.int64)
        y = np.where(ok, np.floor(y_), 0).astype(np.int64)
        d = depths[v][y, x].astype(np.float64)
        ok &= (d > lo) & (d < hi)
        sdf = d - z
        slack = ez + EPS32 * np.abs(sdf)
        ambiguous |= ok & ((np.abs(sdf - tr) <= slack) | (np.abs(sdf + tr) <= slack))
        ok &= ~(sdf < -tr)
        S += np.where(ok, np.minimum(sdf, tr) / tr, 0.0)
        W += ok
        term_err = np.maximum(term_err, np.where(ok, slack / tr + 2 * EPS32, 0.0))
        col = ok & (np.abs(sdf) <= tr)
        near |= col
        if images is not None:
            CS += np.where(col[:, None], images[v][y, x].astype(np.int64), 0)
            CW += col
    with np.errstate(invalid="ignore", divide="ignore"):
        tsdf = np.where(W > 0, S / W, 1.0)
        colour = np.where(CW[:, None] > 0, (2 * CS + CW[:, None]) // np.maximum(2 * CW[:, None], 1), 0).astype(np.uint8)
    shape = (nz, ny, nx)
    return {"W": W.reshape(shape), "S": S.reshape(shape), "tsdf": tsdf.reshape(shape), "CS": CS.reshape(shape + (3,)),
            "CW": CW.reshape(shape), "colour": colour.reshape(shape + (3,)), "ambiguous": ambiguous.reshape(shape),
            "bound": (term_err + (W + 1) * EPS32).reshape(shape), "near": near.reshape(shape)}


def _vec(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def _tet_triangles(tet, inside):
    """The triangles of one tetrahedron as lists of three (corner, corner) edges, wound by the docstring's rule."""
    P = [c for c in tet if inside[c]]
    Q = [c for c in tet if not inside[c]]
    if len(P) == 1:
        tris = [[(P[0], Q[0]), (P[0], Q[1]), (P[0], Q[2])]]
    elif len(Q) == 1:
        tris = [[(P[0], Q[0]), (P[1], Q[0]), (P[2], Q[0])]]
    elif len(P) == 2:
        e = [(P[0], Q[0]), (P[0], Q[1]), (P[1], Q[1]), (P[1], Q[0])]
        tris = [[e[0], e[1], e[2]], [e[0], e[2], e[3]]]
    else:
        return []
    out_dir = np.mean([_vec(c) for c in Q], axis=0) - np.mean([_vec(c) for c in P], axis=0)
    for tri in tris:
        m = [(_vec(p) + _vec(q)) / 2.0 for p, q in tri]
        if not np.dot(np.cross(m[1] - m[0], m[2] - m[0]), out_dir) > 0:
            tri[1], tri[2] = tri[2], tri[1]
    return tris


def statement_extract(tsdf, weight, origin, voxel, min_weight=1, colour=None):
    """Marching tetrahedra of the docstring.  Returns keys (Nv,) int64, faces (Nf, 3) int64, vertices (Nv, 3) float64,
    colours (Nv, 3) float64 before rounding or None, and per vertex ``scale`` = |p_a| + |p_b| per coordinate (Nv, 3)."""
    nz, ny, nx = tsdf.shape
    inside = tsdf < 0
    ok = weight >= min_weight
    corners = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]

    def cell_view(a, c):
        dx, dy, dz = corners[c]
        return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

    if min(nx, ny, nz) < 2:
        cells = np.zeros((0, 3), np.int64)
    else:
        active = np.all([cell_view(ok, c) for c in range(8)], axis=0)
        n_in = np.sum([cell_view(inside, c) for c in range(8)], axis=0)
        cells = np.argwhere(active & (n_in > 0) & (n_in < 8))                      # (k, j, i) ascending = cell index ascending
    tri_keys = []
    for k, j, i in cells:
        ins = [bool(inside[k + dz, j + dy, i + dx]) for dx, dy, dz in corners]
        for tet in TETS:
            for tri in _tet_triangles(tet, ins):
                row = []
                for p, q in tri:
                    lo, hi_ = (p, q) if np.all(_vec(p) <= _vec(q)) else (q, p)
                    assert np.all(_vec(lo) <= _vec(hi_))
                    d = _vec(hi_) - _vec(lo)
                    a = np.array([i, j, k]) + _vec(lo)
                    row.append(((int(a[2]) * ny + int(a[1])) * nx + int(a[0])) * 8 + int(d[0] + 2 * d[1] + 4 * d[2]))
                tri_keys.append(row)
    tri_keys = np.asarray(tri_keys, np.int64).reshape(-1, 3)
    keys = np.unique(tri_keys)
    faces = np.searchsorted(keys, tri_keys)
    pos = sample_positions(origin, voxel, (nx, ny, nz)).astype(np.float64)
    a = keys >> 3
    ai, aj, ak = a % nx, (a // nx) % ny, a // (nx * ny)
    bi, bj, bk = ai + (keys & 1), aj + ((keys >> 1) & 1), ak + ((keys >> 2) & 1)
    fa, fb = tsdf[ak, aj, ai].astype(np.float64), tsdf[bk, bj, bi].astype(np.float64)
    assert ((fa < 0) != (fb < 0)).all()
    t = fa / (fa - fb)
    pa, pb = pos[ak, aj, ai], pos[bk, bj, bi]
    vertices = pa + t[:, None] * (pb - pa)
    colours = None
    if colour is not None:
        ca, cb = colour[ak, aj, ai].astype(np.float64), colour[bk, bj, bi].astype(np.float64)
        colours = ca + t[:, None] * (cb - ca)
    return keys, faces, vertices, colours, np.abs(pa) + np.abs(pb)


def canonical(faces):
    """Every face rotated so that its smallest index comes first."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if not len(faces):
        return faces
    first = np.argmin(faces, axis=1)
    idx = (first[:, None] + np.arange(3)[None, :]) % 3
    return np.take_along_axis(faces, idx, axis=1)


def sphere_volume(n, centre, r, trunc=3.0):
    """``(tsdf (n, n, n) float32, weight int32)`` of a sphere sampled at the integer lattice (origin 0, voxel 1)."""
    pos = sample_positions((0.0, 0.0, 0.0), 1.0, (n, n, n)).astype(np.float64)
    dist = np.sqrt(((pos - np.asarray(centre, np.float64)) ** 2).sum(-1))
    return np.clip((dist - r) / trunc, -1.0, 1.0).astype(np.float32), np.ones((n, n, n), np.int32)


SPHERES = {"off_lattice_24": (24, (11.3, 11.6, 11.45), 8.3), "on_sample_17": (17, (8.0, 8.0, 8.0), 5.0)}


def check_sphere_mesh(vertices, faces, centre, r, voxel=1.0):
    """The sphere conditions of the module docstring on a mesh; returns (largest |distance - r| / bound, zero-area faces)."""
    vertices, faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    centre = np.asarray(centre, np.float64)
    assert len(faces) > 100 and faces.min() >= 0 and faces.max() < len(vertices)
    assert len(np.unique(faces)) == len(vertices)                                  # no vertex is unused
    directed = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    assert (directed[:, 0] != directed[:, 1]).all()
    code = directed[:, 0] * len(vertices) + directed[:, 1]
    assert len(np.unique(code)) == len(code), "a directed edge occurs twice"
    assert np.isin(directed[:, 1] * len(vertices) + directed[:, 0], code).all(), "an edge without its reverse: not closed"
    assert len(vertices) - len(code) // 2 + len(faces) == 2                        # Euler characteristic
    p0, p1, p2 = (vertices[faces[:, c]] for c in range(3))
    normal = np.cross(p1 - p0, p2 - p0)
    solid = np.linalg.norm(normal, axis=1) > 1e-12 * voxel * voxel
    outward = (normal * ((p0 + p1 + p2) / 3.0 - centre)).sum(1)
    assert (outward[solid] > 0).all(), "%d faces look inward" % int((outward[solid] <= 0).sum())
    L = np.sqrt(3.0) * voxel
    bound = L * L / (8.0 * (r - L))
    off = np.abs(np.linalg.norm(vertices - centre, axis=1) - r)
    assert off.max() <= bound, (off.max(), bound)
    volume = (p0 * np.cross(p1, p2)).sum() / 6.0
    assert 4.0 / 3.0 * np.pi * (r - bound) ** 3 <= volume <= 4.0 / 3.0 * np.pi * (r + bound) ** 3, volume
    return off.max() / bound, int((~solid).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the scene of the share check and the GPU comparison
# ---------------------------------------------------------------------------------------------------------------------
def plane_scene_box():
    depths, K, E, images, _ = make_plane_scene(5)
    V, h, w = depths.shape
    pix = _pixel_centres(h, w)
    pts = np.concatenate([_back_project(K[v], E[v], pix, depths[v].astype(np.float64))[depths[v] > 0] for v in range(V)])
    return depths, K, E, images, np.percentile(pts, 2, axis=0), np.percentile(pts, 98, axis=0)


def grid_of(lo, hi, dims):
    """The grid of ``dims`` samples centred on the box, its pitch the largest axis pitch (so it spans the box on every axis
    and reaches beyond it, before and behind the plane, on the others); trunc = 3 voxel."""
    voxel = float(np.float32(np.max((hi - lo) / (np.asarray(dims) - 1))))
    origin = (lo + hi) / 2.0 - voxel * (np.asarray(dims) - 1) / 2.0
    return np.asarray(origin, np.float32), voxel, float(np.float32(3.0 * voxel))


@pytest.fixture(scope="module")
def plane_scene():
    depths, K, E, images, lo, hi = plane_scene_box()
    proj = render.world_maps(K, E)
    out = {"depths": depths, "K": K, "E": E, "images": images, "proj": proj, "grids": {}}
    for dims in GRIDS:
        origin, voxel, trunc = grid_of(lo, hi, dims)
        out["grids"][dims] = (origin, voxel, trunc, statement_integrate(depths, images, proj, origin, voxel, dims, trunc))
    return out


@pytest.fixture(scope="module")
def sphere_statements():
    out = {}
    for name, (n, centre, r) in SPHERES.items():
        f, wgt = sphere_volume(n, centre, r)
        out[name] = (f, wgt, statement_extract(f, wgt, (0.0, 0.0, 0.0), 1.0))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SPHERES))
def test_extraction_statement_on_spheres(sphere_statements, name):
    """The statement alone: closed 2-manifold, Euler characteristic 2, outward faces, vertices and volume within the sag."""
    n, centre, r = SPHERES[name]
    f, _, (keys, faces, vertices, _, _) = sphere_statements[name]
    assert (np.diff(keys) > 0).all()
    worst, flat = check_sphere_mesh(vertices, faces, centre, r)
    print(name, "vertices", len(vertices), "faces", len(faces), "distance / bound", worst, "zero-area faces", flat)
    if name == "on_sample_17":
        assert int((f == 0).sum()) == 30 and flat == 228
    else:
        assert int((f == 0).sum()) == 0 and flat == 0


@pytest.mark.parametrize("dims", GRIDS)
def test_integration_statement_near_ties_and_not_vacuous(plane_scene, dims):
    st = plane_scene["grids"][dims][3]
    share = st["ambiguous"].mean()
    seen3, near = (st["W"] >= 3).mean(), st["near"].mean()
    print(dims, "ambiguous share", share, "W >= 3", seen3, "within trunc", near)
    assert share <= 0.005
    assert seen3 >= 0.10 and near >= 0.15


def test_arguments_are_checked_before_a_device_is_needed(plane_scene):
    from pointmvsnet_amd import tsdf as T
    ok = dict(origin=(0.0, 0.0, 0.0), voxel=1.0, dims=(4, 4, 4), trunc=3.0)
    for bad in (dict(voxel=0.0), dict(voxel=-1.0), dict(trunc=0.0), dict(trunc=float("nan")), dict(dims=(4, 4)),
                dict(dims=(4, 0, 4)), dict(dims=(4, 2.5, 4)), dict(dims=(2048, 2048, 512)), dict(origin=(0.0, 1.0)),
                dict(origin=(0.0, float("inf"), 0.0))):
        with pytest.raises(ValueError):
            T.TSDFVolume(**dict(ok, **bad))
    T.TSDFVolume(**dict(ok, dims=(2048, 2048, 511)))                                # 2^31 - 2^22 samples: stated, not allocated
    depths, K, E = torch.from_numpy(plane_scene["depths"]), plane_scene["K"], plane_scene["E"]
    images = torch.from_numpy(plane_scene["images"])
    vol, col = T.TSDFVolume(**ok), T.TSDFVolume(with_colour=True, **ok)
    with pytest.raises(ValueError, match="cameras"):
        vol.integrate(depths, K[:3], E[:3])
    with pytest.raises(ValueError, match="depths must be"):
        vol.integrate(depths[0], K, E)
    with pytest.raises(ValueError, match="depth_min"):
        vol.integrate(depths, K, E, depth_min=5.0, depth_max=1.0)
    with pytest.raises(ValueError, match="images"):
        vol.integrate(depths, K, E, images=images)
    with pytest.raises(ValueError, match="images"):
        col.integrate(depths, K, E)
    col.views = T.MAX_VIEWS_COLOUR - 4
    with pytest.raises(ValueError, match="overflow"):
        col.integrate(depths, K, E, images=images)
    f, wgt = torch.zeros((3, 3, 3)), torch.ones((3, 3, 3), dtype=torch.int32)
    for args, kw in (((f.double(), wgt, (0, 0, 0), 1.0), {}), ((f, wgt.long(), (0, 0, 0), 1.0), {}),
                     ((f, wgt[:2], (0, 0, 0), 1.0), {}), ((f, wgt, (0, 0), 1.0), {}), ((f, wgt, (0, 0, 0), 0.0), {}),
                     ((f, wgt, (0, 0, 0), 1.0), {"min_weight": 1.5}),
                     ((f, wgt, (0, 0, 0), 1.0), {"colour": torch.zeros((3, 3, 3, 3))})):
        with pytest.raises(ValueError):
            T.extract_mesh(*args, **kw)
    with pytest.raises(ValueError):
        T.dims_for(((0, 0, 0), (1, 1, 1)), 0.0)
    with pytest.raises(ValueError):
        T.dims_for(((0, 0, 0), (1, -1, 1)), 0.5)
    with pytest.raises(ValueError, match="no pixel"):
        T.volume_bounds(torch.zeros((5, 4, 4)), K, E)


def test_kernels_are_built_bound_and_have_no_cpu_path(lib_built):
    import json
    from pointmvsnet_amd import _lib, build, tsdf as T
    names = {"pf_tsdf_integrate_f32", "pf_tsdf_count_triangles", "pf_tsdf_emit_triangles", "pf_tsdf_vertices_f32"}
    assert names <= set(_lib.PROTOTYPES) and "tsdf.hip" in build.SOURCES
    usage = json.load(open(build.USAGE_FILE))["tsdf.hip"]
    kernels = [k for k in usage if "tsdf_" in k]
    assert len(kernels) == 4
    for k in kernels:                                                              # tables in integers: no scratch, no LDS
        assert usage[k]["scratch_bytes_per_lane"] == 0 and usage[k]["static_lds_bytes"] == 0, k
    f, wgt = torch.zeros((3, 3, 3)), torch.ones((3, 3, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.extract_mesh(f, wgt, (0.0, 0.0, 0.0), 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.TSDFVolume((0.0, 0.0, 0.0), 1.0, (3, 3, 3), 2.0, device="cpu").integrate(torch.ones((1, 4, 4)), np.eye(3)[None],
                                                                                   np.eye(4)[None])
    lib = _lib.load()                                                              # limits are checked before any launch
    assert lib.pf_tsdf_count_triangles(None, None, 0, 4, 4, 1, None, None) != 0
    assert lib.pf_tsdf_count_triangles(None, None, 2048, 2048, 512, 1, None, None) != 0
    assert lib.pf_tsdf_count_triangles(None, None, 4, 4, 1, 1, None, None) == 0    # no cells: nothing to do


def test_volume_bounds_and_dims_for(plane_scene):
    """Plain torch, so it runs here: the box of the back-projected valid pixels, and the grid that spans it."""
    from pointmvsnet_amd import tsdf as T
    depths, K, E = plane_scene["depths"], plane_scene["K"], plane_scene["E"]
    V, h, w = depths.shape
    pix = _pixel_centres(h, w)
    pts = np.concatenate([_back_project(K[v], E[v], pix, depths[v].astype(np.float64))[depths[v] > 0] for v in range(V)])
    lo, hi = T.volume_bounds(torch.from_numpy(depths), K, E, pad=2.0)
    tol = 64 * EPS32 * np.abs(pts).max()
    assert np.abs(lo - (pts.min(0) - 2.0)).max() <= tol and np.abs(hi - (pts.max(0) + 2.0)).max() <= tol
    near = T.volume_bounds(torch.from_numpy(depths), K, E, depth_max=650.0)          # the outlier block (x 1.3) is cut
    assert near[1][2] < hi[2] - 50.0
    origin, dims = T.dims_for((lo, hi), 7.0)
    assert (origin == lo).all() and all(isinstance(n, int) for n in dims)
    span = origin + 7.0 * (np.asarray(dims) - 1)
    assert (span >= hi).all() and (span - 7.0 < hi).all()
    assert T.dims_for(((0, 0, 0), (0, 0, 0)), 1.0)[1] == (1, 1, 1)


def test_ply_faces_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(7, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    nrm = rng.normal(size=(7, 3)).astype(np.float32)
    faces = rng.integers(0, 7, (5, 3)).astype(np.int32)
    for colours, normals in ((None, None), (cols, None), (None, nrm), (cols, nrm)):
        path = str(tmp_path / "mesh.ply")
        IO.write_ply(path, pts, colours, normals, faces=faces)
        p, c, n, f = IO.load_ply_mesh(path)
        assert p.dtype == np.float32 and (p == pts).all() and f.dtype == np.int32 and (f == faces).all()
        assert (c is None) == (colours is None) and (c is None or (c == cols).all())
        assert (n is None) == (normals is None) and (n is None or (n == nrm).all())
        assert (IO.load_ply_points(path) == pts).all()                              # it skips the faces as before
        plain = str(tmp_path / "cloud.ply")
        IO.write_ply(plain, pts, colours, normals)
        blob, mesh_blob = open(plain, "rb").read(), open(path, "rb").read()
        head = b"ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
        if normals is not None:
            head += b"property float nx\nproperty float ny\nproperty float nz\n"
        if colours is not None:
            head += b"property uchar red\nproperty uchar green\nproperty uchar blue\n"
        body = len(blob) - len(head) - len(b"end_header\n")
        assert blob.startswith(head + b"end_header\n") and body == 7 * (12 + (12 if normals is not None else 0) + (3 if colours is not None else 0))
        assert mesh_blob.startswith(head + b"element face 5\nproperty list uchar int vertex_indices\nend_header\n")
        assert mesh_blob[-(5 * 13):] == b"".join(b"\x03" + row.astype("<i4").tobytes() for row in faces)
        assert mesh_blob[:len(head)] == blob[:len(head)] and blob[-body:] == mesh_blob[-(5 * 13) - body:-(5 * 13)]
        p, c, n, f = IO.load_ply_mesh(plain)                                          # a cloud is a mesh without faces
        assert (p == pts).all() and f.shape == (0, 3)
    IO.write_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32))
    p, c, n, f = IO.load_ply_mesh(str(tmp_path / "empty.ply"))
    assert p.shape == (0, 3) and f.shape == (0, 3)
    for bad in (np.zeros((2, 4), np.int32), np.array([[0, 1, 7]]), np.array([[0, -1, 2]])):
        with pytest.raises(Exception):
            IO.write_ply(str(tmp_path / "bad.ply"), pts, faces=bad)


# ---------------------------------------------------------------------------------------------------------------------
# 2. GPU
# ---------------------------------------------------------------------------------------------------------------------
def _volume(dev, plane_scene, dims, views=None, colour=True):
    from pointmvsnet_amd import tsdf as T
    origin, voxel, trunc, _ = plane_scene["grids"][dims]
    vol = T.TSDFVolume(origin, voxel, dims, trunc, with_colour=colour, device=dev)
    depths = torch.from_numpy(plane_scene["depths"]).to(dev)
    images = torch.from_numpy(plane_scene["images"]).to(dev)
    for chunk in (views or [slice(None)]):
        vol.integrate(depths[chunk], plane_scene["K"][chunk], plane_scene["E"][chunk], images=images[chunk] if colour else None)
    return vol


@pytest.fixture(scope="module")
def gpu_volumes(dev, plane_scene):
    return {dims: _volume(dev, plane_scene, dims) for dims in GRIDS}


@pytest.mark.gpu
@pytest.mark.parametrize("dims", GRIDS)
def test_integration_matches_the_float64_statement(dev, plane_scene, gpu_volumes, dims):
    st = plane_scene["grids"][dims][3]
    vol = gpu_volumes[dims]
    clear = ~st["ambiguous"]
    W, CW, CS = vol.weight().cpu().numpy(), vol.CW.cpu().numpy(), vol.CS.cpu().numpy()
    tsdf, colour = vol.tsdf().cpu().numpy(), vol.colour().cpu().numpy()
    assert tsdf.dtype == np.float32 and W.dtype == np.int32 and colour.dtype == np.uint8 and tsdf.shape == dims[::-1]
    ratio = (np.abs(tsdf.astype(np.float64) - st["tsdf"]) / st["bound"])[clear].max()
    print(dims, "ambiguous share", 1.0 - clear.mean(), "largest error / bound", ratio,
          "W differs on", int((W != st["W"])[clear].sum()), "CW on", int((CW != st["CW"])[clear].sum()))
    report("tsdf_integration", nx=dims[0], ambiguous_share=1.0 - clear.mean(), err_over_bound_max=ratio)
    assert (W == st["W"])[clear].all()
    assert (CW == st["CW"])[clear].all() and (CS == st["CS"])[clear].all() and (colour == st["colour"])[clear].all()
    assert ratio <= 1.0
    assert (tsdf[W == 0] == 1.0).all() and (colour[CW == 0] == 0).all()


@pytest.mark.gpu
def test_chunked_integration_is_whole_and_runs_are_identical(dev, plane_scene, gpu_volumes):
    dims = GRIDS[0]
    whole = gpu_volumes[dims]
    for other in (_volume(dev, plane_scene, dims, views=[slice(0, 3), slice(3, 5)]), _volume(dev, plane_scene, dims)):
        for name in ("S", "W", "CS", "CW"):
            a, b = getattr(whole, name).cpu().numpy(), getattr(other, name).cpu().numpy()
            assert a.tobytes() == b.tobytes(), name
    plain = _volume(dev, plane_scene, dims, colour=False)                           # without colour: the same S and W
    assert plain.CS is None and plain.colour() is None
    assert plain.S.cpu().numpy().tobytes() == whole.S.cpu().numpy().tobytes() and torch.equal(plain.W, whole.W)


@pytest.mark.gpu
def test_closed_form_constant_depth(dev):
    """One identity camera and a constant depth map D: z is the sample's own Z, so tsdf = clip((D - Z) / trunc) after two
    roundings (the subtraction, the quotient) of numbers of at most 1: within 3 eps.  A vertex interpolates a function that is
    linear in Z, so it lies on Z = D up to rounding: ``f`` carries a relative 2 eps, which moves ``t`` by at most
    4 eps |f_a| |f_b| / (|f_a| + |f_b|)^2 <= eps, i.e. the vertex by eps voxel (2 eps voxel with the second order), and the
    interpolation itself adds 6 eps (|Z_a| + |Z_b|) as everywhere."""
    from pointmvsnet_amd import tsdf as T
    h, w, f, D = 24, 40, 60.0, 8.0
    K = np.array([[[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]]])
    E = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
    dims, voxel = (27, 19, 23), 0.27
    origin = np.array([-3.4, -2.3, D - 11.3 * voxel], np.float32)
    trunc = float(np.float32(3.0 * voxel))
    vol = T.TSDFVolume(origin, voxel, dims, trunc, device=dev)
    vol.integrate(torch.full((1, h, w), D, dtype=torch.float32, device=dev), K, E)
    pos = sample_positions(origin, voxel, dims).astype(np.float64)
    g = project64(pos.reshape(-1, 3), render.world_maps(K, E))
    u, v, eu, ev = (g[n][0].reshape(dims[::-1]) for n in ("u", "v", "eps_u", "eps_v"))
    Z = pos[..., 2]
    assert (g["z"][0].reshape(dims[::-1]) == Z).all()
    inside = (u >= eu) & (u < w - eu) & (v >= ev) & (v < h - ev)
    outside = (u < -eu) | (u >= w + eu) | (v < -ev) | (v >= h + ev)
    sdf = D - Z
    band = EPS32 * np.abs(sdf)
    kept, behind = inside & (sdf > -trunc + band), sdf < -trunc - band
    tsdf, W = vol.tsdf().cpu().numpy(), vol.weight().cpu().numpy()
    assert kept.mean() > 0.1 and outside.mean() > 0.1 and (behind & inside).mean() > 0.05
    err = np.abs(tsdf - np.clip(sdf / trunc, -1.0, 1.0))[kept].max() / EPS32
    assert (W[kept] == 1).all() and (W[outside] == 0).all() and (W[behind] == 0).all() and err <= 3.0
    vertices, faces, colours, keys = vol.extract()
    assert colours is None and len(faces) > 100
    keys, vz = keys.cpu().numpy(), vertices.cpu().numpy()[:, 2].astype(np.float64)
    a = keys >> 3
    za = Z.reshape(-1)[a]
    zb = Z.reshape(-1)[a + (keys & 1) + ((keys >> 1) & 1) * dims[0] + ((keys >> 2) & 1) * dims[0] * dims[1]]
    ratio = (np.abs(vz - D) / (6 * EPS32 * (np.abs(za) + np.abs(zb)) + 2 * EPS32 * voxel)).max()
    print("closed form: tsdf error", err, "eps; vertex |z - D| / bound", ratio)
    report("tsdf_closed_form", tsdf_err_eps=err, vertex_err_over_bound=ratio)
    assert ratio <= 1.0


def _compare_extraction(dev, f, wgt, origin, voxel, min_weight, colour, tag):
    from pointmvsnet_amd import tsdf as T
    vertices, faces, colours, keys = T.extract_mesh(torch.from_numpy(f).to(dev), torch.from_numpy(wgt).to(dev), origin, voxel,
                                                    min_weight=min_weight,
                                                    colour=None if colour is None else torch.from_numpy(colour).to(dev))
    assert vertices.dtype == torch.float32 and faces.dtype == torch.int32 and keys.dtype == torch.int64
    vertices, faces, keys = vertices.cpu().numpy(), faces.cpu().numpy(), keys.cpu().numpy()
    skeys, sfaces, svertices, scolours, scale = statement_extract(f, wgt, origin, voxel, min_weight, colour)
    assert keys.shape == skeys.shape and (keys == skeys).all(), tag
    assert faces.shape == sfaces.shape and (canonical(faces) == canonical(sfaces)).all(), tag
    ratio = 0.0
    if len(keys):
        ratio = (np.abs(vertices - svertices) / (6 * EPS32 * scale + 1e-300)).max()
    if colour is None:
        assert colours is None
        level = 0.0
    else:
        colours = colours.cpu().numpy()
        assert colours.dtype == np.uint8 and colours.shape == scolours.shape
        level = np.abs(colours.astype(np.float64) - np.clip(np.floor(scolours + 0.5), 0, 255)).max() if len(keys) else 0.0
    print(tag, "vertices", len(keys), "faces", len(faces), "position error / bound", ratio, "colour levels", level)
    report("tsdf_extraction", vertices=len(keys), faces=len(faces), err_over_bound_max=ratio, colour_levels=level)
    assert ratio <= 1.0 and level <= 1.0, tag
    return vertices, faces


@pytest.mark.gpu
@pytest.mark.parametrize("dims", GRIDS)
def test_extraction_matches_the_statement_on_the_scene(dev, plane_scene, gpu_volumes, dims):
    origin, voxel, _, _ = plane_scene["grids"][dims]
    vol = gpu_volumes[dims]
    f, wgt, colour = vol.tsdf().cpu().numpy(), vol.weight().cpu().numpy(), vol.colour().cpu().numpy()
    holed = wgt.copy()
    holed[:, dims[1] // 3:dims[1] // 2, dims[0] // 4:dims[0] // 2] = 0            # inactive cells and a mesh boundary inside
    sizes = []
    for tag, w_, mw, col in (("min_weight 1", wgt, 1, colour), ("min_weight 3", wgt, 3, None), ("holed", holed, 1, colour)):
        _, faces = _compare_extraction(dev, f, w_, origin, voxel, mw, col, "%s %s" % (dims, tag))
        sizes.append(len(faces))
    assert sizes[0] > 100 and 0 < sizes[1] < sizes[0] and 0 < sizes[2] < sizes[0]
    mesh = vol.extract(min_weight=3)                                              # the method is the function on the volume's state
    assert len(mesh[1]) == sizes[1] and mesh[2] is not None


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SPHERES))
def test_extraction_on_spheres(dev, sphere_statements, name):
    n, centre, r = SPHERES[name]
    f, wgt, _ = sphere_statements[name]
    vertices, faces = _compare_extraction(dev, f, wgt, (0.0, 0.0, 0.0), 1.0, 1, None, name)
    worst, flat = check_sphere_mesh(vertices, faces, centre, r)
    assert flat == (228 if name == "on_sample_17" else 0)


@pytest.mark.gpu
def test_degenerate_volumes(dev):
    from pointmvsnet_amd import tsdf as T

    def mesh(f, wgt, **kw):
        out = T.extract_mesh(torch.as_tensor(f, dtype=torch.float32).to(dev), torch.as_tensor(wgt, dtype=torch.int32).to(dev),
                             (0.5, -1.0, 2.0), 0.25, **kw)
        assert out[0].shape[1:] == (3,) and out[1].shape[1:] == (3,) and out[0].shape[0] == out[3].shape[0]
        return out

    def empty(out):
        return out[0].shape[0] == 0 and out[1].shape[0] == 0

    ones = np.ones((5, 6, 7), np.int32)
    assert empty(mesh(np.full((5, 6, 7), 0.5), ones))                            # all outside
    assert empty(mesh(np.zeros((5, 6, 7)), ones))                                # exactly 0 is outside
    assert empty(mesh(np.full((5, 6, 7), -0.5), ones))                           # all inside
    mixed = np.where(np.arange(7)[None, None, :] < 3, -0.5, 0.5) * np.ones((5, 6, 1))
    assert not empty(mesh(mixed, ones))
    assert empty(mesh(mixed, ones * 4, min_weight=5))                            # min_weight above every W
    assert not empty(mesh(mixed, ones * 4, min_weight=4))
    assert empty(mesh(mixed[:1], ones[:1])) and empty(mesh(mixed[:, :1], ones[:, :1]))          # an axis of 1: no cells
    assert empty(mesh(mixed[:, :, :1], ones[:, :, :1])) and empty(mesh(mixed[:1, :1, :1], ones[:1, :1, :1]))
    cell = np.full((2, 2, 2), 0.5, np.float32)                                   # one cell, corner 0 inside: all six tetrahedra
    cell[0, 0, 0] = -0.5                                                         # contain it, so six triangles on seven vertices
    v, f, c, k = mesh(cell, np.ones((2, 2, 2), np.int32))
    sk, sf, sv, _, scale = statement_extract(cell, np.ones((2, 2, 2), np.int32), np.array([0.5, -1.0, 2.0], np.float32), 0.25)
    assert len(sf) == 6 and len(sk) == 7
    assert (k.cpu().numpy() == sk).all() and (canonical(f.cpu().numpy()) == canonical(sf)).all()
    assert (np.abs(v.cpu().numpy() - sv) <= 6 * EPS32 * scale).all()
    from pointmvsnet_amd import _lib                                             # keys that name no edge of the volume: (0, 0, 0)
    bogus = torch.tensor([0, 5 * 8, 7 * 8 + 7, 1 * 8 + 1, 8 * 8 + 1, -3, 2 ** 40], dtype=torch.int64).to(dev)
    field = torch.as_tensor(cell).to(dev)                                        # direction 0; an end outside; no such sample
    got = torch.full((len(bogus), 3), 9.0, device=dev)
    with _lib.on_device(field.device):
        _lib.call("pf_tsdf_vertices_f32", _lib.ptr(bogus), len(bogus), _lib.ptr(field), None, 0.5, -1.0, 2.0, 0.25, 2, 2, 2,
                  _lib.ptr(got), None, _lib.stream())
    assert (got.cpu() == 0).all()
    vol = T.TSDFVolume((0, 0, 0), 1.0, (3, 1, 2), 2.0, device=dev)               # never integrated: W == 0 everywhere
    assert empty(vol.extract()) and (vol.tsdf() == 1.0).all() and int(vol.weight().sum()) == 0


@pytest.mark.gpu
def test_scan_accumulator_mesh(dev, tmp_path):
    """``ScanAccumulator.mesh`` / ``write_mesh`` on an accumulator that is handed the plane scene's noise-free depth maps
    with full confidence (the filter keeps everything; the zero and outlier blocks are holes): the file loads, every face
    index addresses a vertex, and every vertex lies within ``trunc`` of the plane."""
    from pointmvsnet_amd import scan as S
    depths, K, E, images, cams = make_plane_scene(5, sigma=0.0)
    depths = depths.copy()
    depths[depths > 700.0] = 0.0                                                  # the outlier block becomes a hole
    nv, h, w = depths.shape
    R0, t0 = E[0][:, :3], E[0][:, 3]
    n = R0.T @ np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    c = n @ (np.linalg.inv(R0) @ (np.array([0.0, 0.0, 600.0]) - t0))
    acc = S.ScanAccumulator(nv, name="flow2", mode="NEAREST")
    with pytest.raises(ValueError, match="have not been added"):
        acc.mesh(4.0)
    prob = torch.zeros((1, 5, h, w), device=dev)
    prob[:, 2] = 1.0
    for v in range(nv):
        order = [v] + [u for u in range(nv) if u != v]
        batch = {"img_list": torch.zeros((1, nv, 3, h, w)), "cam_params_list": cams[None, order],
                 "ref_img": torch.from_numpy(images[v][None, :, :, ::-1].copy())}               # BGR, as the loader hands it
        preds = {"flow2": torch.from_numpy(depths[v])[None, None].to(dev), "flow2_prob": prob,
                 "coarse_prob_map": torch.ones((1, 1, h, w), device=dev)}
        acc.add(batch, preds, view_index=v)
    voxel = 4.0
    path = str(tmp_path / "mesh.ply")
    vertices, faces, colours = acc.write_mesh(path, voxel=voxel, min_weight=2)
    p, col, nrm, f = IO.load_ply_mesh(path)
    assert len(p) > 1000 and len(f) > 1000 and nrm is None
    assert (p == vertices.cpu().numpy()).all() and (f == faces.cpu().numpy()).all() and (col == colours.cpu().numpy()).all()
    assert f.min() >= 0 and f.max() < len(p)
    off = np.abs(p.astype(np.float64) @ n - c)
    print("ScanAccumulator.mesh:", len(p), "vertices", len(f), "faces; farthest from the plane", off.max(), "trunc", 4 * voxel)
    assert off.max() <= 4 * voxel
    again = acc.mesh(voxel, min_weight=2, with_colour=False)
    assert again[2] is None and torch.equal(again[0], vertices) and torch.equal(again[1], faces)
    lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    boxed = acc.mesh(voxel, trunc=12.0, bounds=(lo + 20.0, hi - 20.0), filtered=False)
    bp = boxed[0].cpu().numpy()
    assert len(bp) and (bp >= lo + 20.0 - 1e-3).all() and (bp <= hi - 20.0 + voxel).all()
