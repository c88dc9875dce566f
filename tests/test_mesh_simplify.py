"""Mesh simplification (pointmvsnet_amd/mesh_simplify.py, csrc/mesh_simplify.hip) against a NumPy statement of its
specification, and the layer above: ``ScanAccumulator.mesh(simplify_cell=...)``.

The specification is the module's docstring and the yardstick is ``statement_simplify`` below, written from that text with
no code shared with the product: clusters and colours from a float32 / integer statement, faces from a Python loop, the
placement in float64 with the sums in ascending corner order (``np.add.at`` adds in the order of its index array).

Integers are equal
------------------
``vertex_map``, the faces, ``face_source``, the colours and every entry of ``report`` equal the statement's, and so do the
``"mean"`` positions bit for bit: the float64 sum in ascending vertex index, one quotient and one rounding to float32 are
``voxel_downsample``'s rule, which NumPy reproduces exactly.

The bound on ``"quadric"`` positions (``statement_simplify``: ``bound``)
-----------------------------------------------------------------------
u = 2^-53.  The kernel and the statement evaluate the same float64 expression per corner (conversions, differences,
products: IEEE operations, no contraction on either side), so the *terms* of the nine sums are the same numbers; what may
differ is the order in which a cluster's N terms are added (ascending for the statement and for a short list, lanes and a
butterfly for a long one, and any order once the faces are permuted).  A sum of N numbers in any order is within
``(N - 1) u / (1 - (N - 1) u) <= N u`` times the sum of their absolute values of the exact sum, so two orders differ by at
most ``dA = 2 N u sum|n_i n_j|`` and ``db = 2 N u sum|d n_i|`` entrywise; the statement accumulates these absolute sums next
to the sums themselves.  ``lam = reg t / 3`` inherits ``reg / 3 (dA00 + dA11 + dA22)``; with it ``dM = dA + dlam I``.

The solve.  To first order ``x + dx`` of ``(M + dM)(x + dx) = -(b + db)`` has ``|dx| <= |M^-1| (db + dM |x|)`` entrywise.
The arithmetic of forming and solving adds, per side: ``t`` and ``lam`` four roundings (a perturbation of at most
``4 u lam <= 4 u |M|_2``), the diagonal one (``u |M|_2``), and the factorisation with its two substitutions a backward error
``|DM| <= gamma_(3n+1) |L||D||L^T|`` whose 2-norm is at most ``n gamma_(3n+1) |M|_2 = 30 u |M|_2`` for n = 3 (Higham, Accuracy
and Stability of Numerical Algorithms, theorem 10.4 and lemma 10.6, which hold for the root-free form alike).  A
perturbation of 2-norm ``e |M|_2`` moves ``x`` by at most ``e cond(M) |x|_2`` to first order, and ``cond(M) <= 3 / reg + 1``
because ``lam <= eig(M) <= t + lam``.  Two sides: ``70 u (3 / reg + 1) |x|_2`` per coordinate.  Last, ``v = float32(m + x)``:
the float64 sum is one rounding (``u |v|``) per side and rounding two float64 numbers ``delta`` apart to float32 gives
numbers at most ``delta + 2^-24 |v|`` apart.  The bound is the sum of these terms, per cluster and coordinate; nothing is
tuned.  It is dominated by ``2^-24 |v|``: the positions must agree to within about one unit in the last place.

The fallback decision may differ from the statement's only in a cluster where ``| max_k |x_k| - cell |`` is within that
bound of zero.  The statement has no such cluster on any fixture here (asserted first), so the cap is zero and
``report["fallback"]`` must be equal.

Measured on an MI355X, and the same on tests/hipemu (the kernel sources compiled for the host): in all nine cases every
integer is equal and no position coordinate differs from the statement's at all (0 of 8 136; share of the bound used 0),
with 20 of 20 clusters on the wave path at cell 8 and 1 045 of 1 578 on the thread path at cell 0.75, and none differs under a
permutation of the faces either: the float64 sums' last bits do not survive the rounding to float32 here.  Over all
mapped input vertices (``point_mesh_distances`` of every one of them) the farthest is 0.47 cells from the simplified surface
(the roof, both placements; 0.06 to 0.19 cells on the spheres); the limit is 3.46.  ``conftest.report`` carries
the figures (``mesh_simplify``, ``mesh_simplify_distance``).
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_fusion import make_plane_scene
from test_mesh_ops import plane_mesh
from test_tsdf import SPHERES, sphere_volume, statement_extract

U = 2.0 ** -53
EPS32 = 2.0 ** -24
SPHERE_CELLS = (1.5, 2.0, 3.0, 4.0)


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def cell_keys(v32, cell, origin=None):
    """``(cx << 42 | cy << 21 | cz, cells (N, 3))`` by the float32 rule of the text."""
    v32 = np.asarray(v32, np.float32)
    inv = np.float32(1.0) / np.float32(cell)
    o = v32.min(axis=0) if origin is None else np.asarray(origin, np.float32)
    scaled = (v32 - o) * inv
    assert scaled.dtype == np.float32
    c = np.floor(scaled).astype(np.int64)
    assert c.min() >= 0 and c.max() < (1 << 17)
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2], c


def solve_ldl(A, b, reg):
    """The solve of the text on Python floats (IEEE float64): ``(x, M)`` or ``(None, None)`` when the trace is no use."""
    a00, a01, a02, a11, a12, a22 = (float(t) for t in A)
    b0, b1, b2 = (float(t) for t in b)
    t = (a00 + a11) + a22
    if not (np.isfinite(t) and t > 0.0):
        return None, None
    lam = (reg * t) / 3.0
    m00, m11, m22 = a00 + lam, a11 + lam, a22 + lam
    l10 = a01 / m00
    l20 = a02 / m00
    d1 = m11 - l10 * a01
    u21 = a12 - l20 * a01
    l21 = u21 / d1
    d2 = m22 - (l20 * a02 + l21 * u21)
    y0 = -b0
    y1 = -b1 - l10 * y0
    y2 = -b2 - (l20 * y0 + l21 * y1)
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = y0 / m00 - (l10 * x1 + l20 * x2)
    return np.array([x0, x1, x2]), np.array([[m00, a01, a02], [a01, m11, a12], [a02, a12, m22]])


def statement_simplify(vertices, faces, cell, colours=None, placement="quadric", reg=1e-3, origin=None):
    """The module docstring in NumPy.  Returns a dict: ``vertices`` (float32), ``faces``, ``colours``, ``vertex_map``,
    ``face_source``, ``report``, ``keys`` (per output vertex), and for ``"quadric"`` per OUTPUT vertex ``bound`` (Mv, 3),
    ``x`` (Mv, 3; nan where the trace was no use), ``margin`` = | max|x_k| - cell | (inf there), ``fell``, ``cond``,
    ``corners`` (the list lengths)."""
    v32 = np.ascontiguousarray(vertices, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    Nv, Nf = len(v32), len(faces)
    empty_report = {"vertices_in": Nv, "faces_in": Nf, "vertices_out": 0, "faces_out": 0, "clusters": 0, "collapsed": Nf,
                    "duplicates": 0, "fallback": 0, "unreferenced_clusters": 0}
    if Nv == 0:
        return {"vertices": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.int64), "colours": colours,
                "vertex_map": np.zeros((0,), np.int64), "face_source": np.zeros((0,), np.int64), "report": empty_report}
    key, _ = cell_keys(v32, cell, origin)
    uniq, C, counts = np.unique(key, return_inverse=True, return_counts=True)
    C = C.reshape(-1)
    M = len(uniq)
    total = np.zeros((M, 3))
    np.add.at(total, C, v32.astype(np.float64))                             # ascending vertex index inside a cluster
    mean = (total / counts[:, None]).astype(np.float32)
    cluster_colours = None
    if colours is not None:
        s = np.zeros((M, 3), np.int64)
        np.add.at(s, C, np.asarray(colours).astype(np.int64))
        cluster_colours = ((2 * s + counts[:, None]) // (2 * counts[:, None])).astype(np.uint8)
    # faces: a Python loop
    seen, kept, source, collapsed, duplicates = set(), [], [], 0, 0
    for f in range(Nf):
        t = (int(C[faces[f, 0]]), int(C[faces[f, 1]]), int(C[faces[f, 2]]))
        if t[0] == t[1] or t[1] == t[2] or t[0] == t[2]:
            collapsed += 1
            continue
        unordered = tuple(sorted(t))
        if unordered in seen:
            duplicates += 1
            continue
        seen.add(unordered)
        kept.append(t)
        source.append(f)
    kept = np.asarray(kept, np.int64).reshape(-1, 3)
    used = np.zeros(M, bool)
    used[kept.reshape(-1)] = True
    cluster_map = np.where(used, np.cumsum(used) - 1, -1)
    out = {"faces": cluster_map[kept], "face_source": np.asarray(source, np.int64), "vertex_map": cluster_map[C],
           "colours": None if cluster_colours is None else cluster_colours[used], "keys": uniq[used]}
    fell = np.zeros(M, bool)
    position = mean.copy()
    if placement == "quadric":
        m64 = mean.astype(np.float64)
        corner_cluster = C[faces.reshape(-1)]                                   # corner 3 f + j, ascending
        face_of = np.repeat(np.arange(Nf), 3)
        mm = m64[corner_cluster]
        pa, pb, pc = (v32[faces[face_of, j]].astype(np.float64) - mm for j in range(3))
        e1, e2 = pb - pa, pc - pa
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        good = np.isfinite(n).all(axis=1)
        d = -((n[:, 0] * pa[:, 0] + n[:, 1] * pa[:, 1]) + n[:, 2] * pa[:, 2])
        terms = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2],
                          n[:, 2] * n[:, 2], d * n[:, 0], d * n[:, 1], d * n[:, 2]], axis=1)[good]
        sums, sums_abs = np.zeros((M, 9)), np.zeros((M, 9))
        np.add.at(sums, corner_cluster[good], terms)                            # ascending corner order
        np.add.at(sums_abs, corner_cluster[good], np.abs(terms))
        N = np.bincount(corner_cluster[good], minlength=M)
        bound = np.zeros((M, 3))
        xs = np.full((M, 3), np.nan)
        margin = np.full(M, np.inf)
        cond = np.ones(M)
        limit = float(np.float32(cell))
        for s in range(M):
            x, Mat = solve_ldl(sums[s, :6], sums[s, 6:], reg)
            if x is None:
                continue
            xs[s] = x
            dA6, db = 2.0 * N[s] * U * sums_abs[s, :6], 2.0 * N[s] * U * sums_abs[s, 6:]
            dM = np.array([[dA6[0], dA6[1], dA6[2]], [dA6[1], dA6[3], dA6[4]], [dA6[2], dA6[4], dA6[5]]])
            dM = dM + np.eye(3) * (reg / 3.0 * (dA6[0] + dA6[3] + dA6[5]))
            first_order = np.abs(np.linalg.inv(Mat)) @ (db + dM @ np.abs(x))
            solve = 70.0 * U * (3.0 / reg + 1.0) * float(np.sqrt((x * x).sum()))
            cond[s] = np.linalg.cond(Mat)
            assert cond[s] <= (3.0 / reg + 1.0) * (1.0 + 1e-9)
            fell[s] = not bool((np.abs(x) <= limit).all())
            v = m64[s] + (0.0 if fell[s] else x)
            bound[s] = first_order + solve + (2.0 * U + EPS32) * np.abs(v)
            margin[s] = abs(float(np.abs(x).max()) - limit)
            if not fell[s]:
                position[s] = v.astype(np.float32)
        out.update(bound=bound[used], x=xs[used], margin=margin[used], fell=fell[used], cond=cond[used],
                   corners=np.bincount(corner_cluster, minlength=M)[used],
                   bound_decides=(margin[used] <= bound[used].max(axis=1)))
    out["vertices"] = position[used]
    out["report"] = {"vertices_in": Nv, "faces_in": Nf, "vertices_out": int(used.sum()), "faces_out": len(kept), "clusters": M,
                     "collapsed": collapsed, "duplicates": duplicates, "fallback": int((fell & used).sum()),
                     "unreferenced_clusters": int(M - used.sum())}
    return out


def edge_counts_numpy(faces):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    count = {}
    for a, b, c in faces:
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                e = (min(p, q), max(p, q))
                count[e] = count.get(e, 0) + 1
    v = np.asarray(list(count.values()), np.int64)
    return {"boundary": int((v == 1).sum()), "manifold": int((v == 2).sum()), "nonmanifold": int((v > 2).sum())}


def is_closed_manifold_of_euler_2(faces, nv):
    """Every undirected edge has exactly two faces, every vertex is used and V - E + F = 2.  (Orientation is not asked: the
    survivor of a set of duplicates keeps its own winding, which may be the mirrored one.)"""
    faces = np.asarray(faces, np.int64)
    edges = edge_counts_numpy(faces)
    return (edges["boundary"] == 0 and edges["nonmanifold"] == 0 and len(np.unique(faces)) == nv
            and nv - edges["manifold"] + len(faces) == 2)


# ---------------------------------------------------------------------------------------------------------------------
# the fixtures
# ---------------------------------------------------------------------------------------------------------------------
def sphere_mesh(name):
    n, centre, r = SPHERES[name]
    f, wgt = sphere_volume(n, centre, r)
    _, faces, vertices, _, _ = statement_extract(f, wgt, (0.0, 0.0, 0.0), 1.0)
    return vertices.astype(np.float32), faces.astype(np.int64)


def sheet(xy, z):
    """The two triangles of every quad of an (n, n) grid of points ``xy`` (n, n, 2) lifted to ``z(x, y)``."""
    n = xy.shape[0]
    v = np.concatenate([xy.reshape(-1, 2), z(xy[..., 0], xy[..., 1]).reshape(-1, 1)], axis=1)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a, b, c, d = (i * n + j).ravel(), ((i + 1) * n + j).ravel(), ((i + 1) * n + j + 1).ravel(), (i * n + j + 1).ravel()
    return v, np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])


def jittered_grid(n, pitch, first, amplitude, seed):
    rng = np.random.default_rng(seed)
    g = first + pitch * np.arange(n)
    return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1) + rng.uniform(-amplitude, amplitude, (n, n, 2))


def two_sheets():
    """``z = 0.2`` and ``z = 0.7 + 0.05 x`` over [0, 4.3]^2 on a jittered 9 x 9 grid of pitch 0.5: both sheets share every
    cell of edge 1 (origin 0), so every cluster's quadric has two nearly parallel planes and its minimiser runs away."""
    xy = jittered_grid(9, 0.5, 0.15, 0.1, seed=21)
    v0, f0 = sheet(xy, lambda x, y: 0.2 + 0.0 * x)
    v1, f1 = sheet(xy, lambda x, y: 0.7 + 0.05 * x)
    return np.concatenate([v0, v1]).astype(np.float32), np.concatenate([f0, f1 + len(v0)]).astype(np.int64)


def roof_z(x, y):
    return 3.0 - 0.8 * np.abs(x - 2.3)


def roof():
    """``z = 3 - 0.8 |x - 2.3|`` on a jittered 10 x 10 grid: a crease inside a column of cells of edge 1."""
    xy = jittered_grid(10, 0.5, 0.05, 0.1, seed=22)
    v, f = sheet(xy, roof_z)
    return v.astype(np.float32), f.astype(np.int64)


def roof_distance(p):
    """Distance of points from the roof's surface: two half planes that leave the crease ``(x, z) = (2.3, 3)`` along
    ``(+-1, -0.8)``.  Per half plane: the distance to its plane where the foot lies on it, else the distance to the crease."""
    p = np.asarray(p, np.float64)
    qx, qz = p[:, 0] - 2.3, p[:, 2] - 3.0
    s = np.sqrt(1.0 + 0.64)
    out = np.full(len(p), np.inf)
    for side in (1.0, -1.0):
        along = (side * qx - 0.8 * qz) / s
        across = np.abs(0.8 * side * qx + qz) / s
        out = np.minimum(out, np.where(along >= 0.0, across, np.sqrt(qx * qx + qz * qz)))
    return out


# (name, cell, origin): every case that the GPU tests compare with the statement
CASES = [("off_lattice_24", c, None) for c in (0.75, 1.5, 2.0, 3.0, 8.0)] + [("on_sample_17", 2.0, None), ("plane", None, None),
                                                                        ("two_sheets", 1.0, (0.0, 0.0, 0.0)),
                                                                        ("roof", 1.0, None)]


@pytest.fixture(scope="module")
def inputs():
    out = {name: sphere_mesh(name) + (None,) for name in SPHERES}
    out["plane"] = plane_mesh()
    out["two_sheets"] = two_sheets() + (None,)
    out["roof"] = roof() + (None,)
    return out


def plane_cell(vertices):
    """Three voxels of the plane scene's grid: the cell that a user of a TSDF mesh would take."""
    extent = float((vertices.max(axis=0) - vertices.min(axis=0)).max())
    return float(np.float32(extent / 20.0 * 3.0))


@pytest.fixture(scope="module")
def statements(inputs):
    """Per (name, cell, placement) the statement, computed once and never changed."""
    out = {}
    for name, cell, origin in CASES:
        v, f, col = inputs[name]
        cell = plane_cell(v) if cell is None else cell
        for placement in ("quadric", "mean"):
            out[(name, cell, placement)] = statement_simplify(v, f, cell, col, placement, origin=origin)
    return out


def case_cell(inputs, name, cell):
    return plane_cell(inputs[name][0]) if cell is None else cell


# ---------------------------------------------------------------------------------------------------------------------
# 1. CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_a_device_is_needed():
    from pointmvsnet_amd import mesh_simplify as MS
    from pointmvsnet_amd import scan as S
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 2.0]])
    f = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    for bad in (f.float(), f[:, :2], f[0], None, f.to(torch.int16)):
        with pytest.raises(ValueError, match="faces must be"):
            MS.simplify_mesh(v, bad, 1.0)
    for bad in (v.double(), v[:, :2], v[0], None):
        with pytest.raises(ValueError, match="vertices must be"):
            MS.simplify_mesh(bad, f, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x", None, 1e-46):
        with pytest.raises(ValueError, match="cell"):
            MS.simplify_mesh(v, f, bad)
    for bad in ("median", None, 3):
        with pytest.raises(ValueError, match="placement"):
            MS.simplify_mesh(v, f, 1.0, placement=bad)
    for bad in (0.0, 9e-7, 1.0001, -1e-3, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="regularisation"):
            MS.simplify_mesh(v, f, 1.0, regularisation=bad)
    for bad in ((0.0, 0.0), (0.0, 0.0, float("nan")), "abc", (0.0, 0.0, 0.0, 0.0)):
        with pytest.raises(ValueError, match="origin must be three"):
            MS.simplify_mesh(v, f, 1.0, origin=bad)
    for bad in ((0.5, 0.0, 0.0), (-1.0, -1.0, 1e-6)):
        with pytest.raises(ValueError, match="origin must be <="):
            MS.simplify_mesh(v, f, 1.0, origin=bad)
    with pytest.raises(ValueError, match="more than 131072 voxels on an axis"):
        MS.simplify_mesh(v, f, 1e-5)
    with pytest.raises(ValueError, match="more than 131072 voxels on an axis"):
        MS.simplify_mesh(v, f, 1.0, origin=(-2e5, 0.0, 0.0))
    for bad in (float("nan"), float("inf")):
        w = v.clone()
        w[3, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            MS.simplify_mesh(w, f[:1], 1.0)                                  # even where no face names the vertex
    for bad in (torch.zeros((3, 3), dtype=torch.uint8), torch.zeros((4, 3)), np.zeros((4, 3), np.uint8)):
        with pytest.raises(ValueError, match="colours must be"):
            MS.simplify_mesh(v, f, 1.0, colours=bad)
    for kw in ({}, {"placement": "mean"}, {"origin": (-1.0, 0.0, -0.5)}, {"colours": torch.zeros((4, 3), dtype=torch.uint8)},
               {"regularisation": 1e-6}, {"regularisation": 1}):
        with pytest.raises(RuntimeError, match="no CPU path"):               # well-formed: only the device is missing
            MS.simplify_mesh(v, f, 1.0, **kw)
    with pytest.raises(ValueError, match="faces must be"):
        MS.mesh_edge_counts(f.float())
    acc = S.ScanAccumulator(2)
    assert acc.last_simplify_report is None
    for kw, what in (({"simplify_cell": -1.0}, "cell"), ({"simplify_cell": float("nan")}, "cell"),
                     ({"simplify_cell": 1.0, "simplify_placement": "median"}, "placement"),
                     ({"simplify_placement": "median"}, "placement")):
        with pytest.raises(ValueError, match=what):
            acc.mesh(1.0, **kw)
    with pytest.raises(ValueError, match="have not been added"):
        acc.mesh(1.0, simplify_cell=2.0, simplify_placement="mean")


def test_kernels_are_built_and_bound(lib_built):
    import json
    import subprocess
    from pointmvsnet_amd import _lib, build
    names = ["pf_mesh_simplify_faces", "pf_mesh_simplify_keep_first", "pf_mesh_quadric_thread_f64", "pf_mesh_quadric_wave_f64"]
    assert "mesh_simplify.hip" in build.SOURCES
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib_built]).decode()
    lib = _lib.load()
    for name in names:
        assert name in _lib.PROTOTYPES and (" T %s\n" % name) in exported and getattr(lib, name) is not None
    assert lib.pf_mesh_simplify_faces(None, -1, 4, None, 2, None, None, None, None) == -1     # sizes are checked first
    assert lib.pf_mesh_simplify_faces(None, 2, 4, None, 5, None, None, None, None) == -1      # more clusters than vertices
    assert lib.pf_mesh_simplify_faces(None, 0, 0, None, 0, None, None, None, None) == 0
    assert lib.pf_mesh_simplify_keep_first(None, 3, None, 4, None, None) == -1
    assert lib.pf_mesh_quadric_thread_f64(None, 4, None, 2, None, None, None, 2, 1.0, 1e-7, 128, None, None, None) == -1
    assert lib.pf_mesh_quadric_thread_f64(None, 4, None, 2, None, None, None, 2, 0.0, 1e-3, 128, None, None, None) == -1
    assert lib.pf_mesh_quadric_wave_f64(None, 4, None, 2, None, None, None, 2, 1.0, 1e-3, None, 3, None, None, None) == -1
    assert lib.pf_mesh_quadric_wave_f64(None, 4, None, 2, None, None, None, 2, 1.0, 1e-3, None, 0, None, None, None) == 0
    with open(build.USAGE_FILE) as fh:
        usage = json.load(fh)["mesh_simplify.hip"]
    mine = {k: u for k, u in usage.items() if "mesh_" in k}
    assert len(mine) == 4 and all(u["scratch_bytes_per_lane"] == 0 and u["static_lds_bytes"] == 0 for u in mine.values())


def test_statement_meets_the_facts_of_the_fixtures(inputs, statements):
    """The shapes and counts that the fixtures were chosen for, on the statement alone."""
    from pointmvsnet_amd import mesh_simplify as MS
    v, f, _ = inputs["off_lattice_24"]
    assert v.shape == (3832, 3) and f.shape == (7660, 3)
    for cell, clusters, duplicates, largest in ((1.5, 483, 12, 0.42), (2.0, 290, 5, 0.41), (3.0, 130, 2, 0.56)):
        st = statements[("off_lattice_24", cell, "quadric")]
        rep = st["report"]
        assert (rep["clusters"], rep["duplicates"], rep["fallback"]) == (clusters, duplicates, 0), rep
        assert rep["collapsed"] + rep["duplicates"] + rep["faces_out"] == 7660
        assert round(float(np.nanmax(np.abs(st["x"]))), 2) == largest and st["cond"].max() <= 2980.0
        assert (st["margin"] >= 0.4 * cell).all()
    for cell in (3.0, 4.0):
        st = statement_simplify(v, f, cell) if cell == 4.0 else statements[("off_lattice_24", 3.0, "quadric")]
        assert is_closed_manifold_of_euler_2(st["faces"], len(st["vertices"]))
        assert edge_counts_numpy(st["faces"]) == {"boundary": 0, "manifold": 3 * len(st["faces"]) // 2, "nonmanifold": 0}
    st = statements[("off_lattice_24", 8.0, "quadric")]
    assert 8 <= st["report"]["clusters"] <= 27 and (st["corners"] >= 2000).sum() >= 8
    assert st["corners"].min() >= MS.WAVE_MIN_CORNERS                                               # the wave path alone
    short = statements[("off_lattice_24", 0.75, "quadric")]["corners"] < MS.WAVE_MIN_CORNERS        # two in three: the thread path
    assert short.sum() > 0.5 * len(short) and (~short).sum() >= 10
    mixed = statements[("off_lattice_24", 2.0, "quadric")]["corners"]                               # both, either side of it
    assert (mixed == MS.WAVE_MIN_CORNERS).any() or ((mixed < MS.WAVE_MIN_CORNERS).any() and (mixed > MS.WAVE_MIN_CORNERS).any())
    v, f, _ = inputs["on_sample_17"]
    assert v.shape == (1298, 3) and f.shape == (2592, 3)
    p0, p1, p2 = (v[f[:, c]].astype(np.float64) for c in range(3))
    assert (np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1) == 0).sum() == 228
    st = statements[("on_sample_17", 2.0, "quadric")]
    assert st["report"]["clusters"] == 101 and st["report"]["unreferenced_clusters"] == 3
    assert is_closed_manifold_of_euler_2(st["faces"], len(st["vertices"]))
    v, f, col = inputs["plane"]
    assert f.shape == (2568, 3) and col is not None and col.shape == (len(v), 3)
    st = statements[("plane", plane_cell(v), "quadric")]
    assert edge_counts_numpy(st["faces"])["boundary"] > 0 and st["report"]["faces_out"] > 50 and st["colours"] is not None
    v, f, _ = inputs["two_sheets"]
    assert v.shape == (162, 3) and f.shape == (256, 3)
    assert v[:, :2].min() >= 0.0 and v[:, :2].max() <= 4.3
    rep = statements[("two_sheets", 1.0, "quadric")]["report"]
    assert rep == {"vertices_in": 162, "faces_in": 256, "vertices_out": 25, "faces_out": 32, "clusters": 25, "collapsed": 192,
                   "duplicates": 32, "fallback": 25, "unreferenced_clusters": 0}
    v, f, _ = inputs["roof"]
    q, m = statements[("roof", 1.0, "quadric")], statements[("roof", 1.0, "mean")]
    assert q["report"]["fallback"] == 0 and q["report"]["faces_out"] > 0
    dq, dm = roof_distance(q["vertices"]).mean(), roof_distance(m["vertices"]).mean()
    print("roof: mean distance from the surface, quadric %.4f, mean %.4f" % (dq, dm))
    assert dq < dm
    # no fixture has a cluster whose fallback decision the bound could flip: the cap on differing decisions is zero
    for key, st in statements.items():
        if key[2] == "quadric":
            assert not st["bound_decides"].any(), key
            print(key, "smallest | max|x| - cell | = %.3f cells" % (st["margin"].min() / key[1]))
            moved = np.abs(st["vertices"].astype(np.float64) - statements[key[:2] + ("mean",)]["vertices"])
            assert (moved <= float(np.float32(key[1])) + EPS32 * np.abs(st["vertices"])).all()


@pytest.mark.parametrize("name", sorted(SPHERES))
def test_quadric_placement_is_nearer_the_sphere_than_the_mean(inputs, name):
    n, centre, r = SPHERES[name]
    v, f, _ = inputs[name]
    for cell in SPHERE_CELLS:
        err = {}
        for placement in ("quadric", "mean"):
            st = statement_simplify(v, f, cell, placement=placement)
            err[placement] = np.abs(np.linalg.norm(st["vertices"].astype(np.float64) - np.asarray(centre), axis=1) - r).mean()
        print("%s cell %.1f: mean | |v - c| - r |  quadric %.4f  mean %.4f" % (name, cell, err["quadric"], err["mean"]))
        assert err["quadric"] < err["mean"]


def test_edge_counts_match_a_numpy_count(inputs):
    from pointmvsnet_amd import mesh_simplify as MS
    rng = np.random.default_rng(4)
    fan = np.stack([np.zeros(5, np.int64), 1 + np.arange(5), 1 + (np.arange(5) + 1) % 5], axis=1)
    cases = [inputs["on_sample_17"][1], inputs["plane"][1], fan, np.concatenate([fan, fan[:2], [[0, 1, 9], [3, 3, 4]]]),
             rng.integers(0, 30, (200, 3)), np.zeros((0, 3), np.int64)]
    for faces in cases:
        want = edge_counts_numpy(faces)
        assert MS.mesh_edge_counts(torch.from_numpy(np.asarray(faces, np.int64))) == want
        assert MS.mesh_edge_counts(torch.from_numpy(np.asarray(faces, np.int32))) == want
    assert edge_counts_numpy(cases[0]) == {"boundary": 0, "manifold": 3 * len(cases[0]) // 2, "nonmanifold": 0}
    assert edge_counts_numpy(cases[3])["nonmanifold"] > 0 and edge_counts_numpy(cases[2])["boundary"] == 5


# ---------------------------------------------------------------------------------------------------------------------
# 2. GPU
# ---------------------------------------------------------------------------------------------------------------------
def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _run(dev, v, f, cell, col=None, faces_dtype=None, **kw):
    from pointmvsnet_amd import mesh_simplify as MS
    out = MS.simplify_mesh(_t(v, dev), _t(f, dev, faces_dtype), cell, colours=None if col is None else _t(col, dev),
                           return_maps=True, **kw)
    assert len(out) == 6
    return out


def _check_integers(got, st, tag):
    vertices, faces, colours, rep, vertex_map, face_source = got
    assert rep == st["report"], (tag, rep, st["report"])
    assert all(type(x) is int for x in rep.values())
    assert vertices.dtype == torch.float32 and vertices.shape == (rep["vertices_out"], 3)
    assert vertex_map.dtype == torch.int64 and face_source.dtype == torch.int64
    assert (vertex_map.cpu().numpy() == st["vertex_map"]).all(), tag
    assert (faces.cpu().numpy() == st["faces"]).all() and (face_source.cpu().numpy() == st["face_source"]).all(), tag
    if st["colours"] is None:
        assert colours is None
    else:
        assert colours.dtype == torch.uint8 and (colours.cpu().numpy() == st["colours"]).all(), tag


def _check_positions(vertices, st, tag):
    """``"quadric"`` positions against the statement's, per coordinate within its bound; returns (share, differing)."""
    got, want = vertices.cpu().numpy().astype(np.float64), st["vertices"].astype(np.float64)
    diff = np.abs(got - want)
    share = float(np.divide(diff, st["bound"], out=np.zeros_like(diff), where=st["bound"] > 0).max()) if diff.size else 0.0
    differing = int((diff > 0).sum())
    print("%s: largest |difference| / bound %.3f, %d of %d coordinates differ" % (tag, share, differing, diff.size))
    assert (diff <= st["bound"]).all(), (tag, share)
    return share, differing


@pytest.mark.gpu
@pytest.mark.parametrize("name,cell,origin", CASES)
def test_simplify_matches_the_statement(dev, inputs, statements, name, cell, origin):
    """Integers equal, ``"mean"`` bit for bit, ``"quadric"`` within the bound (module docstring); two runs identical.  Cell
    8 of the larger sphere takes the wave path alone, cell 0.75 the thread path for two clusters in three, the others both."""
    from pointmvsnet_amd import mesh_simplify as MS
    v, f, col = inputs[name]
    cell = case_cell(inputs, name, cell)
    tag = "%s cell %.3g" % (name, cell)
    st = statements[(name, cell, "mean")]
    got = _run(dev, v, f, cell, col, placement="mean", origin=origin)
    _check_integers(got, st, tag)
    assert (got[0].cpu().numpy().view(np.uint32) == st["vertices"].view(np.uint32)).all(), tag
    st = statements[(name, cell, "quadric")]
    assert not st["bound_decides"].any()
    got = _run(dev, v, f, cell, col, origin=origin)
    _check_integers(got, st, tag)
    share, differing = _check_positions(got[0], st, tag)
    again = _run(dev, v, f, cell, col, origin=origin)
    assert all(torch.equal(a, b) for a, b in zip(got[:2] + got[4:], again[:2] + again[4:])) and again[3] == got[3]
    long_lists = int((st["corners"] >= MS.WAVE_MIN_CORNERS).sum())
    if name == "off_lattice_24" and cell in (0.75, 8.0):
        assert long_lists == len(st["corners"]) if cell == 8.0 else 10 <= long_lists < 0.5 * len(st["corners"])
    edges = MS.mesh_edge_counts(got[1])
    assert edges == edge_counts_numpy(st["faces"])
    report("mesh_simplify", cell=cell, clusters=st["report"]["clusters"], faces_out=st["report"]["faces_out"],
           bound_share=share, coordinates_differing=differing, coordinates=3 * len(st["vertices"]),
           wave_clusters=long_lists, nonmanifold_edges=edges["nonmanifold"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,cell", [("off_lattice_24", 1.5), ("off_lattice_24", 4.0), ("on_sample_17", 2.0), ("roof", 1.0)])
def test_input_vertices_stay_within_two_root_three_cells(dev, inputs, name, cell):
    """An output vertex is within ``cell`` per axis of its cluster's mean, which lies in the cluster's cell with all its
    members: every input vertex that is mapped is within ``2 sqrt(3) cell`` of the simplified surface."""
    from pointmvsnet_amd.mesh_distance import point_mesh_distances
    v, f, _ = inputs[name]
    limit = 2.0 * np.sqrt(3.0) * cell * (1.0 + 2.0 ** -20)
    for placement in ("quadric", "mean"):
        vertices, faces, _, rep, vertex_map, _ = _run(dev, v, f, cell, placement=placement)
        assert rep["faces_out"] > 0
        mapped = torch.nonzero(vertex_map >= 0).view(-1)
        dist = point_mesh_distances(_t(v, dev)[mapped], vertices, faces, max_dist=4.0 * limit)
        assert dist.shape == (mapped.numel(),) and mapped.numel() > 0.9 * len(v)
        worst = float(dist.max())
        print("%s cell %.1f %s: farthest mapped input vertex %.3f cells (limit %.3f)" % (name, cell, placement, worst / cell,
                                                                                        limit / cell))
        assert worst <= limit
        report("mesh_simplify_distance", cell=cell, worst_in_cells=worst / cell, mean_in_cells=float(dist.mean()) / cell)


@pytest.mark.gpu
def test_permutations_of_faces_and_vertices(dev, inputs, statements):
    v, f, _ = inputs["off_lattice_24"]
    rng = np.random.default_rng(8)
    for cell in (2.0, 8.0):
        st = statements[("off_lattice_24", cell, "quadric")]
        key_of = st["keys"]
        want_faces = {frozenset(key_of[row].tolist()) for row in st["faces"]}
        assert len(want_faces) == len(st["faces"])
        perm = rng.permutation(len(f))
        vertices, faces, _, rep, vertex_map, _ = _run(dev, v, f[perm], cell)
        assert (vertex_map.cpu().numpy() == st["vertex_map"]).all()                       # the same clusters
        assert {frozenset(key_of[row].tolist()) for row in faces.cpu().numpy()} == want_faces
        assert rep == st["report"]
        _check_positions(vertices, st, "faces permuted, cell %.1f" % cell)
        perm = rng.permutation(len(v))
        inverse = np.argsort(perm)
        vertices, faces, _, rep, vertex_map, _ = _run(dev, v[perm], inverse[f], cell, placement="mean")
        keys = cell_keys(v[perm], cell)[0]
        vm = vertex_map.cpu().numpy()
        rows = np.full(rep["vertices_out"], -1, np.int64)
        rows[vm[vm >= 0]] = keys[vm >= 0]
        assert (keys[vm >= 0] == rows[vm[vm >= 0]]).all() and (rows == key_of).all()       # one key per row, ascending
        assert {frozenset(rows[row].tolist()) for row in faces.cpu().numpy()} == want_faces


@pytest.mark.gpu
def test_edge_cases(dev):
    from pointmvsnet_amd import mesh_simplify as MS
    v = np.array([[0.1, 0.1, 0.1], [0.4, 0.1, 0.2], [0.1, 0.4, 0.3], [2.5, 0.2, 0.1], [0.2, 2.5, 0.1], [2.6, 2.4, 1.5]], np.float32)
    none = np.zeros((0, 3), np.int64)

    def check(v_, f_, cell, **kw):
        st = statement_simplify(v_, f_, cell, placement=kw.get("placement", "quadric"), origin=kw.get("origin"))
        got = _run(dev, v_, f_, cell, **kw)
        _check_integers(got, st, "edge case")
        assert got[1].dtype == (kw.get("faces_dtype") or torch.int64)
        if kw.get("placement") == "mean" or not len(st["vertices"]):
            assert (got[0].cpu().numpy() == st["vertices"]).all()
        else:
            _check_positions(got[0], st, "edge case")
        return got, st

    got, _ = check(v, none, 1.0)                                                         # Nf == 0
    assert got[3]["clusters"] == 4 and got[3]["unreferenced_clusters"] == 4 and (got[4] == -1).all() and got[0].shape == (0, 3)
    got, _ = check(np.zeros((0, 3), np.float32), none, 1.0)                              # Nv == 0
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[4].shape == (0,) and got[5].shape == (0,)
    got, _ = check(v, np.array([[0, 1, 2]]), 1.0)                                        # one triangle inside one cell
    assert got[3]["collapsed"] == 1 and got[1].shape == (0, 3) and got[0].shape == (0, 3)
    got, _ = check(v, np.array([[0, 3, 4], [3, 5, 4], [1, 3, 4]]), 100.0)                # a cell larger than the mesh
    assert got[3]["clusters"] == 1 and got[3]["collapsed"] == 3 and got[1].shape == (0, 3)
    got, _ = check(v, np.array([[0, 3, 3], [0, 3, 4], [5, 5, 5]]), 1.0)                  # a face naming a vertex twice
    assert got[3]["collapsed"] == 2 and got[5].tolist() == [1]
    got, _ = check(v, np.array([[1, 3, 4], [0, 3, 4], [4, 3, 2], [3, 5, 4]]), 1.0)       # a face given twice, and mirrored
    assert got[3]["duplicates"] == 2 and got[5].tolist() == [0, 3] and got[1].tolist() == [[0, 2, 1], [2, 3, 1]]
    got, _ = check(v, np.array([[0, 3, 4], [3, 5, 4]]), 1.0, faces_dtype=torch.int32, placement="mean")
    assert got[1].dtype == torch.int32
    # a cluster whose faces all have no area: its trace is 0 and its position the mean
    line = np.array([[0.2, 0.2, 0.2], [0.6, 0.6, 0.6], [1.5, 1.5, 1.5], [2.5, 2.5, 2.5], [2.5, 0.5, 0.5], [0.5, 2.5, 0.5]], np.float32)
    faces = np.array([[0, 2, 3], [1, 2, 3], [3, 4, 5]])
    got, st = check(line, faces, 1.0)
    mean = statement_simplify(line, faces, 1.0, placement="mean")["vertices"]
    assert np.isnan(st["x"][0]).all() and got[3]["fallback"] == 0 and (got[0][:1].cpu().numpy() == mean[:1]).all()
    edges = MS.mesh_edge_counts(got[1])
    assert edges == edge_counts_numpy(st["faces"])


@pytest.mark.gpu
def test_voxel_downsample_is_unchanged_by_the_shared_helper(dev):
    """``voxel_downsample`` and the clustering share ``cloud_filter._voxel_reduce``: the means that ``simplify_mesh`` places at
    are ``voxel_downsample``'s rows, and an ``origin`` below the minimum moves the grid for the one and not for the other."""
    from pointmvsnet_amd.cloud_filter import voxel_downsample
    v, f = roof()
    col = np.random.default_rng(2).integers(0, 256, v.shape, dtype=np.uint8)
    points, colours, _, inverse, counts = voxel_downsample(_t(v, dev), 1.0, colors=_t(col, dev), return_inverse=True,
                                                           return_counts=True)
    keys = cell_keys(v, 1.0)[0]
    uniq, inv = np.unique(keys, return_inverse=True)
    assert (inverse.cpu().numpy() == inv.reshape(-1)).all() and int(counts.sum()) == len(v)
    got = _run(dev, v, f, 1.0, col, placement="mean")
    used = torch.unique(got[4][got[4] >= 0])
    assert used.numel() == got[0].shape[0]
    rows = torch.unique(inverse[got[4] >= 0])
    assert torch.equal(got[0], points[rows]) and torch.equal(got[2], colours[rows])


@pytest.mark.gpu
def test_scan_accumulator_simplifies(dev):
    """``simplify_cell=None`` returns the bytes of a call without the argument, dense and sparse; with a cell the call is
    ``simplify_mesh`` of that mesh (after the removal of small pieces), and ``with_normals`` are the simplified mesh's."""
    from pointmvsnet_amd import mesh_ops as M
    from pointmvsnet_amd import mesh_simplify as MS
    from pointmvsnet_amd import scan as S
    depths, K, E, images, cams = make_plane_scene(5, sigma=0.0)
    nv, h, w = depths.shape
    acc = S.ScanAccumulator(nv, name="flow2", mode="NEAREST")
    prob = torch.zeros((1, 5, h, w), device=dev)
    prob[:, 2] = 1.0
    for view in range(nv):
        order = [view] + [u for u in range(nv) if u != view]
        batch = {"img_list": torch.zeros((1, nv, 3, h, w)), "cam_params_list": cams[None, order],
                 "ref_img": torch.from_numpy(images[view][None, :, :, ::-1].copy())}
        preds = {"flow2": torch.from_numpy(depths[view])[None, None].to(dev), "flow2_prob": prob,
                 "coarse_prob_map": torch.ones((1, 1, h, w), device=dev)}
        acc.add(batch, preds, view_index=view)
    voxel = 4.0
    for sparse in (False, True):
        plain = acc.mesh(voxel, min_weight=2, sparse=sparse)
        same = acc.mesh(voxel, min_weight=2, sparse=sparse, simplify_cell=None)
        assert len(plain) == 3 and len(same) == 3 and all(torch.equal(a, b) for a, b in zip(plain, same))
        assert acc.last_simplify_report is None
        want = MS.simplify_mesh(plain[0], plain[1], 3.0 * voxel, colours=plain[2])
        got = acc.mesh(voxel, min_weight=2, sparse=sparse, simplify_cell=3.0 * voxel, with_normals=True)
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got[:3], want[:3]))
        assert acc.last_simplify_report == want[3] and 0 < want[3]["faces_out"] < int(plain[1].shape[0])
        assert torch.equal(got[3], M.vertex_normals(got[0], got[1])) and got[1].dtype == plain[1].dtype
    biggest = acc.mesh(voxel, min_weight=2, keep_largest=1)
    want = MS.simplify_mesh(biggest[0], biggest[1], 2.0 * voxel, colours=biggest[2], placement="mean")
    got = acc.mesh(voxel, min_weight=2, keep_largest=1, simplify_cell=2.0 * voxel, simplify_placement="mean")
    assert all(torch.equal(a, b) for a, b in zip(got, want[:3])) and acc.last_simplify_report == want[3]
    assert acc.last_mesh_report["faces_after"] == want[3]["faces_in"]
    acc.mesh(voxel, min_weight=2)
    assert acc.last_simplify_report is None
