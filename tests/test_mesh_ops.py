"""Mesh clean-up and scoring (pointmvsnet_amd/mesh_ops.py, csrc/mesh_ops.hip) against NumPy statements written from the
module's docstring.  The statements share no code with the product.  Meshes come from the existing CPU statements
(``statement_extract`` on the sphere volumes and on the plane scene of tests/test_tsdf.py) and from a few lines of NumPy.

What is checked, and the bounds
-------------------------------
EPS = 2^-24, the unit roundoff of float32.

Components.  Yardstick: a NumPy union-find, cross-checked with ``scipy.sparse.csgraph.connected_components``.  Labels are
**equal**; two runs are byte-identical; permuted faces give the same vertex labels.  Rounds: a strip of 20 000 faces
``(i, i+1, i+2)``, identity-numbered and under three random renumberings, is one component with label 0 in at most
**32 rounds** (``2 ceil(log2 Nv) + 2``: a cap that separates logarithmic from linear; plain propagation needs about 10 000).
A synchronous NumPy simulation of hook-and-compress (hooks of a round all see the round's first state) needs 2 rounds on
the identity strip and at most 10 on the renumbered ones (asserted on the CPU).  Measured on an MI355X: 2 rounds on the identity strip
and 2 on each renumbered one (a hook that finds its root taken goes on with the root's parent, so the first round unites
everything and the second confirms it); 2 rounds on the octahedra.

Vertex normals.  The statement reproduces the float32 cross products in NumPy float32 and the float64 sum in corner order.
Zero-masks are equal and every component is within **1 float32 ulp** (the only allowance: the device's float64 ``sqrt`` and
division against the host's).  Measured on an MI355X: 0 of 17 958 components differ at all (bound: 1 ulp).

Sampling.  Yardstick: a float64 statement.  Counts must equal ``floor(x64 + u_f)``; where ``x64 + u_f`` lies within the
float32 rounding of an integer either neighbour is accepted.  The rounding bound of ``x`` follows the operations listed in
the docstring (``band_of``): the subtractions ``e = p_b - p_a`` are correctly rounded, so their error is known exactly;
each product and each sum adds EPS of its result; ``sqrtf`` at most 2 EPS (one ulp); the product with ``inv`` and the sum
with ``u_f`` EPS each.  At most **0.5 %** of the faces may lie in the band.  With the GPU's own counts ``face_index`` and
``bary`` are **equal** (integers and exact dyadics) and every point is within ``10 EPS (|p_a| + |p_b| + |p_c|)`` per
coordinate: per coordinate ``p_a + (r1 e1 + r2 e2)`` rounds ``e`` (EPS |e| each), the two products, their sum and the last
sum, and with ``|e| <= |p_a| + |p_b|``, ``r <= 1`` that is at most ``9 EPS`` of the three magnitudes' sum to first order.
The statement alone meets ``|N - sum x64| <= 6 sqrt(sum frac (1 - frac))`` and fills the four congruent quarter-triangles
of the big face with ``n / 4`` each within 6 binomial sigma (asserted on the CPU, and again on the GPU's samples).
Measured on an MI355X: plane scene mesh (2 568 faces, 2 658 719 samples) 0.156 % of the faces in the band (cap 0.5 %), no
count off, positions at most 0.186 of the bound, ``|N - sum x|`` 0.20 sigma (cap 6); triangle mesh (1 003 faces, 20 012
samples) 0.100 % in the band, no count off, positions 0.093 of the bound, total 0.15 sigma, quarters 1.35 sigma (cap 6).

``conftest.report`` carries the figures as ``mesh_components``, ``mesh_vertex_normals`` and ``mesh_sampling``.
"""
import numpy as np
import pytest
import torch

from conftest import report
from test_fusion import make_plane_scene
from test_tsdf import (SPHERES, check_sphere_mesh, grid_of, plane_scene_box, sphere_volume, statement_extract,
                       statement_integrate)
from pointmvsnet_amd import render
from pointmvsnet_amd.utils import io as IO

EPS = 2.0 ** -24
PITCH = 0.2
PLANE_D = 3.25                                  # the big triangle's plane z = D
MAX_ROUNDS = 32


# ---------------------------------------------------------------------------------------------------------------------
# the statements
# ---------------------------------------------------------------------------------------------------------------------
def statement_components(faces, nv):
    """Union-find: per vertex the smallest vertex index of its component."""
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(nv)], np.int64)


def scipy_components(faces, nv):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    rows = np.concatenate([faces[:, 0], faces[:, 1]])
    cols = np.concatenate([faces[:, 1], faces[:, 2]])
    _, comp = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nv, nv)), directed=False)
    smallest = np.full(comp.max() + 1 if nv else 0, nv, np.int64)
    np.minimum.at(smallest, comp, np.arange(nv))
    return smallest[comp]


def simulate_rounds(faces, nv):
    """A synchronous hook-and-compress: per round every edge reads the roots of the round's first state, every larger
    root takes the smallest root offered to it, then full compression.  Returns (labels, rounds), the clean round counted."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    u = np.concatenate([faces[:, 0], faces[:, 0]])
    v = np.concatenate([faces[:, 1], faces[:, 2]])
    label = np.arange(nv)
    rounds = 0
    while True:
        rounds += 1
        ru, rv = label[u], label[v]
        differ = ru != rv
        if differ.any():
            np.minimum.at(label, np.maximum(ru, rv)[differ], np.minimum(ru, rv)[differ])
        while True:
            nxt = label[label]
            if (nxt == label).all():
                break
            label = nxt
        if not differ.any():
            return label, rounds


def hash32(x):
    x = np.asarray(x).astype(np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def face_normals32(vertices, faces):
    """The float32 cross products of the docstring, every operation rounded on its own."""
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    assert n.dtype == np.float32
    return n


def statement_normals(vertices, faces):
    """float32 cross products, float64 sums in ascending corner order, float64 normalisation: (Nv, 3) float32."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n = face_normals32(vertices, faces)
    ok = np.isfinite(n).all(axis=1)
    n64 = n.astype(np.float64)
    s = np.zeros((len(vertices), 3))
    for corner, v in enumerate(faces.reshape(-1).tolist()):
        if ok[corner // 3]:
            s[v] += n64[corner // 3]
    with np.errstate(all="ignore"):
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        good = np.isfinite(length) & (length > 0)
        out = np.where(good[:, None], s / np.where(good, length, 1.0)[:, None], 0.0)
    return out.astype(np.float32)


def band_of(vertices, faces, inv):
    """``(x64, band)`` per face: ``x = area * inv`` in float64 from the float32 vertices, and the bound on the float32
    kernel's ``|x32 - x64|`` plus the rounding of ``x + u`` (module docstring).  Faces with a non-finite vertex: NaN."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e = [v[f[:, k]] - v[f[:, 0]] for k in (1, 2)]                          # exact in float64
        de = [np.abs(x.astype(np.float32).astype(np.float64) - x) for x in e]  # the float32 subtraction's own error
        e32 = [x.astype(np.float32).astype(np.float64) for x in e]
        n, dn = [], []
        for i, j in ((1, 2), (2, 0), (0, 1)):
            a, b = e[0][:, i] * e[1][:, j], e[0][:, j] * e[1][:, i]
            ain = de[0][:, i] * np.abs(e32[1][:, j]) + np.abs(e[0][:, i]) * de[1][:, j]
            bin_ = de[0][:, j] * np.abs(e32[1][:, i]) + np.abs(e[0][:, j]) * de[1][:, i]
            n.append(a - b)
            dn.append((ain + bin_ + EPS * (np.abs(a) + np.abs(b)) + EPS * np.abs(a - b)) * (1 + 8 * EPS))
        q = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        dq = sum(2 * np.abs(n[k]) * dn[k] + dn[k] * dn[k] for k in range(3)) + 3 * EPS * q * (1 + 8 * EPS)
        root = np.sqrt(q)
        droot = np.minimum(np.sqrt(dq), dq / np.maximum(root, 1e-300)) + 2 * EPS * (root + np.sqrt(dq))
        x = 0.5 * root * float(inv)
        dx = 0.5 * droot * float(inv) + EPS * (x + 0.5 * droot * float(inv))
        band = dx + EPS * (x + dx + 1.0)
    return x, band


def statement_counts(vertices, faces, pitch, seed):
    """``(count (Nf,) int64, x64, frac, band)``: ``floor(x64 + u_f)``, 0 unless x is finite."""
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / (np.float32(pitch) * np.float32(pitch))
    x, band = band_of(vertices, faces, inv)
    idx = np.arange(len(x), dtype=np.uint64)
    u = (hash32(hash32(idx ^ np.uint64(seed))) >> 8).astype(np.float64) * 2.0 ** -24
    finite = np.isfinite(x)
    y = np.where(finite, x, 0.0) + u
    count = np.where(finite, np.minimum(np.floor(y), 2.0 ** 31 - 1), 0).astype(np.int64)
    return count, np.where(finite, x, 0.0), np.where(finite, y - np.floor(y), np.nan), np.where(finite, band, 0.0), y


def statement_samples(vertices, faces, count, seed):
    """With the counts given: ``face_index`` (N,) int64, ``bary`` (N, 3) float32 (exact), ``points`` (N, 3) float64 and the
    per-sample magnitude ``|p_a| + |p_b| + |p_c|`` per coordinate."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    count = np.asarray(count, np.int64)
    fi = np.repeat(np.arange(len(f)), count)
    first = np.cumsum(count) - count
    j = (np.arange(len(fi)) - first[fi]).astype(np.uint64)
    h0 = hash32(fi.astype(np.uint64) ^ np.uint64(seed))
    i1 = (hash32((h0 + 2 * j + 1) & 0xFFFFFFFF) >> 8).astype(np.int64)
    i2 = (hash32((h0 + 2 * j + 2) & 0xFFFFFFFF) >> 8).astype(np.int64)
    r1, r2 = i1 * 2.0 ** -24, i2 * 2.0 ** -24
    fold = r1 + r2 > 1.0                                                          # exact in float64
    r1, r2 = np.where(fold, 1.0 - r1, r1), np.where(fold, 1.0 - r2, r2)
    bary = np.stack([1.0 - r1 - r2, r1, r2], axis=1)
    assert (bary >= 0).all() and (bary.astype(np.float32).astype(np.float64) == bary).all()
    assert ((bary[:, 0] + bary[:, 1]) + bary[:, 2] == 1.0).all()
    pa, pb, pc = v[f[fi, 0]], v[f[fi, 1]], v[f[fi, 2]]
    points = pa + (r1[:, None] * (pb - pa) + r2[:, None] * (pc - pa))
    return fi, bary.astype(np.float32), points, np.abs(pa) + np.abs(pb) + np.abs(pc)


def quarter_counts(bary):
    """How many samples fall into each of the four congruent quarter-triangles (corner a, corner b, corner c, middle)."""
    b = np.asarray(bary, np.float64)
    corner = [(b[:, k] > 0.5).sum() for k in range(3)]
    return np.array(corner + [len(b) - sum(corner)])


def check_sampling_statistics(x, frac, total, big_bary):
    """The two conditions the statement alone must meet (module docstring); returns their figures in sigmas."""
    sigma = np.sqrt(np.nansum(frac * (1.0 - frac)))
    off = abs(total - x.sum()) / max(sigma, 1e-300)
    assert off <= 6.0, (total, x.sum(), sigma)
    n = len(big_bary)
    quarters = quarter_counts(big_bary)
    qs = np.abs(quarters - n / 4.0).max() / np.sqrt(n * 0.25 * 0.75)
    assert qs <= 6.0, quarters
    return off, qs


# ---------------------------------------------------------------------------------------------------------------------
# the meshes
# ---------------------------------------------------------------------------------------------------------------------
def octahedra_mesh(count=300, seed=3):
    """``count`` octahedra, vertex numbering and face order shuffled, 5 unreferenced vertices, a duplicated face and a face
    (a, a, b): faces (8 count + 2, 3) int64, nv = 6 count + 5."""
    rng = np.random.default_rng(seed)
    octa = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    nv = 6 * count + 5
    number = rng.permutation(nv)
    faces = np.concatenate([number[octa + 6 * i] for i in range(count)])
    faces = np.concatenate([faces, faces[17:18], [[faces[40, 0], faces[40, 0], faces[40, 1]]]])
    return faces[rng.permutation(len(faces))].astype(np.int64), nv


def strip_mesh(n=20000, seed=None):
    faces = np.arange(n)[:, None] + np.arange(3)[None, :]
    if seed is not None:
        faces = np.random.default_rng(seed).permutation(n + 2)[faces]
    return faces.astype(np.int64), n + 2


def sphere17_mesh():
    n, centre, r = SPHERES["on_sample_17"]
    f, wgt = sphere_volume(n, centre, r)
    _, faces, vertices, _, _ = statement_extract(f, wgt, (0.0, 0.0, 0.0), 1.0)
    return vertices.astype(np.float32), faces.astype(np.int64), np.asarray(centre)


def plane_mesh():
    """The plane scene's TSDF mesh by the CPU statements of tests/test_tsdf.py at its smaller grid, with colours."""
    depths, K, E, images, lo, hi = plane_scene_box()
    dims = (21, 19, 17)
    origin, voxel, trunc = grid_of(lo, hi, dims)
    st = statement_integrate(depths, images, render.world_maps(K, E), origin, voxel, dims, trunc)
    _, faces, vertices, colours, _ = statement_extract(st["tsdf"].astype(np.float32), st["W"].astype(np.int32), origin, voxel, 1,
                                                       st["colour"])
    return vertices.astype(np.float32), faces.astype(np.int64), np.clip(np.floor(colours + 0.5), 0, 255).astype(np.uint8)


def fan_mesh(n=1000, lift=0.0):
    """A fan of ``n`` faces around one apex (vertex 0), counter-clockwise seen from +z; ``lift`` raises the apex."""
    ang = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([3.0 * np.cos(ang) + 0.7, 2.0 * np.sin(ang) - 0.4, np.full(n, 1.5)], axis=1)
    vertices = np.concatenate([[[0.7, -0.4, 1.5 + lift]], ring]).astype(np.float32)
    i = np.arange(n)
    return vertices, np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1)


def triangle_mesh():
    """One right triangle in the plane z = D sized for about 20 000 samples at PITCH, next to 1 000 faces of area
    0.01 PITCH^2, a zero-area face and a face with a NaN vertex."""
    leg = np.sqrt(2.0 * 20000.0) * PITCH
    big = np.array([[1.0, 2.0, PLANE_D], [1.0 + leg, 2.0, PLANE_D], [1.0, 2.0 + leg, PLANE_D]])
    small_leg = np.sqrt(2.0 * 0.01) * PITCH
    k = np.arange(1000)
    base = np.stack([50.0 + 0.1 * (k % 40), -3.0 + 0.1 * (k // 40), 0.01 * k], axis=1)
    small = np.stack([base, base + [small_leg, 0, 0], base + [0, small_leg, 0]], axis=1).reshape(-1, 3)
    extra = np.array([[5.0, 5.0, 5.0], [6.0, 6.0, 6.0], [7.0, 7.0, 7.0], [np.nan, 0.0, 0.0]])      # collinear; NaN
    vertices = np.concatenate([big, small, extra]).astype(np.float32)
    faces = np.concatenate([[[0, 1, 2]], 3 + np.arange(3000).reshape(1000, 3), [[3003, 3004, 3005], [0, 1, 3006]]])
    return vertices, faces.astype(np.int64)


def two_sphere_volume(n=33):
    """Two spheres of different radius in one (n, n, n) volume (origin 0, voxel 1), and a seeded colour volume."""
    big = sphere_volume(n, (11.3, 11.6, 11.45), 8.3)[0]
    small = sphere_volume(n, (25.4, 25.2, 25.6), 4.2)[0]
    colour = np.random.default_rng(5).integers(0, 256, (n, n, n, 3), dtype=np.uint8)
    return np.minimum(big, small), np.ones((n, n, n), np.int32), colour


@pytest.fixture(scope="module")
def meshes():
    out = {"sphere17": sphere17_mesh(), "plane": plane_mesh(), "triangle": triangle_mesh()}
    v, f, _ = out["sphere17"]
    assert (np.linalg.norm(face_normals32(v, f), axis=1) == 0).sum() > 100          # it has zero-area faces
    return out


@pytest.fixture(scope="module")
def sampling_statements(meshes):
    """Per input: the statement's counts and, for the triangle mesh, its own samples (the CPU test's non-vacuity check)."""
    out = {}
    for name in ("plane", "triangle"):
        v, f = meshes[name][:2]
        out[name] = statement_counts(v, f, PITCH, seed=0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_a_device_is_needed():
    from pointmvsnet_amd import mesh_ops as M
    from pointmvsnet_amd import scan as S
    v = torch.zeros((4, 3))
    f = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    for bad in (f.float(), f[:, :2], f[0], None, f.to(torch.int16)):
        with pytest.raises(ValueError, match="faces must be"):
            M.mesh_components(bad, 4)
        with pytest.raises(ValueError, match="faces must be"):
            M.vertex_normals(v, bad)
    for bad in (-1, 2.5, None, 2 ** 31, True):
        with pytest.raises(ValueError, match="num_vertices|fewer than 2\\^31"):
            M.mesh_components(f, bad)
    for bad in (v.double(), v[:, :2], v[0], None):
        with pytest.raises(ValueError, match="vertices must be"):
            M.vertex_normals(bad, f)
        with pytest.raises(ValueError, match="vertices must be"):
            M.sample_surface(bad, f, 0.1)
        with pytest.raises(ValueError, match="vertices must be"):
            M.remove_small_components(bad, f)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x", 1e-30, 1e30):
        with pytest.raises(ValueError, match="pitch"):
            M.sample_surface(v, f, bad)
    for bad in (-1, 2 ** 32, 0.5, None, True):
        with pytest.raises(ValueError, match="seed"):
            M.sample_surface(v, f, 0.1, seed=bad)
    for kw in ({"min_faces": -1}, {"min_faces": 1.5}, {"keep_largest": -2}, {"keep_largest": True}):
        with pytest.raises(ValueError, match="non-negative integer"):
            M.remove_small_components(v, f, **kw)
    with pytest.raises(ValueError, match="colours must be"):
        M.remove_small_components(v, f, colours=torch.zeros((3, 3)))
    with pytest.raises(ValueError, match="normals must be"):
        M.remove_small_components(v, f, normals=torch.zeros((4,)))
    with pytest.raises(ValueError, match="face_label"):
        M.component_sizes(torch.zeros((3,)))
    for call in (lambda: M.mesh_components(f, 4), lambda: M.vertex_normals(v, f), lambda: M.sample_surface(v, f, 0.1),
                 lambda: M.remove_small_components(v, f)):
        with pytest.raises(RuntimeError, match="no CPU path"):                       # well-formed: only the device is missing
            call()
    acc = S.ScanAccumulator(2)
    assert acc.last_mesh_report is None
    with pytest.raises(ValueError, match="non-negative integer"):
        acc.mesh(1.0, min_component_faces=-3)
    with pytest.raises(ValueError, match="have not been added"):
        acc.mesh(1.0, min_component_faces=3, with_normals=True)
    # the plumbing that is plain torch works on the host: the corner table and the sizes
    with pytest.raises(ValueError, match="face indices run from"):
        M.vertex_corner_table(torch.tensor([[0, 1, 4]]), 4)
    offsets, corners = M.vertex_corner_table(torch.tensor([[2, 0, 2], [0, 3, 2]]), 5)
    assert offsets.tolist() == [0, 2, 2, 5, 6, 6] and corners.tolist() == [1, 3, 0, 2, 5, 4]
    labels, counts = M.component_sizes(torch.tensor([7, 0, 7, 7, 3], dtype=torch.int32))
    assert labels.tolist() == [0, 3, 7] and counts.tolist() == [1, 1, 3]
    keep, n = M._select_faces(torch.tensor([7, 0, 7, 3, 3, 9, 9]), None, 2)          # sizes 1, 2, 2, 2: ties to 3 and 7
    assert n == 4 and keep.tolist() == [True, False, True, True, True, False, False]
    keep, _ = M._select_faces(torch.tensor([7, 0, 7, 3, 3, 9, 9]), 2, 1)
    assert keep.tolist() == [False, False, False, True, True, False, False]


def test_kernels_are_built_and_bound(lib_built):
    import subprocess
    from pointmvsnet_amd import _lib, build
    names = ["pf_mesh_cc_hook", "pf_mesh_cc_compress", "pf_mesh_face_labels", "pf_mesh_vertex_normals_f32",
             "pf_mesh_sample_count_f32", "pf_mesh_sample_emit_f32"]
    assert "mesh_ops.hip" in build.SOURCES
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib_built]).decode()
    lib = _lib.load()
    for name in names:
        assert name in _lib.PROTOTYPES and (" T %s\n" % name) in exported and getattr(lib, name) is not None
    assert lib.pf_mesh_cc_hook(None, -1, 4, None, None, None) == -1                   # sizes are checked before anything runs
    assert lib.pf_mesh_sample_emit_f32(None, 4, None, 2, None, 2 ** 31, 0, None, None, None, None) == -1
    assert lib.pf_mesh_cc_compress(None, 0, None) == 0 and lib.pf_mesh_face_labels(None, 0, 0, None, None, None) == 0


def test_component_statements_agree_and_rounds_are_logarithmic():
    faces, nv = octahedra_mesh()
    assert nv % 64 and len(faces) % 64 and nv % 256 and len(faces) % 256
    want = statement_components(faces, nv)
    assert (want == scipy_components(faces, nv)).all()
    assert len(np.unique(want)) == 300 + 5 and (np.bincount(want)[np.unique(want)] <= 6).all()
    sim, rounds = simulate_rounds(faces, nv)
    assert (sim == want).all() and rounds <= MAX_ROUNDS
    faces, nv = strip_mesh()
    assert MAX_ROUNDS == 2 * int(np.ceil(np.log2(nv))) + 2
    sim, rounds = simulate_rounds(faces, nv)
    assert (sim == 0).all() and rounds == 2
    worst = 0
    for seed in (11, 12, 13):
        faces, nv = strip_mesh(seed=seed)
        assert sorted(np.unique(faces).tolist()) == list(range(nv))
        sim, rounds = simulate_rounds(faces, nv)
        assert (sim == 0).all()
        worst = max(worst, rounds)
    print("synchronous simulation: rounds on renumbered strips", worst)
    assert worst <= 10


def test_normal_statement_is_not_vacuous(meshes):
    v, f, centre = meshes["sphere17"]
    n = statement_normals(v, f).astype(np.float64)
    defined = np.abs(n).sum(1) > 0
    assert defined.mean() > 0.9 and np.abs(np.linalg.norm(n[defined], axis=1) - 1.0).max() < 1e-6
    assert ((n * (v - centre)).sum(1) > 0)[defined].all()        # (a vertex with only zero-area faces has no normal)
    vf, ff = fan_mesh()
    nf = statement_normals(vf, ff)
    assert (nf == np.array([0.0, 0.0, 1.0], np.float32)).all()
    bad = v.copy()
    bad[7] = np.nan
    nb = statement_normals(bad, f)
    touched = np.unique(f[(f == 7).any(1)])
    assert (nb[7] == 0).all() and np.isfinite(nb).all() and (nb[touched] != n[touched].astype(np.float32)).any()


def test_sampling_statement_is_not_vacuous(meshes, sampling_statements):
    for name in ("plane", "triangle"):
        v, f = meshes[name][:2]
        count, x, frac, band, y = sampling_statements[name]
        near = np.abs(y - np.round(y)) <= band
        share = near.mean()
        print(name, "faces", len(f), "samples", count.sum(), "share of faces in the rounding band", share,
              "largest band", band.max())
        assert share <= 0.005
        if name == "plane":
            assert 2.0e6 < count.sum() < 3.5e6 and (count > 0).mean() > 0.95
            sigma = np.sqrt(np.nansum(frac * (1 - frac)))
            assert abs(count.sum() - x.sum()) <= 6 * sigma
        else:
            assert count[-2] == 0 and count[-1] == 0 and x[-2] == 0.0                    # zero area; NaN
            assert abs(x[0] - 20000.0) < 1.0 and np.abs(x[1:1001] - 0.01).max() < 1e-4
            assert 0 < count[1:1001].sum() < 40 and count[1:1001].max() == 1            # 10 expected, sigma 3.2
            fi, bary, points, _ = statement_samples(v, f, count, 0)
            off, qs = check_sampling_statistics(x, frac, count.sum(), bary[fi == 0])
            print("triangle: |N - sum x| in sigmas", off, "quarters off in sigmas", qs)
            assert (points[fi == 0][:, 2] == PLANE_D).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. GPU
# ---------------------------------------------------------------------------------------------------------------------
def _t(a, dev, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dtype is None else torch.from_numpy(
        np.ascontiguousarray(a)).to(dtype).to(dev)


@pytest.mark.gpu
def test_components_match_union_find(dev):
    from pointmvsnet_amd import mesh_ops as M
    faces, nv = octahedra_mesh()
    want = statement_components(faces, nv)
    assert (want == scipy_components(faces, nv)).all()
    vl, fl, rounds = M.mesh_components(_t(faces, dev), nv, return_rounds=True)
    assert vl.dtype == torch.int32 and fl.dtype == torch.int32 and vl.shape == (nv,) and fl.shape == (len(faces),)
    assert (vl.cpu().numpy() == want).all() and (fl.cpu().numpy() == want[faces[:, 0]]).all()
    assert 1 <= rounds <= MAX_ROUNDS and M.last_component_rounds() == rounds
    vl2, fl2 = M.mesh_components(_t(faces, dev, torch.int32), nv)
    assert torch.equal(vl, vl2) and torch.equal(fl, fl2)                              # two runs, and int32 as int64
    perm = np.random.default_rng(1).permutation(len(faces))
    vl3, fl3 = M.mesh_components(_t(faces[perm], dev), nv)
    assert torch.equal(vl, vl3) and torch.equal(fl3, fl[_t(perm, dev)])
    labels, counts = M.component_sizes(fl)
    assert labels.tolist() == np.unique(want[faces[:, 0]]).tolist() and int(counts.sum()) == len(faces)
    assert sorted(counts.tolist())[-2:] == [9, 9] and sorted(counts.tolist())[0] == 8
    empty = torch.zeros((0, 3), dtype=torch.int64, device=dev)
    vl0, fl0, r0 = M.mesh_components(empty, 7, return_rounds=True)
    assert vl0.tolist() == list(range(7)) and fl0.shape == (0,) and r0 == 0
    vl0, fl0 = M.mesh_components(empty, 0)
    assert vl0.shape == (0,) and fl0.shape == (0,)
    with pytest.raises(ValueError, match="face indices run from"):
        M.mesh_components(_t(np.array([[0, 1, nv]]), dev), nv)
    with pytest.raises(ValueError, match="face indices run from"):
        M.mesh_components(_t(np.array([[0, -1, 2]]), dev), nv)
    report("mesh_components", vertices=nv, faces=len(faces), components=len(np.unique(want)), rounds=rounds)


@pytest.mark.gpu
def test_component_rounds_on_strips(dev):
    from pointmvsnet_amd import mesh_ops as M
    measured = []
    for seed in (None, 11, 12, 13):
        faces, nv = strip_mesh(seed=seed)
        vl, fl, rounds = M.mesh_components(_t(faces, dev), nv, return_rounds=True)
        measured.append(rounds)
        assert int(vl.max()) == 0 and int(fl.max()) == 0 and int(vl.min()) == 0
    print("rounds on the strips (identity, three renumberings):", measured)
    report("mesh_components", strip_rounds_identity=measured[0], strip_rounds_renumbered_max=max(measured[1:]))
    assert max(measured) <= MAX_ROUNDS


@pytest.mark.gpu
def test_removal_on_two_spheres(dev):
    from pointmvsnet_amd import mesh_ops as M
    from pointmvsnet_amd import tsdf as T
    f, wgt, colour = two_sphere_volume()
    vertices, faces, colours, _ = T.extract_mesh(_t(f, dev), _t(wgt, dev), (0.0, 0.0, 0.0), 1.0, colour=_t(colour, dev))
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    vl, fl = M.mesh_components(faces, nv)
    labels, counts = M.component_sizes(fl)
    assert labels.numel() == 2 and int(vl.unique().numel()) == 2
    small, large = sorted(counts.tolist())
    assert small * 2 < large
    normals = M.vertex_normals(vertices, faces)
    results = []
    for kw in ({"min_faces": (small + large) // 2}, {"keep_largest": 1}, {"min_faces": small + 1, "keep_largest": 2}):
        v2, f2, c2, n2, vmap, keep = M.remove_small_components(vertices, faces, colours=colours, normals=normals,
                                                               return_maps=True, **kw)
        results.append((v2, f2))
        assert f2.dtype == faces.dtype and int(f2.shape[0]) == large and int(keep.sum()) == large
        worst, flat = check_sphere_mesh(v2.cpu().numpy(), f2.cpu().numpy(), (11.3, 11.6, 11.45), 8.3)   # closed, chi 2, outward
        used = vmap >= 0
        assert torch.equal(v2, vertices[used]) and torch.equal(c2, colours[used]) and torch.equal(n2, normals[used])
        assert torch.equal(vmap[used], torch.arange(int(used.sum()), device=dev))                      # original order
        assert torch.equal(f2.long(), vmap[faces[keep].long()]) and int(vmap[faces[~keep].long()].max()) == -1
        assert int(f2.unique().numel()) == int(v2.shape[0])                                            # none unreferenced
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    extra = torch.cat([vertices, torch.full((3, 3), 9.0, device=dev)])                                 # both None: the mesh
    v3, f3, c3, n3 = M.remove_small_components(extra, faces.long())                                    # minus unreferenced
    assert torch.equal(v3, vertices) and torch.equal(f3, faces.long()) and c3 is None and n3 is None
    v4, f4, _, _ = M.remove_small_components(vertices, faces, min_faces=large + 1)
    assert v4.shape == (0, 3) and f4.shape == (0, 3)
    v5, f5, _, _ = M.remove_small_components(vertices, faces, keep_largest=0)
    assert v5.shape == (0, 3) and f5.shape == (0, 3)
    v6, f6, _, _ = M.remove_small_components(vertices[:0], faces[:0], min_faces=1)
    assert v6.shape == (0, 3) and f6.shape == (0, 3)


@pytest.mark.gpu
def test_vertex_normals_match_the_statement(dev, meshes):
    from pointmvsnet_amd import mesh_ops as M
    sv, sf, centre = meshes["sphere17"]
    nan_v = sv.copy()
    nan_v[7] = np.nan
    cases = {"sphere17": (sv, sf), "plane": meshes["plane"][:2], "fan": fan_mesh(lift=0.8), "nan": (nan_v, sf),
             "flat_fan": fan_mesh()}
    differ = worst = total = 0
    for name, (v, f) in cases.items():
        want = statement_normals(v, f)
        got = M.vertex_normals(_t(v, dev), _t(f, dev, torch.int32 if name == "plane" else None)).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all(), name
        assert ((got == 0).all(1) == (want == 0).all(1)).all(), name
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
        off = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp
        differ += int((got != want).sum())
        total += got.size
        worst = max(worst, float(off.max()))
        assert off.max() <= 1.0, (name, off.max())
        length = np.linalg.norm(got.astype(np.float64), axis=1)
        assert np.abs(length[length > 0] - 1.0).max() < 4 * EPS * 2, name
        if name == "sphere17":
            assert (length > 0).mean() > 0.9 and ((got * (v - centre)).sum(1) > 0)[length > 0].all()
        if name == "nan":
            assert (got[7] == 0).all()
        if name == "flat_fan":
            assert (got == np.array([0.0, 0.0, 1.0], np.float32)).all()
    print("vertex normals: components that differ at all", differ, "of", total, "; largest difference in ulp", worst)
    report("mesh_vertex_normals", components=total, differ=differ, worst_ulp=worst)
    lone = M.vertex_normals(torch.zeros((3, 3), device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev))
    assert lone.shape == (3, 3) and (lone == 0).all()
    none = M.vertex_normals(torch.zeros((0, 3), device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev))
    assert none.shape == (0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plane", "triangle"])
def test_sampling_matches_the_statement(dev, meshes, sampling_statements, name):
    from pointmvsnet_amd import mesh_ops as M
    v, f = meshes[name][:2]
    want, x, frac, band, y = sampling_statements[name]
    tv, tf = _t(v, dev), _t(f, dev)
    points, face_index, bary = M.sample_surface(tv, tf, PITCH)
    again = M.sample_surface(tv, tf.to(torch.int32), PITCH, seed=0)
    assert all(torch.equal(a, b) for a, b in zip((points, face_index, bary), again))          # two runs, byte for byte
    assert points.dtype == torch.float32 and face_index.dtype == torch.int32 and bary.dtype == torch.float32
    fi = face_index.cpu().numpy().astype(np.int64)
    assert (np.diff(fi) >= 0).all() and fi.min() >= 0 and fi.max() < len(f)
    count = np.bincount(fi, minlength=len(f))
    near = np.abs(y - np.round(y)) <= band
    wrong = count != want
    assert not (wrong & ~near).any(), np.nonzero(wrong & ~near)[0][:10]
    assert (np.abs(count - want)[wrong] == 1).all() and near.mean() <= 0.005
    sfi, sbary, spoints, scale = statement_samples(v, f, count, 0)                            # with the GPU's own counts
    assert (sfi == fi).all() and (bary.cpu().numpy() == sbary).all()
    got = points.cpu().numpy().astype(np.float64)
    ratio = (np.abs(got - spoints) / (10 * EPS * scale + 1e-300)).max()
    assert ratio <= 1.0, ratio
    sigma = np.sqrt(np.nansum(frac * (1 - frac)))
    total_off = abs(len(fi) - x.sum()) / sigma
    assert total_off <= 6.0
    figures = dict(faces=len(f), samples=len(fi), band_share=near.mean(), counts_off_by_one=int(wrong.sum()),
                   position_err_over_bound=ratio, total_off_sigmas=total_off)
    if name == "triangle":
        assert count[-2] == 0 and count[-1] == 0                                              # zero area; NaN vertex
        big = fi == 0
        _, qs = check_sampling_statistics(x, frac, len(fi), sbary[big])
        figures["quarters_off_sigmas"] = qs
        assert (points.cpu().numpy()[big][:, 2] == np.float32(PLANE_D)).all()                 # in the plane z = D exactly
        other, _, _ = M.sample_surface(tv, tf, PITCH, seed=12345)
        assert other.shape[0] != points.shape[0] or not torch.equal(other, points)
    else:
        colours = _t(meshes["plane"][2], dev).float()                                         # the attribute route
        rgb = render.interpolate_vertex_attributes(face_index.view(1, 1, -1), bary.view(1, 1, -1, 3), tf, colours)
        c = meshes["plane"][2].astype(np.float64)[f[fi]]                                      # (N, 3 corners, 3)
        want_rgb = (sbary.astype(np.float64)[:, :, None] * c).sum(1)
        assert rgb.shape == (1, 1, len(fi), 3) and np.abs(rgb[0, 0].cpu().numpy() - want_rgb).max() <= 8 * EPS * 255
    print(name, figures)
    report("mesh_sampling", **figures)


@pytest.mark.gpu
def test_sampling_refuses_more_than_int32_samples_before_the_emit_launch(dev, meshes, monkeypatch):
    from pointmvsnet_amd import _lib
    from pointmvsnet_amd import mesh_ops as M
    v, f = meshes["triangle"]
    launched = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **kw: (launched.append(name), real(name, *a, **kw))[1])
    with pytest.raises(ValueError, match="more than 2\\^31 - 1"):
        M.sample_surface(_t(v, dev), _t(f, dev), 1e-4)                # the big face alone asks for 8e10: its count is clamped
    assert launched == ["pf_mesh_sample_count_f32"]
    empty = M.sample_surface(_t(v, dev), torch.zeros((0, 3), dtype=torch.int32, device=dev), PITCH)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,) and empty[2].shape == (0, 3)
    none = M.sample_surface(_t(v[-4:-1], dev), torch.tensor([[0, 1, 2]], device=dev), PITCH)   # only a zero-area face
    assert none[0].shape == (0, 3)


@pytest.mark.gpu
def test_scan_accumulator_mesh_options(dev, tmp_path):
    """``ScanAccumulator.mesh`` with the defaults is what it was (a 3-tuple, equal to a second call and to the plain
    TSDF route); with ``min_component_faces`` and ``with_normals`` it is ``remove_small_components`` and
    ``vertex_normals`` of that mesh, ``write_mesh`` round-trips normals and faces, and ``last_mesh_report`` says what went."""
    from pointmvsnet_amd import mesh_ops as M
    from pointmvsnet_amd import scan as S
    depths, K, E, images, cams = make_plane_scene(5, sigma=0.0)
    nv, h, w = depths.shape
    acc = S.ScanAccumulator(nv, name="flow2", mode="NEAREST")
    prob = torch.zeros((1, 5, h, w), device=dev)
    prob[:, 2] = 1.0
    for v in range(nv):
        order = [v] + [u for u in range(nv) if u != v]
        batch = {"img_list": torch.zeros((1, nv, 3, h, w)), "cam_params_list": cams[None, order],
                 "ref_img": torch.from_numpy(images[v][None, :, :, ::-1].copy())}
        preds = {"flow2": torch.from_numpy(depths[v])[None, None].to(dev), "flow2_prob": prob,
                 "coarse_prob_map": torch.ones((1, 1, h, w), device=dev)}
        acc.add(batch, preds, view_index=v)
    voxel = 4.0
    plain = acc.mesh(voxel, min_weight=2)
    assert len(plain) == 3 and acc.last_mesh_report is None
    second = acc.mesh(voxel, min_weight=2)
    assert all(torch.equal(a, b) for a, b in zip(plain, second))
    vertices, faces, colours = plain
    _, fl, rounds = M.mesh_components(faces, int(vertices.shape[0]), return_rounds=True)
    labels, counts = M.component_sizes(fl)
    assert labels.numel() >= 2                                        # the outlier block is a piece of its own
    threshold = int(counts.max())
    want = M.remove_small_components(vertices, faces, min_faces=threshold, colours=colours)
    path = str(tmp_path / "mesh.ply")
    got = acc.write_mesh(path, voxel=voxel, min_weight=2, min_component_faces=threshold, with_normals=True)
    assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got[:3], want[:3]))
    assert torch.equal(got[3], M.vertex_normals(got[0], got[1])) and got[1].dtype == torch.int32
    rep = acc.last_mesh_report
    assert rep == {"components": int(labels.numel()), "vertices_before": int(vertices.shape[0]),
                   "vertices_after": int(got[0].shape[0]), "faces_before": int(faces.shape[0]), "faces_after": threshold,
                   "rounds": rounds}
    assert rep["vertices_after"] < rep["vertices_before"] and 1 <= rep["rounds"] <= MAX_ROUNDS
    p, col, nrm, f = IO.load_ply_mesh(path)
    assert (p == got[0].cpu().numpy()).all() and (f == got[1].cpu().numpy()).all()
    assert (col == got[2].cpu().numpy()).all() and (nrm == got[3].cpu().numpy()).all()
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    largest = acc.mesh(voxel, min_weight=2, keep_largest=1)
    assert len(largest) == 3 and torch.equal(largest[1], got[1]) and acc.last_mesh_report["faces_after"] == threshold
    acc.mesh(voxel, min_weight=2, with_normals=True)
    assert acc.last_mesh_report is None
