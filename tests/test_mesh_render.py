"""Mesh rasterisation (pointmvsnet_amd/render.py "Mesh rasterisation", csrc/mesh_render.hip) against a NumPy statement of its
specification, and the layers above it: ``interpolate_vertex_attributes``, ``ScanAccumulator.depth_errors(gt_faces=...)``
and ``ScanAccumulator.render_mesh``.

The specification is the text in pointmvsnet_amd/render.py; the yardstick is ``statement`` below, written from that text
with no code shared with the product.  Coverage is exact integer arithmetic on the table of fixed-point screen positions,
so the raster tests are **teacher-forced on the GPU's own table** (``render.mesh_screen_coordinates``, which the kernels
compute with the one device function they share): coverage, ownership of shared edges and the winner are then judged in
exact integers and excuse no pixel.  The table itself is judged against float64 on its own (test 3).

The bounds (eps = 2^-24, gamma_n = n eps / (1 - n eps))
-------------------------------------------------------
*Screen table.*  ``project64`` of tests/test_render.py gives ``u64``, ``z64`` and the derived ``eps_u``, ``eps_z``.
``u * 256.0f`` is exact and ``rintf`` moves it by at most 0.5: ``|xi - 256 u64| <= 0.5 + 256 eps_u``, ``|z - z64| <= eps_z``.
``valid`` must be equal for every vertex; the test first asserts that every inequality of the validity test holds or fails by
more than its eps, so the float64 verdict is the only one a correct kernel can reach.

*Depth.*  ``z = fl(fl(area2) / inv)``, ``inv = fl(fl(fl(Ea) ra + fl(Eb) rb) + fl(Ec) rc)``, ``ra = fl(1 / za)``.  A term
``fl(fl(E) r)`` carries three roundings (the reciprocal, the conversion, the product), the first sum adds one to two of the
terms and the second sum one to all three: every term of ``inv`` carries at most 5 factors ``(1 + d)``, all terms are
non-negative, so ``inv = inv64 (1 + t5)`` with ``|t5| <= gamma_5``.  The conversion of ``area2`` and the division add two:
``|z - z64| <= gamma_7 z64``.  ``z64`` is the same formula in float64 on the same table (its own error, gamma_8 of 2^-53, is
added).  No factor on top.

*Barycentrics.*  ``fl(fl(fl(E) r) / inv)``: 3 + 5 + 1 roundings, each weight is its exact value times ``(1 + t9)``; the exact
weights lie in [0, 1] and sum to 1, so each is in ``[0, 1 + gamma_9]``, their float64 sum is within ``gamma_9`` of 1, and
``sum_k bary_k z_k`` is within ``gamma_9 depth`` of the depth (``fl(1 / z_k) z_k = 1 + d`` is among the nine).

*Closed form.*  For a plane, ``1 / z`` is affine in the image position: ``g(u, v) = alpha + beta u + gamma v``.  The
rasteriser interpolates the vertices' exact ``1 / z`` over the SNAPPED triangle ``p_i' = p_i + d_i``, ``|d_i|_inf <= 1/512 +
eps_u``: ``g'(s) - g(s) = - sum_i lambda_i(s) grad g . d_i`` with barycentrics ``lambda_i >= 0`` summing to 1, so ``|g' - g|
<= (|beta| + |gamma|) (1/512 + eps_u)`` and ``|z' - z| = z z' |g' - g| <= zmax^2 (|beta| + |gamma|) (1/512 + eps_u) =:
snap`` -- the plane's depth slope per pixel times 1/512 pixel.  The map is within ``gamma_7 (z + snap) + snap`` of the closed
form; for a fronto-parallel plane ``snap = 0``.

The scene of tests 4, 8 and 10 (``make_scene``): a wavy height-field grid (shared edges everywhere) in front of a
two-triangle back plane (faces far above ``MESH_LANE_PIXELS``), three cameras; faces sticking out of the map on every side
and one entirely outside; zero-area faces (collinear, exactly so in view 0, and a repeated index); a face with an index
``>= Nv`` and one with a negative index; faces with a vertex behind the cameras, a NaN and an inf vertex; exact duplicates;
shuffled.  ``test_statement_scene_is_not_vacuous`` verifies on the CPU, on a table made with NumPy float32, that at least
half of the pixels have a coverer and at least a tenth of those two coverers farther apart than the sum of their bounds.

Measured on tests/hipemu (the kernel sources compiled for the host) and on an MI355X, the same figures on both: no pixel
violates a condition in any test; largest ``|xi - 256 u64| / bound`` 0.994 (the bound is 0.5 + 256 eps_u, and ``rintf`` alone
may use 0.5 of it), ``|z - z64| / eps_z`` 0.31 (test 3); largest ``|depth - z64| / bound`` 0.45 in the random scene (test 4),
0.42 at the lane / wave boundary (test 6); closed form (test 7) 0.32 of the bound on the fronto-parallel plane (bound 3.0e-6)
and 0.11 on the tilted one (bound 8.4e-4, of which snapping 8.3e-4); ``|sum bary z - depth| / (gamma_9 depth)`` 0.31 (test
10).  ``conftest.report`` carries them (``mesh_screen_table``, ``mesh_random_scene``, ``mesh_lane_wave``,
``mesh_closed_form``, ``mesh_barycentrics``).
"""
import numpy as np
import pytest
import torch

from conftest import report
from pointmvsnet_amd import render
from test_render import EPS32, project64

H, W, V = 24, 40, 3                   # not a multiple of any tile
G = 16384


def gamma(n, eps=EPS32):
    return n * eps / (1 - n * eps)


REL_DEPTH = gamma(7) + gamma(8, 2.0 ** -53)
REL_BARY = gamma(9)


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def table32(vertices, proj, h, w, depth_min=1e-3, depth_max=1e5):
    """"Screen coordinates" in NumPy float32 in the text's order: ``xy`` (V, Nv, 2) int64, ``z`` (V, Nv) float32, ``valid``."""
    P = np.asarray(proj, np.float32).reshape(-1, 3, 4)
    X, Y, Z = (np.asarray(vertices, np.float32)[:, k][None, :] for k in range(3))
    with np.errstate(all="ignore"):
        qx, qy, z = (((P[:, r, 0, None] * X + P[:, r, 1, None] * Y) + P[:, r, 2, None] * Z) + P[:, r, 3, None] for r in range(3))
        u, v = qx / z, qy / z
        assert u.dtype == np.float32 and z.dtype == np.float32
        valid = (z > np.float32(depth_min)) & (z < np.float32(depth_max))
        valid &= (u >= np.float32(-G)) & (u < np.float32(w + G)) & (v >= np.float32(-G)) & (v < np.float32(h + G))
        xy = np.stack([np.rint(np.where(valid, u, 0) * np.float32(256.0)), np.rint(np.where(valid, v, 0) * np.float32(256.0))], -1)
    return xy.astype(np.int64), z, valid


def statement(xy, z, valid, faces, h, w, cull=None):
    """"A face in a view", "Coverage" and "Depth" from a table: ``cover`` (V, Nf, h, w) bool in exact integers, ``z64``
    (V, Nf, h, w) the depth formula in float64 (nan where not covered), ``front`` (V, Nf) and ``boxes`` (V, Nf) the number of
    pixel centres in the bounding box clamped to the map (0 for a face that is not rasterised)."""
    nv, n_vert = valid.shape
    faces = np.asarray(faces).tolist()
    SX, SY = (256 * np.arange(w, dtype=np.int64) + 128)[None, :], (256 * np.arange(h, dtype=np.int64) + 128)[:, None]
    cover = np.zeros((nv, len(faces), h, w), bool)
    z64 = np.full((nv, len(faces), h, w), np.nan)
    front, boxes = np.zeros((nv, len(faces)), bool), np.zeros((nv, len(faces)), np.int64)

    def edge(p, q):
        dx, dy = q[0] - p[0], q[1] - p[1]
        E = dx * (SY - p[1]) - dy * (SX - p[0])
        return E, (E > 0) | ((E == 0) & bool(dy > 0 or (dy == 0 and dx < 0)))

    for v in range(nv):
        for f, tri in enumerate(faces):
            if not all(0 <= i < n_vert for i in tri) or not all(valid[v, i] for i in tri):
                continue
            a, b, c = ((int(xy[v, i, 0]), int(xy[v, i, 1]), float(z[v, i])) for i in tri)
            area2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
            if area2 == 0:
                continue
            front[v, f] = area2 < 0
            if (cull == "back" and area2 > 0) or (cull == "front" and area2 < 0):
                continue
            if area2 < 0:
                b, c, area2 = c, b, -area2
            (Ec, in_c), (Ea, in_a), (Eb, in_b) = edge(a, b), edge(b, c), edge(c, a)
            assert (Ea + Eb + Ec == area2).all()
            cov = in_a & in_b & in_c
            assert (Ea[cov] >= 0).all() and (Eb[cov] >= 0).all() and (Ec[cov] >= 0).all()
            with np.errstate(all="ignore"):
                depth = area2 / (Ea / a[2] + Eb / b[2] + Ec / c[2])
            cover[v, f], z64[v, f] = cov, np.where(cov, depth, np.nan)
            xs, ys = (a[0], b[0], c[0]), (a[1], b[1], c[1])
            in_x = (SX >= min(xs)) & (SX <= max(xs))
            in_y = (SY >= min(ys)) & (SY <= max(ys))
            boxes[v, f] = int(in_x.sum()) * int(in_y.sum())
            assert not (cov & ~(in_x & in_y)).any()                               # coverage implies the bounding box
    return cover, z64, front, boxes


def judge(depth, index, cover, z64, faces):
    """Every pixel of the GPU's maps against the statement; returns the figures, asserts nothing."""
    nv, h, w = depth.shape
    bound = REL_DEPTH * z64
    groups = {}
    for f, tri in enumerate(np.asarray(faces).tolist()):
        groups.setdefault(tuple(tri), []).append(f)
    filled = index >= 0
    bad = {"covers": 0, "depth": 0, "nearer": 0, "tie": 0, "empty": 0, "filled_is_nonzero": int((filled != (depth != 0)).sum()),
           "row": int((index >= len(faces)).sum())}
    worst = 0.0
    for v in range(nv):
        for y in range(h):
            for x in range(w):
                cov = np.nonzero(cover[v, :, y, x])[0]
                if not filled[v, y, x]:
                    bad["empty"] += int(len(cov) > 0)
                    continue
                n = int(index[v, y, x])
                if n >= len(faces) or not cover[v, n, y, x]:
                    bad["covers"] += 1
                    continue
                zn, bn = z64[v, n, y, x], bound[v, n, y, x]
                dev = abs(float(depth[v, y, x]) - zn) / bn
                worst = max(worst, dev)
                bad["depth"] += int(not dev <= 1.0)
                bad["nearer"] += int((z64[v, cov, y, x] < zn - (bn + bound[v, cov, y, x])).any())
                bad["tie"] += int(min(groups[tuple(np.asarray(faces)[n].tolist())]) < n)
    return bad, worst


def cameras():
    """The three cameras of tests/test_render.py: centre on the x axis, turned towards the scene."""
    f = 30.0
    K = np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    Es = []
    for cx, angle in ((0.0, 0.0), (-1.5, 0.15), (1.2, -0.12)):
        c, s = np.cos(angle), np.sin(angle)
        R = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
        Es.append(np.concatenate([R, (-R @ np.array([cx, 0.1 * cx, 0.0]))[:, None]], axis=1))
    return np.stack([K] * V), np.stack(Es)


def make_scene(seed=0):
    """``(vertices (Nv, 3) float32, faces (Nf, 3) int32, K, E, special)``: the scene of the module docstring, shuffled;
    ``special`` maps names to face rows."""
    rng = np.random.default_rng(seed)
    K, E = cameras()
    nx, ny = 14, 12
    gx, gy = np.meshgrid(np.linspace(-2.5, 2.5, nx), np.linspace(-2.0, 2.0, ny), indexing="ij")
    verts = [np.stack([gx.ravel(), gy.ravel(), 7.0 + 0.3 * np.sin(2.0 * gx.ravel()) * np.cos(2.0 * gy.ravel())], axis=1)]
    faces = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            v00, v10, v01, v11 = i * ny + j, (i + 1) * ny + j, i * ny + j + 1, (i + 1) * ny + j + 1
            faces += [(v00, v10, v11), (v00, v11, v01)]
    n_grid = len(faces)
    count = [nx * ny]

    def add(points, *tris):
        base = count[0]
        verts.append(np.asarray(points, np.float64))
        count[0] += len(points)
        faces.extend(tuple(base + i if i >= 0 else -1 - i for i in t) for t in tris)     # -1 - i: an absolute row

    plane = lambda x, y: (x, y, 10.0 + 0.1 * x + 0.05 * y)
    add([plane(-13, -9), plane(13, -9), plane(13, 9), plane(-13, 9)], (0, 1, 2), (0, 2, 3))                 # the back plane
    add([(-8, -1, 8.5), (-4, 0, 8.6), (-8, 1, 8.4)], (0, 1, 2))                                             # out on the left
    add([(8, -1, 8.5), (8, 1, 8.4), (4, 0.5, 8.6)], (0, 1, 2))                                              # on the right
    add([(0, -6, 8.5), (0.5, -2.5, 8.6), (-1, -6, 8.4)], (0, 1, 2))                                         # at the top
    add([(0.5, 6, 8.5), (-1.5, 6, 8.4), (0, 2.5, 8.6)], (0, 1, 2))                                          # at the bottom
    add([(20, 0, 8), (22, 1, 8), (21, 2, 8)], (0, 1, 2))                                                    # entirely outside
    add([(-1, -1, 7.5), (0, 0, 7.5), (1, 1, 7.5)], (0, 1, 2), (0, 0, 1))                                    # zero area
    add([(0, 0, -3.0)], (0, -1 - 5, -1 - 40))                                                               # behind the cameras
    add([(np.nan, 0, 8.0), (0, np.inf, 8.0)], (0, -1 - 7, -1 - 60), (1, -1 - 9, -1 - 80))                   # non-finite
    n_vert = count[0]
    faces += [(0, 1, n_vert), (-1, 2, 3)]                                                                   # rows that do not exist
    faces += [faces[i] for i in rng.choice(n_grid, 24, replace=False)]                                      # exact duplicates
    names = ["back0", "back1", "left", "right", "top", "bottom", "outside", "collinear", "repeated", "behind", "nan", "inf",
             "past_nv", "negative"]
    perm = rng.permutation(len(faces))
    faces = np.asarray(faces, np.int32)[perm]
    where = np.argsort(perm)
    special = {name: int(where[n_grid + k]) for k, name in enumerate(names)}
    assert len(faces) > 256 and len(faces) % 64 != 0
    return np.concatenate(verts).astype(np.float32), faces, K, E, special


@pytest.fixture(scope="module")
def scene():
    verts, faces, K, E, special = make_scene()
    return verts, faces, K, E, special, render.world_maps(K, E)


# the dyadic shapes of tests 2 and 5: camera f = 16, cx = cy = 0, vertices at multiples of 1/16 on Z = 2 (and, tilted, with Z in
# {2, 4}), so that every u * 256 is exact and image positions are multiples of half a pixel
def dyadic_camera():
    return np.array([[[16.0, 0.0, 0.0], [0.0, 16.0, 0.0], [0.0, 0.0, 1.0]]]), np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None]


def lift(pix, depths):
    """World points that the dyadic camera sees at the image positions ``pix`` (n, 2) at ``depths`` (n,)."""
    pix, depths = np.asarray(pix, np.float64), np.asarray(depths, np.float64)
    out = np.concatenate([pix * depths[:, None] / 16.0, depths[:, None]], axis=1).astype(np.float32)
    assert (out[:, :2].astype(np.float64) * 16.0 / depths[:, None] == pix).all()
    return out


def dyadic_shapes():
    """``{name: (pix (n, 2), faces, outline rows)}``: a fan around a pixel centre whose spokes run through pixel centres, and a
    strip between pixel corners whose diagonals do; both windings, and mirrored in x."""
    c = (20.5, 11.5)
    rim = [(28.5, 11.5), (26.5, 17.5), (20.5, 20.5), (14.5, 17.5), (12.5, 11.5), (14.5, 5.5), (20.5, 2.5), (26.5, 5.5)]
    fan = (np.array([c] + rim), [(0, 1 + k, 1 + (k + 1) % 8) for k in range(8)], list(range(1, 9)))
    top, bottom = [(2 + 6 * k, 2) for k in range(5)], [(10 + 6 * k, 10) for k in range(5)]
    tris = []
    for k in range(4):
        tris += [(k, 5 + k, k + 1), (k + 1, 5 + k, 5 + k + 1)]
    strip = (np.array(top + bottom, np.float64), tris, [0, 1, 2, 3, 4, 9, 8, 7, 6, 5])
    out = {}
    for name, (pix, tri, outline) in (("fan", fan), ("strip", strip)):
        for mirrored in (False, True):
            p = pix.copy()
            if mirrored:
                p[:, 0] = W - p[:, 0]
            for reverse in (False, True):
                t = [(a, c_, b) for a, b, c_ in tri] if reverse else list(tri)
                out["%s%s%s" % (name, "_mirrored" if mirrored else "", "_reversed" if reverse else "")] = (p, np.array(t, np.int32), outline)
    return out


def interior_and_ties(pix, faces, outline):
    """Boolean (H, W) maps, in exact float64 arithmetic on half-integers: pixel centres strictly inside the convex outline;
    those of them that lie on an edge of a face."""
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")

    def cross(p, q):
        return (q[0] - p[0]) * (ys - p[1]) - (q[1] - p[1]) * (xs - p[0])

    ring = [pix[i] for i in outline]
    sides = np.stack([cross(ring[k], ring[(k + 1) % len(ring)]) for k in range(len(ring))])
    inside = (sides > 0).all(0) | (sides < 0).all(0)
    on_edge = np.zeros((H, W), bool)
    for tri in faces:
        for k in range(3):
            p, q = pix[tri[k]], pix[tri[(k + 1) % 3]]
            between = (xs >= min(p[0], q[0])) & (xs <= max(p[0], q[0])) & (ys >= min(p[1], q[1])) & (ys <= max(p[1], q[1]))
            on_edge |= (cross(p, q) == 0) & between
    return inside, inside & on_edge


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2. CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_a_device_is_needed(scene):
    verts, faces, K, E = scene[:4]
    p, f = torch.from_numpy(verts), torch.from_numpy(faces)
    for bad in (verts, p.double(), p[:, :2], p[0], p.view(1, -1, 3)):
        with pytest.raises(ValueError, match="vertices"):
            render.render_mesh_depth_maps(bad, f, K, E, H, W)
        with pytest.raises(ValueError, match="vertices"):
            render.mesh_screen_coordinates(bad, K, E, H, W)
    for bad in (faces, f.float(), f[:, :2], f[0], f.to(torch.int16), None):
        with pytest.raises(ValueError, match="faces"):
            render.render_mesh_depth_maps(p, bad, K, E, H, W)
    for kw in (dict(height=-1, width=W), dict(height=H, width=2.5), dict(height=16385, width=W), dict(height=H, width=16385),
               dict(height=H, width=W, cull="both"), dict(height=H, width=W, cull=1), dict(height=H, width=W, lane_pixels=-1)):
        with pytest.raises(ValueError):
            render.render_mesh_depth_maps(p, f, K, E, **kw)
    with pytest.raises(ValueError):
        render.mesh_screen_coordinates(p, K, E, 16385, W)
    with pytest.raises(ValueError, match="intrinsics"):
        render.render_mesh_depth_maps(p, f, K[:2], E, H, W)
    with pytest.raises(RuntimeError, match="no CPU path"):
        render.render_mesh_depth_maps(p, f.long(), K, E, H, W)
    with pytest.raises(RuntimeError, match="no CPU path"):
        render.mesh_screen_coordinates(p, K, E, H, W)
    assert render.MESH_LANE_PIXELS in (16, 32, 64, 128)


def test_interpolate_vertex_attributes_on_hand_made_tensors():
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    attr = torch.tensor([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [8.0, 80.0]])
    index = torch.tensor([[[0, 1, -1], [1, 0, -1]]])
    bary = torch.zeros((1, 2, 3, 3))
    bary[0, 0, 0] = torch.tensor([1.0, 0.0, 0.0])
    bary[0, 0, 1] = torch.tensor([0.5, 0.25, 0.25])
    bary[0, 0, 2] = torch.tensor([0.3, 0.3, 0.4])                                   # empty: ignored
    bary[0, 1, 0] = torch.tensor([0.0, 0.0, 1.0])
    bary[0, 1, 1] = torch.tensor([0.25, 0.25, 0.5])
    out = render.interpolate_vertex_attributes(index, bary, faces, attr)
    assert out.shape == (1, 2, 3, 2) and out.dtype == torch.float32
    want = torch.tensor([[[1.0, 10.0], [0.5 * 4 + 0.25 * 2 + 0.25 * 8, 45.0], [0.0, 0.0]],
                         [[8.0, 80.0], [0.25 * 1 + 0.25 * 2 + 0.5 * 4, 27.5], [0.0, 0.0]]])[None]
    assert torch.equal(out, want)
    assert torch.equal(render.interpolate_vertex_attributes(index.int(), bary, faces.long(), attr), want)
    assert not render.interpolate_vertex_attributes(index, bary, faces[:0], attr).any()
    for bad in (dict(index=index.float()), dict(bary=bary[..., :2]), dict(faces=faces[:, :2]), dict(attributes=attr.double()),
                dict(attributes=attr[:, 0])):
        kw = dict(index=index, bary=bary, faces=faces, attributes=attr)
        kw.update(bad)
        with pytest.raises(ValueError):
            render.interpolate_vertex_attributes(**kw)


def test_statement_gives_every_interior_centre_to_exactly_one_face():
    K, E = dyadic_camera()
    proj = render.world_maps(K, E)
    ties = 0
    for name, (pix, faces, outline) in dyadic_shapes().items():
        inside, tie = interior_and_ties(pix, faces, outline)
        for depths in (np.full(len(pix), 2.0), np.where(np.arange(len(pix)) % 2 == 0, 2.0, 4.0)):
            xy, z, valid = table32(lift(pix, depths), proj, H, W)
            assert valid.all() and (xy[0] == np.rint(pix * 256).astype(np.int64)).all() and (z[0] == depths).all()
            cover, z64, front, _ = statement(xy, z, valid, faces, H, W)
            times = cover[0].sum(axis=0)
            assert (times[inside] == 1).all() and times.max() == 1, name
            assert front[0].all() or not front[0].any()
        print(name, "interior centres", int(inside.sum()), "of them on an edge or a vertex of a face", int(tie.sum()))
        assert inside.sum() >= 60 and tie.sum() >= 20
        ties += int(tie.sum())
    assert ties >= 8 * 20


def test_statement_scene_is_not_vacuous(scene):
    verts, faces, K, E, special, proj = scene
    xy, z, valid = table32(verts, proj, H, W)
    cover, z64, front, boxes = statement(xy, z, valid, faces, H, W)
    bound = REL_DEPTH * z64
    n_cover = cover.sum(axis=1)
    contested = 0
    for v, y, x in zip(*np.nonzero(n_cover >= 2)):
        zs, bs = z64[v, cover[v, :, y, x], y, x], bound[v, cover[v, :, y, x], y, x]
        order = np.argsort(zs)
        contested += int(zs[order[-1]] - zs[order[0]] > bs[order[-1]] + bs[order[0]])
    filled = n_cover >= 1
    print("filled", filled.mean(), "contested", contested / float(filled.sum()), "largest box", boxes.max())
    assert filled.mean() >= 0.5 and contested >= 0.1 * filled.sum()
    assert boxes[:, special["back0"]].min() > 4 * render.MESH_LANE_PIXELS and (boxes > 0).any(axis=0).sum() > 256
    assert 0 < (boxes[boxes > 0] <= render.MESH_LANE_PIXELS).sum() < (boxes > 0).sum()
    for name in ("outside", "repeated", "behind", "nan", "inf", "past_nv", "negative"):
        assert not cover[:, special[name]].any(), name
    tri = faces[special["collinear"]]
    a, b, c = xy[0, tri[0]], xy[0, tri[1]], xy[0, tri[2]]
    assert valid[0, tri].all() and (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) == 0
    for name in ("left", "right", "top", "bottom"):                                # in the map and out of it, in some view
        f = special[name]
        assert cover[:, f].any() and any(valid[v, faces[f]].all() and (xy[v, faces[f]].min() < 0 or xy[v, faces[f], 0].max() > 256 * W
                                         or xy[v, faces[f], 1].max() > 256 * H) for v in range(V)), name
    assert front.any() and not front.all()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _gpu_table(dev, verts, K, E, h=H, w=W, **kw):
    xy, z, valid = render.mesh_screen_coordinates(torch.from_numpy(np.ascontiguousarray(verts)).to(dev), K, E, h, w, **kw)
    assert xy.dtype == torch.int32 and z.dtype == torch.float32 and valid.dtype == torch.bool
    assert xy.shape == (len(K), len(verts), 2) and z.shape == valid.shape == (len(K), len(verts))
    return xy.cpu().numpy().astype(np.int64), z.cpu().numpy(), valid.cpu().numpy()


def _render(dev, verts, faces, K, E, h=H, w=W, **kw):
    faces = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(faces))
    depth, index, bary = render.render_mesh_depth_maps(torch.from_numpy(np.ascontiguousarray(verts)).to(dev), faces.to(dev), K, E,
                                                       h, w, return_index=True, return_barycentric=True, **kw)
    assert depth.dtype == torch.float32 and index.dtype == torch.int64 and bary.dtype == torch.float32
    assert depth.shape == index.shape == (len(K), h, w) and bary.shape == (len(K), h, w, 3)
    return depth.cpu().numpy(), index.cpu().numpy(), bary.cpu().numpy()


@pytest.fixture(scope="module")
def gpu_scene(dev, scene):
    """The random scene rendered once, with the statement on the GPU's own table: shared by tests 4, 8 and 10."""
    verts, faces, K, E, special, proj = scene
    xy, z, valid = _gpu_table(dev, verts, K, E)
    cover, z64, _, _ = statement(xy, z, valid, faces, H, W)
    depth, index, bary = _render(dev, verts, faces, K, E)
    return dict(xy=xy, z=z, valid=valid, cover=cover, z64=z64, depth=depth, index=index, bary=bary)


@pytest.mark.gpu
def test_screen_table_against_float64(dev):
    K, E = cameras()
    proj = render.world_maps(K, E)
    rng = np.random.default_rng(1)
    lo, hi = 2.0, 40.0
    inside = np.stack([rng.uniform(-6, 6, 300), rng.uniform(-4, 4, 300), rng.uniform(5, 12, 300)], axis=1)
    odd = np.array([[0.0, 0.0, -3.0], [1.0, 1.0, -0.5],                          # behind the cameras
                    [0.0, 0.0, 55.0], [3.0, -2.0, 90.0],                         # beyond depth_max
                    [0.2, 0.1, 0.8],                                             # nearer than depth_min
                    [4000.0, 0.0, 5.0], [0.0, -4000.0, 5.0], [-4000.0, 10.0, 5.0],   # outside the guard band
                    [-1500.0, 100.0, 9.0], [800.0, -900.0, 7.0],                 # outside the map, inside the guard band
                    [np.nan, 0.0, 8.0], [0.0, np.inf, 8.0], [0.0, 0.0, -np.inf]])
    verts = np.concatenate([inside, odd]).astype(np.float32)
    xy, z, valid = _gpu_table(dev, verts, K, E, depth_min=lo, depth_max=hi)
    g = project64(verts, proj)
    with np.errstate(invalid="ignore"):
        tests = [(g["z"] - float(np.float32(lo)), g["eps_z"]), (float(np.float32(hi)) - g["z"], g["eps_z"]),
                 (g["u"] + G, g["eps_u"]), (W + G - g["u"], g["eps_u"]), (g["v"] + G, g["eps_v"]), (H + G - g["v"], g["eps_v"])]
        margins, epses = np.stack([m for m, _ in tests]), np.stack([e for _, e in tests])
        finite = np.isfinite(verts).all(axis=1)[None, :] & np.ones((V, 1), bool)
        surely, surely_not = (margins > epses).all(axis=0), (margins < -epses).any(axis=0)
    assert (~finite | (surely != surely_not)).all()                               # clearly inside or clearly outside
    want = finite & surely
    assert np.array_equal(valid, want)
    assert want[:, :300].all() and not want[:, 300:308].any() and want[0, 308:310].all() and not want[:, 310:].any()
    assert (xy[~valid] == 0).all()
    ex = np.abs(xy[..., 0][valid] - 256.0 * g["u"][valid]) / (0.5 + 256.0 * g["eps_u"][valid])
    ey = np.abs(xy[..., 1][valid] - 256.0 * g["v"][valid]) / (0.5 + 256.0 * g["eps_v"][valid])
    ez = np.abs(z[valid] - g["z"][valid]) / g["eps_z"][valid]
    print("screen table: |xi - 256 u64| / bound", ex.max(), ey.max(), "|z - z64| / eps_z", ez.max())
    report("mesh_screen_table", xi_err_over_bound_max=max(ex.max(), ey.max()), z_err_over_eps_z_max=ez.max())
    assert ex.max() <= 1.0 and ey.max() <= 1.0 and ez.max() <= 1.0
    t_xy, t_z, t_valid = table32(verts, proj, H, W, lo, hi)                       # and the text in NumPy float32, to the bit
    assert np.array_equal(t_valid, valid) and np.array_equal(t_xy, xy) and np.array_equal(t_z[valid], z[valid])


@pytest.mark.gpu
def test_random_scene_teacher_forced(dev, scene, gpu_scene):
    verts, faces, K, E, special, proj = scene
    s = gpu_scene
    bad, worst = judge(s["depth"], s["index"], s["cover"], s["z64"], faces)
    filled = float((s["index"] >= 0).mean())
    print("violations", bad, "largest |depth - z64| / bound", worst, "filled", filled)
    report("mesh_random_scene", depth_err_over_bound_max=worst, filled_share=filled, **{"violations_" + k: v for k, v in bad.items()})
    assert all(v == 0 for v in bad.values()), bad
    assert worst <= 1.0 and filled >= 0.5
    won = set(np.unique(s["index"]).tolist())
    assert special["back0"] in won and special["left"] in won and len(won) > 100
    # int64 rows: one that would wrap into range as int32 must stay out of range
    wide = torch.from_numpy(faces).long()
    wide[special["past_nv"], 2] = 2 ** 32 + 5
    again = _render(dev, verts, wide, K, E)
    assert again[0].tobytes() == s["depth"].tobytes() and np.array_equal(again[1], s["index"])
    only = render.render_mesh_depth_maps(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), K, E, H, W)
    assert isinstance(only, torch.Tensor) and only.cpu().numpy().tobytes() == s["depth"].tobytes()
    # nothing to do: empty maps of the right shape, type and device
    p, f = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    for kw, shape in ((dict(v=p, f=f[:0], h=H, w=W), (V, H, W)), (dict(v=p[:0], f=f, h=H, w=W), (V, H, W)),
                      (dict(v=p, f=f, h=0, w=W), (V, 0, W)), (dict(v=p, f=f, h=H, w=0), (V, H, 0))):
        d, i, b = render.render_mesh_depth_maps(kw["v"], kw["f"], K, E, kw["h"], kw["w"], return_index=True, return_barycentric=True)
        assert d.shape == i.shape == shape and b.shape == shape + (3,) and d.device == p.device
        assert not d.any() and (i == -1).all() and not b.any()


@pytest.mark.gpu
def test_exactly_once_on_the_device(dev):
    K, E = dyadic_camera()
    for name, (pix, faces, outline) in dyadic_shapes().items():
        inside, _ = interior_and_ties(pix, faces, outline)
        for depths in (np.full(len(pix), 2.0), np.where(np.arange(len(pix)) % 2 == 0, 2.0, 4.0)):
            verts = torch.from_numpy(lift(pix, depths)).to(dev)
            times = np.zeros((H, W), np.int64)
            for tri in faces:
                d = render.render_mesh_depth_maps(verts, torch.from_numpy(tri[None]).to(dev), K, E, H, W)
                times += (d[0] > 0).cpu().numpy()
            assert (times[inside] == 1).all() and times.max() == 1, name
            whole = render.render_mesh_depth_maps(verts, torch.from_numpy(faces).to(dev), K, E, H, W)
            assert np.array_equal((whole[0] > 0).cpu().numpy(), times == 1)


@pytest.mark.gpu
def test_lane_wave_boundary(dev):
    S = render.MESH_LANE_PIXELS
    K, E = dyadic_camera()
    shapes = {16: ((5, 3), (3, 5), (17, 1), (8, 8)), 32: ((31, 1), (8, 4), (11, 3), (16, 8)), 64: ((9, 7), (8, 8), (13, 5), (16, 16)),
              128: ((127, 1), (16, 8), (43, 3), (32, 16))}[S]                     # S - 1, S, S + 1 and 4 S pixels
    assert [a * b for a, b in shapes] == [S - 1, S, S + 1, 4 * S]
    pix, depth_of, faces = [], [], []
    for k, (bw, bh) in enumerate(shapes):                                         # right triangles between pixel corners
        x0, y0 = 1 + 2 * k, 1 + k
        assert x0 + bw <= W and y0 + bh <= H
        faces.append((len(pix), len(pix) + 1, len(pix) + 2))
        pix += [(x0, y0), (x0 + bw, y0), (x0, y0 + bh)]
        depth_of += [2.0 + k, 3.0 + k, 2.5 + k]
    for x0, y0, ext, d in ((W - 6, H - 5, 20, 2.0), (W - 20, H - 10, 40, 9.0)):   # clipped by the map's corner: below and above S
        faces.append((len(pix), len(pix) + 1, len(pix) + 2))
        pix += [(x0, y0), (x0 + ext, y0), (x0, y0 + ext)]
        depth_of += [d, d + 1.0, d + 0.5]
    faces = np.array(faces, np.int32)
    verts = lift(pix, depth_of)
    xy, z, valid = _gpu_table(dev, verts, K, E)
    cover, z64, _, boxes = statement(xy, z, valid, faces, H, W)
    assert boxes[0].tolist() == [S - 1, S, S + 1, 4 * S, 30, 200]
    depth, index, bary = _render(dev, verts, faces, K, E)
    bad, worst = judge(depth, index, cover, z64, faces)
    print("lane / wave boundary: violations", bad, "largest |depth - z64| / bound", worst)
    report("mesh_lane_wave", depth_err_over_bound_max=worst, **{"violations_" + k: v for k, v in bad.items()})
    assert all(v == 0 for v in bad.values()) and worst <= 1.0
    assert set(np.unique(index).tolist()) == {-1, 0, 1, 2, 3, 4, 5}
    for lane_pixels in (0, S - 1, S + 1, 10 ** 6):                                # the result does not depend on S
        other = _render(dev, verts, faces, K, E, lane_pixels=lane_pixels)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(other, (depth, index, bary)))


@pytest.mark.gpu
def test_closed_form_planes(dev):
    f, cx, cy = 20.0, W / 2.0, H / 2.0
    K = np.array([[[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]]])
    E = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
    proj = render.world_maps(K, E)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    for name, d0, a, b in (("fronto_parallel", 7.25, 0.0, 0.0), ("tilted", 6.0, 0.25, -0.125)):
        corners = np.array([[-16.0, -8.0], [16.0, -8.0], [16.0, 8.0], [-16.0, 8.0]])
        verts = np.concatenate([corners, (d0 + a * corners[:, :1] + b * corners[:, 1:])], axis=1).astype(np.float32)
        assert (verts.astype(np.float64)[:, 2] == d0 + a * corners[:, 0] + b * corners[:, 1]).all()     # exactly on the plane
        g = project64(verts, proj)
        assert g["u"].min() < 0 and g["u"].max() > W and g["v"].min() < 0 and g["v"].max() > H          # the map lies inside
        closed = d0 / (1.0 - a * (xs - cx) / f - b * (ys - cy) / f)
        zmax = float(verts[:, 2].max())
        snap = zmax ** 2 * (abs(a) + abs(b)) / (f * d0) * (1.0 / 512.0 + max(g["eps_u"].max(), g["eps_v"].max()))
        bound = gamma(7) * (closed + snap) + snap
        depth, index, _ = _render(dev, verts, faces, K, E)
        ratio = np.abs(depth[0] - closed) / bound
        print(name, "largest |depth - closed form| / bound", ratio.max(), "bound", bound.max(), "of which snapping", snap)
        report("mesh_closed_form", plane=float(a != 0), depth_err_over_bound_max=ratio.max())
        assert (index >= 0).all() and ratio.max() <= 1.0


@pytest.mark.gpu
def test_determinism_and_permutation(dev, scene, gpu_scene):
    verts, faces, K, E, special, proj = scene
    s = gpu_scene
    again = _render(dev, verts, faces, K, E)
    assert all(a.tobytes() == s[k].tobytes() for a, k in zip(again, ("depth", "index", "bary")))
    perm = np.random.default_rng(7).permutation(len(faces))
    p_depth, p_index, _ = _render(dev, verts, faces[perm], K, E)
    assert p_depth.tobytes() == s["depth"].tobytes() and np.array_equal(p_index >= 0, s["index"] >= 0)
    filled = s["index"] >= 0
    rows, counts = np.unique(faces, axis=0, return_counts=True)
    repeated = {tuple(r) for r in rows[counts > 1].tolist()}
    single = filled & ~np.isin(s["index"], [f for f, tri in enumerate(faces.tolist()) if tuple(tri) in repeated])
    assert single.sum() > 0.5 * filled.sum() and (filled & ~single).any()
    assert np.array_equal(perm[p_index[single]], s["index"][single])
    assert np.array_equal(faces[perm][p_index[filled]], faces[s["index"][filled]])    # duplicates: the same triple


@pytest.mark.gpu
def test_culling(dev):
    from pointmvsnet_amd import tsdf
    from test_tsdf import sphere_volume
    f, wgt = sphere_volume(20, (9.6, 9.4, 9.5), 6.3)
    vertices, faces = tsdf.extract_mesh(torch.from_numpy(f).to(dev), torch.from_numpy(wgt).to(dev), (0.0, 0.0, 0.0), 1.0)[:2]
    assert len(faces) > 500
    K = np.array([[[50.0, 0.0, W / 2.0], [0.0, 50.0, H / 2.0], [0.0, 0.0, 1.0]]])
    E = np.concatenate([np.eye(3), np.array([[-9.5], [-9.5], [30.0]])], axis=1)[None]     # the camera at (9.5, 9.5, -30)
    maps = {cull: render.render_mesh_depth_maps(vertices, faces, K, E, H, W, cull=cull, return_index=True) for cull in (None, "back", "front")}
    maps = {k: (d.cpu().numpy(), i.cpu().numpy()) for k, (d, i) in maps.items()}
    assert 100 < (maps[None][0] > 0).sum() < H * W
    assert maps["back"][0].tobytes() == maps[None][0].tobytes() and np.array_equal(maps["back"][1], maps[None][1])
    far = maps["front"][0] > 0
    assert far.sum() > 100 and (maps[None][0][far] > 0).all() and (maps["front"][0][far] > maps[None][0][far]).all()
    # one face alone: each winding appears under exactly one of the two
    Kd, Ed = dyadic_camera()
    verts = torch.from_numpy(lift([(3, 2), (30, 4), (10, 20)], [2.0, 3.0, 4.0])).to(dev)
    seen = {}
    for order in ((0, 1, 2), (0, 2, 1)):
        tri = torch.tensor([order], dtype=torch.int32, device=dev)
        got = {cull: render.render_mesh_depth_maps(verts, tri, Kd, Ed, H, W, cull=cull).cpu().numpy() for cull in (None, "back", "front")}
        assert (got[None] > 0).sum() > 100
        shown = [cull for cull in ("back", "front") if got[cull].any()]
        assert len(shown) == 1 and got[shown[0]].tobytes() == got[None].tobytes()
        seen[order] = shown[0]
    assert seen == {(0, 1, 2): "front", (0, 2, 1): "back"}                        # area2 > 0 in x-right / y-down: not front-facing


@pytest.mark.gpu
def test_barycentrics(dev, scene, gpu_scene):
    verts, faces, K, E, special, proj = scene
    s = gpu_scene
    filled = s["index"] >= 0
    bary = s["bary"].astype(np.float64)
    assert not s["bary"][~filled].any()
    assert (s["bary"][filled] >= 0).all() and bary[filled].max() <= 1.0 + REL_BARY
    assert np.abs(bary[filled].sum(-1) - 1.0).max() <= REL_BARY
    assert (s["bary"][filled] > 0.01).all(axis=-1).sum() > 0.5 * filled.sum()      # not only corners
    worst = 0.0
    for v in range(V):
        corner_z = s["z"][v].astype(np.float64)[faces[s["index"][v][filled[v]]]]  # (n, 3): the table's z of the winner's corners
        got = (bary[v][filled[v]] * corner_z).sum(-1)
        worst = max(worst, float((np.abs(got - s["depth"][v][filled[v]]) / (REL_BARY * s["depth"][v][filled[v]])).max()))
    print("barycentrics: largest |sum bary z - depth| / (gamma_9 depth)", worst)
    report("mesh_barycentrics", z_from_bary_err_over_bound_max=worst)
    assert worst <= 1.0
    # the stored order: the weights move the stored corners' screen positions onto the pixel centre, up to perspective --
    # checked exactly instead on the dyadic fronto-parallel fan, where perspective-correct and screen-space weights agree
    Kd, Ed = dyadic_camera()
    for name in ("fan", "fan_reversed"):
        pix, tri, _ = dyadic_shapes()[name]
        d, i, b = _render(dev, lift(pix, np.full(len(pix), 2.0)), tri, Kd, Ed)
        ys, xs = np.nonzero(i[0] >= 0)
        back = (b[0, ys, xs].astype(np.float64)[..., None] * pix[tri[i[0, ys, xs]]]).sum(1)
        assert np.abs(back - np.stack([xs + 0.5, ys + 0.5], 1)).max() <= W * REL_BARY       # |pix| <= W, weights (1 + t9)
    # interpolate_vertex_attributes on the device against a NumPy gather in the same order of operations
    attr = np.random.default_rng(5).uniform(-1, 1, (len(verts), 4)).astype(np.float32)
    out = render.interpolate_vertex_attributes(torch.from_numpy(s["index"]).to(dev), torch.from_numpy(s["bary"]).to(dev),
                                               torch.from_numpy(faces).to(dev), torch.from_numpy(attr).to(dev)).cpu().numpy()
    corners = faces[np.maximum(s["index"], 0)]
    want = (s["bary"][..., 0, None] * attr[corners[..., 0]] + s["bary"][..., 1, None] * attr[corners[..., 1]]) \
        + s["bary"][..., 2, None] * attr[corners[..., 2]]
    want = np.where(filled[..., None], want, np.float32(0)).astype(np.float32)
    assert out.shape == (V, H, W, 4) and np.array_equal(out, want)


def _accumulate(dev, depths, K, E):
    """A ScanAccumulator that is handed ``depths`` (V, h, w) with full confidence, as tests/test_tsdf.py does."""
    from pointmvsnet_amd import scan as S
    nv, h, w = depths.shape
    cams = torch.zeros((nv, 2, 4, 4), dtype=torch.float64)
    cams[:, 0] = torch.eye(4, dtype=torch.float64)
    cams[:, 0, :3, :4] = torch.from_numpy(np.asarray(E, np.float64)[:, :3, :4])
    cams[:, 1, :3, :3] = torch.from_numpy(np.asarray(K, np.float64))
    acc = S.ScanAccumulator(nv, name="flow2", mode="NEAREST", keep_images=False)
    prob = torch.zeros((1, 5, h, w), device=dev)
    prob[:, 2] = 1.0
    for v in range(nv):
        order = [v] + [u for u in range(nv) if u != v]
        batch = {"img_list": torch.zeros((1, nv, 3, h, w)), "cam_params_list": cams[None, order]}
        preds = {"flow2": torch.from_numpy(depths[v])[None, None].to(dev), "flow2_prob": prob,
                 "coarse_prob_map": torch.ones((1, 1, h, w), device=dev)}
        acc.add(batch, preds, view_index=v)
    return acc


@pytest.mark.gpu
def test_ground_truth_from_a_mesh_has_no_holes(dev):
    """A front patch at depth 6 sampled 3 pixels apart before a back plane at depth 10, two cameras that differ by a
    translation along x (so both see the two depths unchanged).  As a cloud at splat 0 the patch is a sieve; as a mesh it is
    a surface."""
    f, cx, cy = 30.0, W / 2.0, H / 2.0
    K = np.stack([np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])] * 2)
    E = np.stack([np.concatenate([np.eye(3), np.array([[tx], [0.0], [0.0]])], axis=1) for tx in (0.0, -0.4)])
    front, back = 6.0, 10.0
    # the patch: image positions 3 pixels apart in view 0, from (9.5, 5.5) to (30.5, 17.5)
    px, py = np.meshgrid(np.arange(9.5, 31.0, 3.0), np.arange(5.5, 18.0, 3.0), indexing="ij")
    patch = np.stack([(px.ravel() - cx) * front / f, (py.ravel() - cy) * front / f, np.full(px.size, front)], axis=1)
    ny = px.shape[1]
    tris = []
    for i in range(px.shape[0] - 1):
        for j in range(ny - 1):
            tris += [(i * ny + j, (i + 1) * ny + j, (i + 1) * ny + j + 1), (i * ny + j, (i + 1) * ny + j + 1, i * ny + j + 1)]
    corners = np.array([[-20.0, -12.0, back], [20.0, -12.0, back], [20.0, 12.0, back], [-20.0, 12.0, back]])
    verts = np.concatenate([patch, corners]).astype(np.float32)
    faces = np.array(tris + [(len(patch), len(patch) + 1, len(patch) + 2), (len(patch), len(patch) + 2, len(patch) + 3)], np.int32)
    bx, by = np.meshgrid(np.arange(-8.0, 8.0, 0.1), np.arange(-5.0, 5.0, 0.1), indexing="ij")        # 0.3 pixel apart: no holes
    cloud = np.concatenate([patch, np.stack([bx.ravel(), by.ravel(), np.full(bx.size, back)], axis=1)]).astype(np.float32)
    # per view: the pixels whose centre lies inside the patch's outline shrunk by one pixel
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    inner = np.stack([(xs >= 9.5 + shift + 1) & (xs <= 30.5 + shift - 1) & (ys >= 5.5 + 1) & (ys <= 17.5 - 1)
                      for shift in (0.0, f * -0.4 / front)])
    assert inner.sum() > 300
    pred = np.where(inner, np.float32(front), np.float32(0))                     # the "prediction": the patch, only there
    acc = _accumulate(dev, pred, K, E)
    t = 1e-3                                  # far above the rasteriser's bound gamma_7 * 6 = 2.5e-6, far below the gap of 4
    as_cloud = acc.depth_errors(torch.from_numpy(cloud).to(dev), [t], splat=0, filtered=False)
    as_mesh = acc.depth_errors(torch.from_numpy(verts).to(dev), [t], filtered=False, gt_faces=torch.from_numpy(faces).to(dev))
    print("cloud at splat 0:", as_cloud["total"], "mesh:", as_mesh["total"])
    for row in as_cloud["per_view"]:                                             # the back plane shows through the patch
        assert row["n_compared"] == row["n_pred"] and row["within"][0] < 0.25 and row["abs_err_median"] > 3.9
    for row, n in zip(as_mesh["per_view"], inner.sum(axis=(1, 2))):
        assert row["n_pred"] == n and row["n_compared"] == n and row["n_gt"] == H * W and row["coverage"] == n / float(H * W)
        assert row["within"][0] == 1.0 and row["abs_err_mean"] <= gamma(7) * front
    depth = acc.render_mesh(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)).cpu().numpy()
    assert depth.shape == (2, H, W) and (depth > 0).all()                        # coverage 1.0: hole-free
    assert (np.abs(depth[inner] - front) <= gamma(7) * front).all()
    assert (np.abs(depth - back) <= gamma(7) * back)[~(np.abs(depth - front) <= gamma(7) * front)].all()
    again = acc.depth_errors(torch.from_numpy(cloud).to(dev), [t], splat=0, filtered=False, gt_faces=None)
    assert again == as_cloud


@pytest.mark.gpu
def test_scan_mesh_rendered_back_into_its_views(dev):
    """``render_mesh(*acc.mesh(...)[:2])`` on the plane scene of tests/test_fusion.py: wherever a view's map is filled, the
    point it back-projects to lies within ``trunc`` of the plane -- plus what the snapping (1/512 pixel + eps_u of image
    position, seen at depth z: z (1/512 + eps_u) sqrt(2) / f sideways) and the depth's rounding (gamma_7 z) move it."""
    from test_fusion import make_plane_scene
    depths, K, E, _, _ = make_plane_scene(5, sigma=0.0)
    depths = depths.copy()
    depths[depths > 700.0] = 0.0
    nv, h, w = depths.shape
    R0, t0 = E[0][:, :3], E[0][:, 3]
    n = R0.T @ np.array([0.15, -0.1, 1.0])
    n /= np.linalg.norm(n)
    c = n @ (np.linalg.inv(R0) @ (np.array([0.0, 0.0, 600.0]) - t0))
    acc = _accumulate(dev, depths, K, E)
    voxel = 4.0
    vertices, faces = acc.mesh(voxel, min_weight=2)[:2]
    depth, index = acc.render_mesh(vertices, faces, return_index=True)
    depth, index = depth.cpu().numpy(), index.cpu().numpy()
    assert depth.shape == (nv, h, w) and (index < len(faces)).all()
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], axis=-1)
    eps_u = float(max(project64(vertices.cpu().numpy(), render.world_maps(K, E))[k].max() for k in ("eps_u", "eps_v")))
    worst = 0.0
    for v in range(nv):
        got = depth[v] > 0
        assert got.mean() > 0.5
        ray = pix[got] @ np.linalg.inv(K[v]).T
        X = (ray * depth[v][got][:, None].astype(np.float64) - E[v][:3, 3]) @ E[v][:3, :3]           # R^-1 (ray d - t)
        z = depth[v][got].astype(np.float64)
        slack = z * (1.0 / 512.0 + eps_u) * np.sqrt(2.0) / min(K[v][0, 0], K[v][1, 1]) + gamma(7) * z * np.linalg.norm(ray, axis=1)
        worst = max(worst, float((np.abs(X @ n - c) / (4 * voxel + slack)).max()))
    print("the scan's mesh in its own views: farthest from the plane / (trunc + slack)", worst)
    assert worst <= 1.0
