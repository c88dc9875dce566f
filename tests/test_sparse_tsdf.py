"""Sparse TSDF volumes (pointmvsnet_amd/sparse_tsdf.py, csrc/sparse_tsdf.hip) against the dense volume of tsdf.py.

The yardstick is the dense path itself: with the allocation contract ``L <= A <= U`` of the module docstring the sparse
state equals the dense state on every allocated sample and, for ``min_weight >= 1``, the sparse mesh is the dense mesh.  So
every assertion here is an equality of bytes or an inclusion of sets; there is no tolerance anywhere.

``L`` (the bricks that hold a sample within Chebyshev distance 1 of a band sample) comes from ``CW > 0``: on the CPU from
``test_tsdf.statement_integrate`` (float64), on the GPU from the dense ``TSDFVolume`` itself, which is the definition.
``statement_upper`` is the float64 statement of ``U``, written from the docstring with no code shared with the product: the
brick test with doubled slack.

Scenes.  (a) the 5-view plane scene of test_fusion on 67 x 61 x 53 samples (no multiple of 8) with ``trunc = 2 voxel``;
(b) the same with a block of two views moved to 0.8 of its depth, a band of holes and one view perturbed by +-0.5 voxel;
(c) a virtual grid of 2048 x 2048 x 1024 samples, which the dense class refuses, with dyadic ``voxel`` and ``origin`` so
that a dense twin over the allocated bricks' bounding box has exactly the same sample positions; (d) no valid depth,
``dims = (5, 4, 3)``, exactly one brick, and a grid that contains view 0's camera.
"""
import numpy as np
import pytest
import torch

from test_fusion import _back_project, _pixel_centres, make_plane_scene
from test_tsdf import DEPTH_MIN, DEPTH_MAX, canonical, grid_of, plane_scene_box, statement_integrate
from pointmvsnet_amd import render

DIMS = (67, 61, 53)


# ---------------------------------------------------------------------------------------------------------------------
# the statements
# ---------------------------------------------------------------------------------------------------------------------
def brick_dims(dims):
    return tuple((n + 7) // 8 for n in dims)


def bricks_of_samples(mask):
    """(NBz, NBy, NBx) bool: the bricks that hold a sample of ``mask`` (nz, ny, nx)."""
    nz, ny, nx = mask.shape
    nbx, nby, nbz = brick_dims((nx, ny, nz))
    padded = np.zeros((nbz * 8, nby * 8, nbx * 8), bool)
    padded[:nz, :ny, :nx] = mask
    return padded.reshape(nbz, 8, nby, 8, nbx, 8).any(axis=(1, 3, 5))


def lower_set(band):
    """``L`` from the band samples (nz, ny, nx) bool: dilate by Chebyshev distance 1 inside the grid, then the bricks."""
    grown = np.zeros_like(band)
    nz, ny, nx = band.shape
    padded = np.pad(band, 1)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                grown |= padded[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    return bricks_of_samples(grown)


def statement_upper(depths, proj, origin, voxel, dims, trunc, depth_min=DEPTH_MIN, depth_max=DEPTH_MAX, bricks=None):
    """``U`` of the docstring in float64, fed what the kernel is fed (float32 origin, voxel, trunc, proj and depths): the box
    grown by two samples, the pixel box padded by two pixels, the z-interval widened by ``trunc (1 + 2^-10)``, the rounding
    margin doubled and the closeness guard at an eighth of a pixel.  (NBz, NBy, NBx) bool, or for ``bricks`` (n, 3) =
    (bi, bj, bk) rows a vector."""
    V, h, w = depths.shape
    o = np.asarray(origin, np.float32).astype(np.float64)
    vx, tr = float(np.float32(voxel)), float(np.float32(trunc))
    lo, hi = float(np.float32(depth_min)), float(np.float32(depth_max))
    nbx, nby, nbz = brick_dims(dims)
    if bricks is None:
        bk, bj, bi = np.meshgrid(np.arange(nbz), np.arange(nby), np.arange(nbx), indexing="ij")
        shape = bk.shape
        bricks = np.stack([bi.ravel(), bj.ravel(), bk.ravel()], axis=1)
    else:
        bricks = np.asarray(bricks, np.int64).reshape(-1, 3)
        shape = (len(bricks),)
    P = np.asarray(proj, np.float64).reshape(V, 3, 4)
    valid = [(depths[v] > lo) & (depths[v] < hi) for v in range(V)]
    d64 = depths.astype(np.float64)
    out = np.zeros(len(bricks), bool)
    corners = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)], np.float64)           # (8, 3)
    for n, b in enumerate(bricks):
        first, last = b * 8 - 2, b * 8 + 9
        pts = o + (first + corners * (last - first)) * vx                                          # (8, 3)
        for v in range(V):
            terms = P[v][None, :, :3] * pts[:, None, :]                                            # (8, 3 rows, 3)
            q = terms.sum(-1) + P[v][None, :, 3]
            mag = np.abs(terms).sum(-1) + np.abs(P[v][None, :, 3])
            z, Az, Aq = q[:, 2], mag[:, 2].max(), mag[:, :2].max()
            zlo, zhi = z.min(), z.max()
            m = 2.0 * 2.0 ** -20 * (Az + tr)
            if zhi + m <= lo or zlo - m >= hi:
                continue
            whole = zlo - m <= lo or not (2.0 ** -20 * (Aq + max(w, h) * Az) < zlo / 8.0)
            x0, x1, y0, y1 = 0, w - 1, 0, h - 1
            if not whole:
                u, t = q[:, 0] / z, q[:, 1] / z
                x0, x1 = max(int(np.floor(u.min())) - 2, 0), min(int(np.floor(u.max())) + 2, w - 1)
                y0, y1 = max(int(np.floor(t.min())) - 2, 0), min(int(np.floor(t.max())) + 2, h - 1)
            if x0 > x1 or y0 > y1:
                continue
            box = d64[v, y0:y1 + 1, x0:x1 + 1]
            pad = tr * (1.0 + 2.0 ** -10) + m
            if (valid[v][y0:y1 + 1, x0:x1 + 1] & (box >= zlo - pad) & (box <= zhi + pad)).any():
                out[n] = True
                break
    return out.reshape(shape)


def keys_of(brick_mask):
    """The sorted keys of a (NBz, NBy, NBx) bool mask: its flat indices, since the key is (bk NBy + bj) NBx + bi."""
    return np.flatnonzero(brick_mask.reshape(-1)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------
def _scene(damaged):
    depths, K, E, images, lo, hi = plane_scene_box()
    origin, voxel, _ = grid_of(lo, hi, DIMS)
    trunc = float(np.float32(2.0 * voxel))
    depths = depths.copy()
    if damaged:
        V, h, w = depths.shape
        rng = np.random.default_rng(7)
        for v in (1, 3):                                                            # a depth step in two views
            depths[v, h // 4:h // 2, w // 3:2 * w // 3] *= np.float32(0.8)
        depths[:, 2 * h // 3:2 * h // 3 + 3, :] = 0.0                               # a band of holes
        depths[2] += (np.where(rng.random((h, w)) < 0.5, -0.5, 0.5) * voxel).astype(np.float32) * (depths[2] > 0)
    proj = render.world_maps(K, E)
    return {"depths": depths, "K": K, "E": E, "images": images, "proj": proj, "origin": origin, "voxel": voxel,
            "trunc": trunc, "dims": DIMS}


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name, damaged in (("a", False), ("b", True)):
        s = _scene(damaged)
        st = statement_integrate(s["depths"], s["images"], s["proj"], s["origin"], s["voxel"], s["dims"], s["trunc"])
        s["L64"] = lower_set(st["CW"] > 0)
        s["U"] = statement_upper(s["depths"], s["proj"], s["origin"], s["voxel"], s["dims"], s["trunc"])
        out[name] = s
    return out


def degenerate_scenes():
    """Scene (d): name -> scene dict (the plane scene's views on other grids)."""
    depths, K, E, images, lo, hi = plane_scene_box()
    proj = render.world_maps(K, E)
    centre = (lo + hi) / 2.0
    out = {}

    def add(name, dims, voxel, origin=None, d=depths):
        voxel = float(np.float32(voxel))
        if origin is None:
            origin = centre - voxel * (np.asarray(dims) - 1) / 2.0
        out[name] = {"depths": d, "K": K, "E": E, "images": images, "proj": proj, "origin": np.asarray(origin, np.float32),
                     "voxel": voxel, "trunc": float(np.float32(2.0 * voxel)), "dims": dims}

    pitch = float(np.max((hi - lo) / 8.0))
    add("no_valid_depth", (19, 17, 11), pitch / 2.0, d=np.zeros_like(depths))
    add("dims_5_4_3", (5, 4, 3), pitch * 2.0)
    add("one_brick", (8, 8, 8), pitch)
    cam = -np.linalg.inv(E[0][:3, :3]) @ E[0][:3, 3]                                # view 0's centre, inside this grid
    dims = (20, 18, 22)
    voxel = float(np.float32(np.abs(centre - cam).max() * 2.4 / (min(dims) - 1)))
    add("camera_inside", dims, voxel, origin=(centre + cam) / 2.0 - voxel * (np.asarray(dims) - 1) / 2.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_lower_set_within_upper_set_and_neither_vacuous(scenes, name):
    s = scenes[name]
    L, U = s["L64"], s["U"]
    print(name, "virtual bricks", L.size, "L", int(L.sum()), "U", int(U.sum()))
    assert L.shape == U.shape == brick_dims(DIMS)[::-1]
    assert not (L & ~U).any()
    assert L.mean() >= 0.10 and U.mean() <= 0.50


def test_camera_inside_scene_contains_the_camera():
    """Scene (d)'s last case takes the whole-image branch: view 0's centre lies strictly inside the grid, so the brick that
    holds it has corners on both sides of the camera plane."""
    s = degenerate_scenes()["camera_inside"]
    o, vx = s["origin"].astype(np.float64), s["voxel"]
    cam = -np.linalg.inv(s["E"][0][:3, :3]) @ s["E"][0][:3, 3]
    assert (o + vx < cam).all() and (cam < o + vx * (np.asarray(s["dims"]) - 2)).all()


def test_arguments_are_checked_before_a_device_is_needed(scenes, monkeypatch):
    from pointmvsnet_amd import sparse_tsdf as T, tsdf
    ok = dict(origin=(0.0, 0.0, 0.0), voxel=1.0, dims=(4, 4, 4), trunc=3.0)
    for bad in (dict(voxel=0.0), dict(trunc=0.0), dict(trunc=float("nan")), dict(dims=(4, 4)), dict(dims=(4, 0, 4)),
                dict(dims=(4, 2.5, 4)), dict(origin=(0.0, 1.0)), dict(origin=(0.0, float("inf"), 0.0)),
                dict(dims=(2 ** 20 + 1, 4, 4)),                                       # more than 2^20 samples on an axis
                dict(dims=(2 ** 20, 2 ** 20, 2 ** 20)),                               # 2^60 samples
                dict(dims=(2 ** 20, 2 ** 20, 2 ** 16))):                              # 2^47 virtual bricks
        with pytest.raises(ValueError):
            T.SparseTSDFVolume(**dict(ok, **bad))
    with pytest.raises(ValueError):
        tsdf.TSDFVolume(**dict(ok, dims=(2048, 2048, 1024)))                          # the dense class refuses scene (c)
    big = T.SparseTSDFVolume(**dict(ok, dims=(2048, 2048, 1024)))                     # stated, not allocated
    assert big.virtual_bricks == 256 * 256 * 128 and big.report()["allocated_bricks"] == 0
    with pytest.raises(ValueError, match="2\\^31"):
        big.to_dense()
    s = scenes["a"]
    depths, K, E, images = torch.from_numpy(s["depths"]), s["K"], s["E"], torch.from_numpy(s["images"])
    vol, col = T.SparseTSDFVolume(**ok), T.SparseTSDFVolume(with_colour=True, **ok)
    for call in (vol.allocate, vol.integrate):
        with pytest.raises(ValueError, match="cameras"):
            call(depths, K[:3], E[:3])
        with pytest.raises(ValueError, match="depths must be"):
            call(depths[0], K, E)
        with pytest.raises(ValueError, match="depth_min"):
            call(depths, K, E, depth_min=5.0, depth_max=1.0)
    with pytest.raises(ValueError, match="images"):
        vol.integrate(depths, K, E, images=images)
    with pytest.raises(ValueError, match="images"):
        col.integrate(depths, K, E)
    col.views = tsdf.MAX_VIEWS_COLOUR - 4
    with pytest.raises(ValueError, match="overflow"):
        col.integrate(depths, K, E, images=images)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="min_weight"):
            vol.extract(min_weight=bad)
    late = T.SparseTSDFVolume(**ok)
    late._keys = torch.zeros((0,), dtype=torch.int64)                                 # as after a first integrate
    with pytest.raises(ValueError, match="integrated"):
        late.allocate(depths, K, E)
    crowded = T.SparseTSDFVolume(**dict(ok, dims=(40, 40, 40)), device="cpu")
    crowded._touched = torch.ones((crowded.virtual_bricks,), dtype=torch.uint8)
    monkeypatch.setattr(T, "MAX_BRICKS", 124)
    with pytest.raises(ValueError, match="125 bricks"):                               # the message names the brick count
        crowded.weight()


def test_kernels_are_built_bound_and_have_no_cpu_path(lib_built):
    import json
    from pointmvsnet_amd import _lib, build, sparse_tsdf as T
    names = {"pf_sparse_tsdf_touch", "pf_sparse_tsdf_neighbours", "pf_sparse_tsdf_integrate_f32",
             "pf_sparse_tsdf_count_triangles", "pf_sparse_tsdf_emit_triangles", "pf_sparse_tsdf_vertices_f32"}
    assert names <= set(_lib.PROTOTYPES) and "sparse_tsdf.hip" in build.SOURCES
    usage = json.load(open(build.USAGE_FILE))["sparse_tsdf.hip"]
    kernels = [k for k in usage if "sparse_tsdf_" in k]
    assert len(kernels) == 6
    for k in kernels:
        assert usage[k]["scratch_bytes_per_lane"] == 0, k
    vol = T.SparseTSDFVolume((0.0, 0.0, 0.0), 1.0, (3, 3, 3), 2.0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.integrate(torch.ones((1, 4, 4)), np.eye(3)[None], np.eye(4)[None])
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.allocate(torch.ones((1, 4, 4)), np.eye(3)[None], np.eye(4)[None])
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.extract()
    lib = _lib.load()                                                                 # limits are checked before any launch
    assert lib.pf_sparse_tsdf_neighbours(None, 0, 0, 4, 4, None, None) != 0
    assert lib.pf_sparse_tsdf_neighbours(None, 0, 2 ** 20 + 1, 4, 4, None, None) != 0
    assert lib.pf_sparse_tsdf_neighbours(None, 2 ** 22, 4, 4, 4, None, None) != 0     # more bricks than the state addresses
    assert lib.pf_sparse_tsdf_count_triangles(None, None, None, 0, 0, None, None) != 0   # min_weight 0
    assert lib.pf_sparse_tsdf_neighbours(None, 0, 4, 4, 4, None, None) == 0           # no bricks: nothing to do


# ---------------------------------------------------------------------------------------------------------------------
# 2. GPU
# ---------------------------------------------------------------------------------------------------------------------
def _tensors(dev, s):
    return torch.from_numpy(s["depths"]).to(dev), torch.from_numpy(s["images"]).to(dev)


def _sparse(dev, s, colour=True, allocate=(slice(None),), integrate=(slice(None),)):
    from pointmvsnet_amd import sparse_tsdf as T
    vol = T.SparseTSDFVolume(s["origin"], s["voxel"], s["dims"], s["trunc"], with_colour=colour, device=dev)
    depths, images = _tensors(dev, s)
    for chunk in allocate:
        vol.allocate(depths[chunk], s["K"][chunk], s["E"][chunk])
    for chunk in integrate:
        vol.integrate(depths[chunk], s["K"][chunk], s["E"][chunk], images=images[chunk] if colour else None)
    return vol


def _dense(dev, s, colour=True):
    from pointmvsnet_amd import tsdf
    vol = tsdf.TSDFVolume(s["origin"], s["voxel"], s["dims"], s["trunc"], with_colour=colour, device=dev)
    depths, images = _tensors(dev, s)
    return vol.integrate(depths, s["K"], s["E"], images=images if colour else None)


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def gpu_pairs(dev, scenes):
    """name -> (scene, dense volume, sparse volume), both integrated with colour, for (a), (b) and (d)."""
    out = {}
    for name, s in list(scenes.items()) + list(degenerate_scenes().items()):
        out[name] = (s, _dense(dev, s), _sparse(dev, s))
    return out


def _sample_mask(s, keys):
    """(nz, ny, nx) bool: the samples inside dims whose brick is among ``keys``."""
    nx, ny, nz = s["dims"]
    nbx, nby, nbz = brick_dims(s["dims"])
    bricks = np.zeros(nbx * nby * nbz, bool)
    bricks[keys] = True
    return np.repeat(np.repeat(np.repeat(bricks.reshape(nbz, nby, nbx), 8, 0), 8, 1), 8, 2)[:nz, :ny, :nx]


SCENES = ["a", "b", "no_valid_depth", "dims_5_4_3", "one_brick", "camera_inside"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_allocation_lies_between_the_lower_and_the_upper_set(dev, gpu_pairs, name):
    from pointmvsnet_amd import sparse_tsdf as T
    s, dense, sparse = gpu_pairs[name]
    keys = sparse.brick_keys().cpu().numpy()
    assert keys.dtype == np.int64 and (np.diff(keys) > 0).all()                       # sorted and unique
    nbx, nby, nbz = brick_dims(s["dims"])
    assert len(keys) == 0 or (keys[0] >= 0 and keys[-1] < nbx * nby * nbz)
    L = keys_of(lower_set(dense.CW.cpu().numpy() > 0))                                # the definition: the dense CW
    U = keys_of(s["U"]) if "U" in s else keys_of(
        statement_upper(s["depths"], s["proj"], s["origin"], s["voxel"], s["dims"], s["trunc"]))
    print(name, "virtual", nbx * nby * nbz, "L", len(L), "A", len(keys), "U", len(U))
    assert np.isin(L, keys).all() and np.isin(keys, U).all()
    if name == "no_valid_depth":
        assert len(keys) == 0
    elif name == "one_brick":
        assert list(keys) == [0]
    else:
        assert len(L) > 0
    coords = sparse.brick_coords().cpu().numpy()
    assert coords.shape == (len(keys), 3) and ((coords[:, 2] * nby + coords[:, 1]) * nbx + coords[:, 0] == keys).all()
    report = sparse.report()
    assert report["virtual_bricks"] == nbx * nby * nbz and report["allocated_bricks"] == len(keys)
    assert report["state_bytes"] == len(keys) * 512 * 24
    depths, _ = _tensors(dev, s)
    again = T.SparseTSDFVolume(s["origin"], s["voxel"], s["dims"], s["trunc"], device=dev).allocate(depths, s["K"], s["E"])
    assert _bytes(again.brick_keys()) == keys.tobytes()                               # two runs
    parts = T.SparseTSDFVolume(s["origin"], s["voxel"], s["dims"], s["trunc"], device=dev)
    parts.allocate(depths[:3], s["K"][:3], s["E"][:3]).allocate(depths[3:], s["K"][3:], s["E"][3:])
    assert _bytes(parts.brick_keys()) == keys.tobytes()                               # allocate(0..2) + allocate(3..4)
    parts.integrate(depths, s["K"], s["E"])
    with pytest.raises(ValueError, match="integrated"):
        parts.allocate(depths, s["K"], s["E"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_integration_gives_the_dense_bits_on_allocated_samples(dev, gpu_pairs, name):
    s, dense, sparse = gpu_pairs[name]
    keys = sparse.brick_keys().cpu().numpy()
    held = _sample_mask(s, keys)
    got = sparse.to_dense()
    for label, g, d in zip(("S", "W", "CS", "CW"), got, (dense.S, dense.W, dense.CS, dense.CW)):
        g, d = g.cpu().numpy(), d.cpu().numpy()
        assert g.dtype == d.dtype and g.shape == d.shape, label
        assert g[held].tobytes() == d[held].tobytes(), label                          # the dense bits where allocated
        assert not g[~held].any(), label                                              # zero elsewhere
    nb = len(keys)
    assert sparse.tsdf().shape == (nb, 8, 8, 8) and sparse.weight().shape == (nb, 8, 8, 8)
    assert sparse.colour().shape == (nb, 8, 8, 8, 3) and sparse.colour().dtype == torch.uint8
    if nb:                                                                            # the accessors are the dense expressions
        dense_f, dense_c = dense.tsdf().cpu().numpy(), dense.colour().cpu().numpy()
        coords = sparse.brick_coords().cpu().numpy()
        f, c = sparse.tsdf().cpu().numpy(), sparse.colour().cpu().numpy()
        nx, ny, nz = s["dims"]
        for b in (0, nb // 2, nb - 1):
            i0, j0, k0 = coords[b] * 8
            want = dense_f[k0:k0 + 8, j0:j0 + 8, i0:i0 + 8]
            kk, jj, ii = want.shape
            assert f[b, :kk, :jj, :ii].tobytes() == want.tobytes()
            assert c[b, :kk, :jj, :ii].tobytes() == dense_c[k0:k0 + 8, j0:j0 + 8, i0:i0 + 8].tobytes()
            assert (sparse.weight()[b].cpu().numpy()[kk:] == 0).all()                 # outside dims: never integrated
    if name in ("a", "b"):
        whole = [_bytes(t) for t in (sparse.S, sparse.W, sparse.CS, sparse.CW)]
        chunked = _sparse(dev, s, integrate=(slice(0, 3), slice(3, 5)))               # allocate(all), then two chunks
        assert [_bytes(t) for t in (chunked.S, chunked.W, chunked.CS, chunked.CW)] == whole
        own = _sparse(dev, s, allocate=())                                            # integrate allocates for its own views
        assert [_bytes(t) for t in (own.S, own.W, own.CS, own.CW)] == whole
        plain = _sparse(dev, s, colour=False)                                         # without colour: the same S and W
        assert plain.CS is None and plain.colour() is None and plain.to_dense()[2] is None
        assert [_bytes(plain.S), _bytes(plain.W)] == whole[:2]


def _same_mesh(sparse_mesh, dense_mesh, key_map=None):
    """Vertices, colours and (where both carry them) keys byte for byte, faces as multisets of rows; returns the faces."""
    sv, sf, sc = sparse_mesh[:3]
    dv, df, dc = dense_mesh[:3]
    assert sv.dtype == torch.float32 and sf.dtype == torch.int32 and sv.shape[1:] == (3,) and sf.shape[1:] == (3,)
    if len(sparse_mesh) > 3:
        sk, dk = sparse_mesh[3], dense_mesh[3].cpu().numpy()
        assert sk.dtype == torch.int64 and sv.shape[0] == sk.shape[0]
        assert sk.cpu().numpy().tobytes() == (dk if key_map is None else key_map(dk)).tobytes()
    assert _bytes(sv) == _bytes(dv)
    assert (sc is None) == (dc is None)
    if sc is not None:
        assert sc.dtype == torch.uint8 and _bytes(sc) == _bytes(dc)
    a, b = canonical(sf.cpu().numpy()), canonical(df.cpu().numpy())
    assert a.shape == b.shape and sorted(map(tuple, a)) == sorted(map(tuple, b))      # equal as multisets of rows
    return len(a)


@pytest.mark.gpu
@pytest.mark.parametrize("min_weight", [1, 3])
@pytest.mark.parametrize("name", SCENES)
def test_extraction_is_the_dense_mesh(dev, gpu_pairs, name, min_weight):
    s, dense, sparse = gpu_pairs[name]
    mesh = sparse.extract(min_weight)
    faces = _same_mesh(mesh, dense.extract(min_weight))
    print(name, "min_weight", min_weight, "vertices", len(mesh[3]), "faces", faces)
    if name in ("a", "b", "camera_inside"):
        assert faces > 0
    if name == "no_valid_depth":
        assert faces == 0 and mesh[0].shape == (0, 3) and mesh[1].shape == (0, 3) and mesh[2].shape == (0, 3)
    if name == "b":                                                                   # the halo: a cell over several bricks
        keys = mesh[3].cpu().numpy()
        nx, ny, nz = s["dims"]
        a = keys >> 3
        i, j, k = a % nx, (a // nx) % ny, a // (nx * ny)
        crossing = ((i + (keys & 1)) >> 3 != i >> 3) | ((j + ((keys >> 1) & 1)) >> 3 != j >> 3) | \
                   ((k + ((keys >> 2) & 1)) >> 3 != k >> 3)
        assert crossing.any()                                                         # an edge, hence a cell, in two bricks
    plain = _sparse(dev, s, colour=False).extract(min_weight) if name == "a" else None
    if plain is not None:
        assert plain[2] is None and torch.equal(plain[0], mesh[0]) and torch.equal(plain[1], mesh[1])


def _common_window(depths, K, E):
    """``(point, window)``: the first point of view 0's plane (on a coarse pixel grid) that every view sees at least two
    pixels inside its map with neither hole nor outlier around it, and the depth maps with only the 3 x 3 pixels around it."""
    V, h, w = depths.shape
    pix = _pixel_centres(h, w)
    for y0 in range(8, h - 8, 8):
        for x0 in range(8, w - 8, 8):
            if not 0.0 < depths[0][y0, x0] < 700.0:
                continue
            point = _back_project(K[0], E[0], pix[y0, x0], depths[0][y0, x0])
            q = [K[v] @ (E[v][:3, :3] @ point + E[v][:3, 3]) for v in range(V)]
            at = [(int(np.floor(c[1] / c[2])), int(np.floor(c[0] / c[2]))) for c in q]
            if not all(2 <= y < h - 2 and 2 <= x < w - 2 for y, x in at):
                continue
            rows = [(v, slice(y - 1, y + 2), slice(x - 1, x + 2)) for v, (y, x) in enumerate(at)]
            if all(((depths[r] > 0) & (depths[r] < 700.0)).all() for r in rows):
                window = np.zeros_like(depths)
                for r in rows:
                    window[r] = depths[r]
                return point, window
    raise AssertionError("no point of the plane is seen by every view")


@pytest.mark.gpu
def test_virtual_grid_beyond_the_dense_limit(dev):
    """Scene (c): 2048 x 2048 x 1024 samples of pitch 0.5.  Only a small window of every depth map is kept, so the surface
    sits in a few dozen bricks (3 x 3 pixels per view around one point of the plane); the dense twin covers their bounding box with the same sample positions (everything dyadic)."""
    from pointmvsnet_amd import sparse_tsdf as T, tsdf
    depths, K, E, images, _ = make_plane_scene(5, sigma=0.0)
    V, h, w = depths.shape
    point, window = _common_window(depths, K, E)
    assert (window > 0).sum() == 9 * V
    dims, voxel, trunc = (2048, 2048, 1024), 0.5, 1.0
    origin = np.round((point - voxel * (np.asarray(dims) - 1) / 2.0) / 4.0) * 4.0     # a multiple of 4
    s = {"depths": window, "K": K, "E": E, "images": images, "origin": origin.astype(np.float32), "voxel": voxel,
         "trunc": trunc, "dims": dims}
    with pytest.raises(ValueError):
        _dense(dev, s)
    sparse = _sparse(dev, s)
    coords = sparse.brick_coords().cpu().numpy()
    print("scene (c):", sparse.report(), "bounding box of bricks", coords.min(0), coords.max(0))
    assert 12 <= len(coords) <= 600
    first, last = coords.min(0), coords.max(0)
    twin = dict(s, origin=(origin + first * 8 * voxel).astype(np.float32), dims=tuple(int(n) for n in (last - first + 1) * 8))
    assert (twin["origin"].astype(np.float64) == origin + first * 8 * voxel).all()
    assert twin["dims"][0] * twin["dims"][1] * twin["dims"][2] <= 2 ** 19
    dense = _dense(dev, twin)

    def to_virtual(keys):
        tx, ty, _ = twin["dims"]
        a = keys >> 3
        i, j, k = a % tx + first[0] * 8, (a // tx) % ty + first[1] * 8, a // (tx * ty) + first[2] * 8
        return ((k * dims[1] + j) * dims[0] + i) * 8 + (keys & 7)

    for min_weight in (1, 3):
        faces = _same_mesh(sparse.extract(min_weight), dense.extract(min_weight), to_virtual)
        assert faces > 0


@pytest.mark.gpu
def test_scan_accumulator_mesh_sparse(dev, tmp_path):
    """``ScanAccumulator.mesh(sparse=True)`` is the mesh of ``sparse=False``; the default call is the dense route."""
    from pointmvsnet_amd import scan as S
    from pointmvsnet_amd.utils import io as IO
    depths, K, E, images, cams = make_plane_scene(5, sigma=0.0)
    depths = depths.copy()
    depths[depths > 700.0] = 0.0
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
    default = acc.mesh(4.0, min_weight=2)
    dense = acc.mesh(4.0, min_weight=2, sparse=False)
    assert all(_bytes(a) == _bytes(b) for a, b in zip(default, dense))                # the default is the dense route
    sparse = acc.mesh(4.0, min_weight=2, sparse=True)
    assert len(sparse) == 3 and _same_mesh(sparse, dense) > 1000
    assert acc.last_sparse_report["allocated_bricks"] > 0
    assert acc.last_sparse_report["state_bytes"] < acc.last_sparse_report["dense_state_bytes"]
    with_normals = acc.mesh(4.0, min_weight=2, sparse=True, keep_largest=1, with_normals=True)
    assert len(with_normals) == 4 and with_normals[3].shape == with_normals[0].shape
    path = str(tmp_path / "mesh.ply")
    written = acc.write_mesh(path, voxel=4.0, min_weight=2, sparse=True)
    p, col, nrm, f = IO.load_ply_mesh(path)
    assert (p == written[0].cpu().numpy()).all() and (f == written[1].cpu().numpy()).all()
    assert _bytes(written[0]) == _bytes(dense[0])
