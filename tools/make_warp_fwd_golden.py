"""Record what pf_frustum_variance_cl_f32 and pf_flow_features_f32 compute, bit for bit, as a test fixture.

    python tools/make_warp_fwd_golden.py [OUT.npz]          (default tests/golden/warp_fwd_parent_bits.npz)

Run ONCE on an MI355X at the commit whose kernels are the yardstick (the parent of the change that restructures them);
tests/test_gpu_warp_fwd_bits.py then holds every later kernel to these bits.  The file holds the seeded inputs and the
outputs; to stay under 1 MB it keeps each output once and this script CHECKS, on the recording kernels, the three
identities by which the test derives the other cases' expectations (it refuses to write the file if one fails):

  * the arithmetic of a channel does not depend on how many channels its map has: a level of c channels is the first c
    channels of the level's pool, so its output columns are the first c columns of the pool's -- the frustum cases C = 4
    and C = 68 share one recorded volume per V, the feature cases (16, 32, 64) and (36, 4, 68) one recorded block of
    36 + 32 + 68 columns per V;
  * ratio 2 is the row permutation of ratio 1 (feature row g * Ng + d hs ws + (y // 2) ws + x // 2 with
    g = (y % 2) * 2 + x % 2 is row d h w + y w + x): only ratio 1 is recorded;
  * the 24 trailing feature columns repeat xyz (column j holds axis j % 3): only xyz is recorded.

Frustum cases: B = 2, D = 3, H x W = 5 x 7 (N = 105 points: a block straddles rows and depth planes, the second block is
partial), V in {2, 3, 8} (the first V of eight views), generic cameras: taps leave the map in every view, and the nearest
depth plane of item 1 lies BEHIND view 1.  Feature cases: h x w = 6 x 10, V in {1, 3, 8}.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pointmvsnet_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR_B, FR_D, FR_H, FR_W, FR_VS, FR_CS = 2, 3, 5, 7, (2, 3, 8), (4, 68)
FT_H, FT_W, FT_VS, FT_WIDTHS, FT_POOL = 6, 10, (1, 3, 8), ((16, 32, 64), (36, 4, 68)), (36, 32, 68)
VMAX = 8


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis /= np.linalg.norm(axis)
    x, y, z = axis
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def _cameras(rng, H, W, near, behind_view=None, behind_z=0.0):
    """a reference camera and VMAX views around it: float64 (kinv, rinv, t, K (V, 3, 3), E (V, 3, 4)); baselines of
    0.3 .. 1.2 at focal ~ W give disparities of one to three texels at depth `near`"""
    f = 0.75 * W
    K0 = np.array([[f, 0.02, W / 2.0 + 0.13], [0.0, 1.03 * f, H / 2.0 - 0.21], [0.0, 0.0, 1.0]])
    R0 = _rot((0.3, 1.0, -0.2), 0.07)
    t0 = np.array([0.11, -0.07, 0.23])
    K, E = [], []
    for v in range(VMAX):
        Kv = K0.copy()
        Kv[0, 0] *= 1.0 + 0.03 * rng.standard_normal()
        Kv[1, 1] *= 1.0 + 0.03 * rng.standard_normal()
        Kv[:2, 2] += 0.4 * rng.standard_normal(2)
        Rv = R0 @ _rot(rng.standard_normal(3), 0.02 + 0.03 * v)
        tv = t0 + (0.0 if v == 0 else 1.0) * np.array([0.3 + 0.12 * v, -0.25 + 0.1 * v, 0.05 * rng.standard_normal()]) * (-1.0) ** v
        if v == behind_view:
            tv[2] = behind_z
        K.append(Kv)
        E.append(np.concatenate([Rv, tv.reshape(3, 1)], axis=1))
    return np.linalg.inv(K0), R0.T.copy(), t0, np.stack(K), np.stack(E)


def _coverage(kinv, rinv, t, depth_of_point, K, E, H, W):
    """float64 positions of the frustum's points in every view: (# points behind, # nw taps' cells partly outside,
    # wholly inside) per view"""
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    pix = np.stack([xs.reshape(-1), ys.reshape(-1), np.ones(H * W)])
    reps = depth_of_point.size // (H * W)
    world = rinv @ (np.tile(kinv @ pix, (1, reps)) * depth_of_point.reshape(1, -1) - t.reshape(3, 1))
    out = []
    for v in range(K.shape[0]):
        cam = E[v, :, :3] @ world + E[v, :, 3:]
        uv = K[v] @ (cam / cam[2:3])
        ix, iy = uv[0] - 0.5, uv[1] - 0.5
        x0, y0 = np.floor(ix), np.floor(iy)
        inside = (x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1)
        out.append((int((cam[2] < 0).sum()), int((~inside).sum()), int(inside.sum())))
    return out


def _call(name, *args):
    _lib.call(name, *(list(args) + [_lib.stream()]))
    torch.cuda.synchronize()


def frustum_inputs(z):
    """the frustum scene from the file's arrays: maps (B, 8, H * W, 68) and the six camera tensors"""
    pool = torch.from_numpy(z["pool2"])                                              # (8, 60, 68)
    maps = torch.stack([pool[:, :FR_H * FR_W], pool[:, 60 - FR_H * FR_W:]])          # (2, 8, 35, 68)
    return maps, [torch.from_numpy(z["fr_" + k]) for k in ("kinv", "rinv", "t", "depths", "K", "E")]


def run_frustum(dev, maps, cams, V, C):
    """cost (B, C, N), world (B, 3, N) on the CPU"""
    kinv, rinv, t, depths, K, E = cams
    N = FR_D * FR_H * FR_W
    d_maps = maps[:, :V, :, :C].contiguous().to(dev)
    d = [x.contiguous().to(dev) for x in (kinv, rinv, t, depths, K[:, :V], E[:, :V])]
    out = torch.full((FR_B * C * N,), float("nan"), device=dev)
    world = torch.full((FR_B * 3 * N,), float("nan"), device=dev)
    _call("pf_frustum_variance_cl_f32", _lib.ptr(d_maps), *([_lib.ptr(x) for x in d] +
          [_lib.ptr(out), _lib.ptr(world), FR_B, V, C, FR_H, FR_W, FR_D]))
    return out.cpu().view(FR_B, C, N), world.cpu().view(FR_B, 3, N)


def feature_levels(z, widths):
    """level l of a feature case: the first widths[l] channels of pool l, (8, h * w, c)"""
    return [torch.from_numpy(z["pool%d" % l])[:, :, :c] for l, c in enumerate(widths)]


def run_features(dev, levels, widths, V, depth, interval, cam, ratio):
    """feature (G * Ng, ctot), xyz (G, 3, Ng) on the CPU"""
    h, w = FT_H, FT_W
    G, Ng = ratio * ratio, 5 * (h // ratio) * (w // ratio)
    ctot = sum(widths) + 24
    d_lv = [m[:V].contiguous().to(dev) for m in levels]
    feat = torch.full((G * Ng * ctot,), float("nan"), device=dev)
    xyz = torch.full((G * 3 * Ng,), float("nan"), device=dev)
    d = [x.contiguous().to(dev) for x in (depth, interval, cam[:27 + 21 * V])]
    _call("pf_flow_features_f32", _lib.ptr(d_lv[0]), _lib.ptr(d_lv[1]), _lib.ptr(d_lv[2]), widths[0], widths[1], widths[2],
          V, h, w, _lib.ptr(d[0]), h, w, _lib.ptr(d[1]), _lib.ptr(d[2]), ratio, _lib.ptr(feat), _lib.ptr(xyz))
    return feat.cpu().view(G * Ng, ctot), xyz.cpu().view(G, 3, Ng)


def ratio2_rows(h, w):
    """(g, loc) of the ratio-2 layout for the ratio-1 rows d h w + y w + x in order"""
    d, y, x = torch.meshgrid(torch.arange(5), torch.arange(h), torch.arange(w), indexing="ij")
    hs, ws = h // 2, w // 2
    return ((y % 2) * 2 + x % 2).reshape(-1), (d * hs * ws + (y // 2) * ws + x // 2).reshape(-1)


def main(out_path=None, dev=None):
    out_path = out_path or os.path.join(ROOT, "tests", "golden", "warp_fwd_parent_bits.npz")
    dev = dev or torch.device("cuda:0")
    _lib.load()
    rng = np.random.default_rng(20260701)
    g = torch.Generator().manual_seed(20260701)
    z = {"pool%d" % l: torch.randn((VMAX, FT_H * FT_W, c), generator=g).numpy() for l, c in enumerate(FT_POOL)}

    # ---- frustum scene ----
    depths = np.array([[4.0, 5.5, 8.0], [3.0, 6.0, 7.5]])
    cams = [_cameras(rng, FR_H, FR_W, 3.0, behind_view=1 if b == 1 else None, behind_z=-3.3) for b in range(FR_B)]
    for b in range(FR_B):
        kinv, rinv, t, K, E = cams[b]
        cov = _coverage(kinv, rinv, t, np.repeat(depths[b], FR_H * FR_W), K, E, FR_H, FR_W)
        print("frustum item %d: (behind, partly outside, inside) per view" % b, cov)
        assert all(c[1] > 0 and c[2] > 0 for c in cov[1:]), "every warped view needs taps outside and inside the map"
        assert (cov[1][0] > 0) == (b == 1), "item 1's view 1 sees points from behind, nobody else does"
    z["fr_kinv"] = np.stack([c[0].reshape(9) for c in cams]).astype(np.float32)
    z["fr_rinv"] = np.stack([c[1].reshape(9) for c in cams]).astype(np.float32)
    z["fr_t"] = np.stack([c[2] for c in cams]).astype(np.float32)
    z["fr_depths"] = depths.astype(np.float32)
    z["fr_K"] = np.stack([c[3].reshape(VMAX, 9) for c in cams]).astype(np.float32)
    z["fr_E"] = np.stack([c[4].reshape(VMAX, 12) for c in cams]).astype(np.float32)
    maps, fcams = frustum_inputs(z)
    for V in FR_VS:
        cost, world = run_frustum(dev, maps, fcams, V, 68)
        assert bool(torch.isfinite(cost).all()) and bool(torch.isfinite(world).all())
        small, world4 = run_frustum(dev, maps, fcams, V, 4)
        assert torch.equal(small, cost[:, :4]) and torch.equal(world4, world), "C = 4 is not the first rows of C = 68"
        z["fr_cost_V%d" % V], z["fr_world_V%d" % V] = cost.numpy(), world.numpy()

    # ---- feature scene ----
    kinv, rinv, t, K, E = _cameras(rng, FT_H, FT_W, 6.0)
    prior = 6.0 + 1.5 * rng.random((FT_H, FT_W))
    interval = np.array([0.4])
    cov = _coverage(kinv, rinv, t, np.concatenate([(prior + interval[0] * (d - 2)).reshape(-1) for d in range(5)]), K, E,
                    FT_H, FT_W)
    print("features: (behind, partly outside, inside) per view", cov)
    assert all(c[1] > 0 and c[2] > 0 for c in cov)
    cam = np.zeros(27 + 21 * VMAX)
    cam[0:9], cam[9:18], cam[18:21] = kinv.reshape(9), rinv.reshape(9), t
    cam[21:24], cam[24:27] = (0.3, -0.2, 6.1), (1.7, 1.3, 0.9)
    for v in range(VMAX):
        cam[27 + 21 * v:36 + 21 * v], cam[36 + 21 * v:48 + 21 * v] = K[v].reshape(9), E[v].reshape(12)
    z["ft_depth"], z["ft_interval"], z["ft_cam"] = (prior.astype(np.float32), interval.astype(np.float32),
                                                    cam.astype(np.float32))
    ft = [torch.from_numpy(z[k]) for k in ("ft_depth", "ft_interval", "ft_cam")]
    gi, loc = ratio2_rows(FT_H, FT_W)
    Ng2 = 5 * (FT_H // 2) * (FT_W // 2)
    for V in FT_VS:
        block = torch.full((5 * FT_H * FT_W, sum(FT_POOL)), float("nan"))
        xyz1 = None
        for widths in FT_WIDTHS:
            f1, x1 = run_features(dev, feature_levels(z, widths), widths, V, *ft, 1)
            assert bool(torch.isfinite(f1).all()) and bool(torch.isfinite(x1).all())
            assert xyz1 is None or torch.equal(x1, xyz1), "xyz depends on the level widths"
            xyz1 = x1
            src = 0
            for l, c in enumerate(widths):
                dst = sum(FT_POOL[:l])
                cols = f1[:, src:src + c]
                seen = ~torch.isnan(block[:, dst:dst + c])
                assert torch.equal(block[:, dst:dst + c][seen], cols[seen]), "a channel's bits depend on its level's width"
                block[:, dst:dst + c] = cols
                src += c
            for j in range(24):
                assert torch.equal(f1[:, src + j], x1[0, j % 3]), "a trailing column does not repeat xyz"
            f2, x2 = run_features(dev, feature_levels(z, widths), widths, V, *ft, 2)
            assert torch.equal(f2.view(4, Ng2, -1)[gi, loc], f1) and torch.equal(x2[gi, :, loc], x1[0].t()), \
                "ratio 2 is not the row permutation of ratio 1"
        assert not bool(torch.isnan(block).any())
        z["ft_var_V%d" % V], z["ft_xyz_V%d" % V] = block.numpy(), xyz1[0].numpy()

    assert _lib.status() == 0
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **z)
    size = os.path.getsize(out_path)
    print("wrote", out_path, size, "bytes,", len(z), "arrays, library", _lib.load().pf_version().decode())
    assert size < 1000000, "the fixture must stay under 1 MB"


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
