"""pf_frustum_variance_cl_f32 and pf_flow_features_f32 (csrc/fetch.hip) bit for bit against what the kernels computed BEFORE
they took 32-bit tap offsets on a uniform base and the coarse warp began to project once per block: the fixture
tests/golden/warp_fwd_parent_bits.npz was recorded on an MI355X at the parent commit by tools/make_warp_fwd_golden.py (seeded
inputs and outputs; the script's docstring describes the scenes).  The restructured kernels make the same pf_project_taps /
pf_bilerp / pf_variance calls on the same inputs and sum the views in the same order, so every comparison is torch.equal.

To stay under 1 MB the fixture holds each output once; the expectations of the other cases follow by three identities
that the script verified ON THE RECORDING KERNELS before it wrote the file: a channel's bits do not depend on how many
channels its map has (C = 4 is the first four rows of C = 68; the levels of (16, 32, 64) and (36, 4, 68) are the leading
columns of one recorded 36 + 32 + 68 block), ratio 2 is the row permutation of ratio 1, and the 24 trailing feature columns
repeat xyz.

The second half is the addressing bound of the 32-bit form (h w < 2^24 texels, 4 C < 2^24 bytes per texel, 4 C h w < 2^32 bytes per
view and level): both entry points answer PF_ERR_UNSUPPORTED beyond it before launching anything, and the widest texels a few
MB can hold still address every channel.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, report
from pointmvsnet_amd import _lib

pytestmark = pytest.mark.gpu

F32 = torch.float32
NAN = float("nan")
SENT = -7777.25
GUARD = 1024
PF_OK, PF_ERR_UNSUPPORTED = 0, -2
FR_B, FR_D, FR_H, FR_W = 2, 3, 5, 7
FT_H, FT_W, FT_POOL = 6, 10, (36, 32, 68)


@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(os.path.join(GOLDEN_DIR, "warp_fwd_parent_bits.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _raw(name, *args):
    code = getattr(_lib.load(), name)(*(list(args) + [_lib.stream()]))
    torch.cuda.synchronize()
    return int(code)


def _guarded(n, dev, fill=NAN):
    buf = torch.full((n + GUARD,), fill, dtype=F32)
    buf[n:] = SENT
    return buf.to(dev)


def _take(buf, n, what):
    host = buf.cpu()
    assert bool((host[n:] == SENT).all()), "%s: written beyond its %d elements" % (what, n)
    return host[:n]


# ---------------------------------------------------------------------------------------------
# the coarse warp
# ---------------------------------------------------------------------------------------------
def _frustum_scene():
    z = _fixture()
    pool = z["pool2"]                                                                # (8, 60, 68)
    maps = torch.stack([pool[:, :FR_H * FR_W], pool[:, 60 - FR_H * FR_W:]])          # (B, 8, H W, 68)
    return maps, [z["fr_" + k] for k in ("kinv", "rinv", "t", "depths", "K", "E")]


def _frustum(dev, maps, cams, V, H, W, D, want=PF_OK):
    """maps (B, V, H W, C) -> cost (B, C, N), world (B, 3, N); every element written, nothing behind them"""
    kinv, rinv, t, depths, K, E = cams
    B, C, N = maps.shape[0], maps.shape[3], D * H * W
    d_maps = maps.contiguous().to(dev)
    d = [x.contiguous().to(dev) for x in (kinv, rinv, t, depths, K[:, :V], E[:, :V])]
    out, world = _guarded(B * C * N, dev), _guarded(B * 3 * N, dev)
    code = _raw("pf_frustum_variance_cl_f32", _lib.ptr(d_maps), *([_lib.ptr(x) for x in d] +
                [_lib.ptr(out), _lib.ptr(world), B, V, C, H, W, D]))
    assert code == want, code
    cost, wpts = _take(out, B * C * N, "cost volume").view(B, C, N), _take(world, B * 3 * N, "world").view(B, 3, N)
    assert not bool(torch.isnan(cost).any()) and not bool(torch.isnan(wpts).any()), "an element was not written"
    return cost, wpts


@pytest.mark.parametrize("C", [4, 68])
@pytest.mark.parametrize("V", [2, 3, 8])
def test_frustum_variance_cl_keeps_the_parents_bits(dev, V, C):
    """B = 2, D = 3, 5 x 7: N = 105 = 64 + 41 -- the first block straddles map rows and a depth plane, the second is partial
    and its shadow points repeat the last one.  V = 8 parks 64 * 7 = 448 (point, view) pairs with 256 threads (the prologue
    loops), C = 68 runs a second 64-channel round on the parked taps.  Taps leave the map in every view; the nearest plane
    of item 1 lies behind its view 1 (the script that recorded the fixture asserts both)."""
    z = _fixture()
    assert (FR_D * FR_H * FR_W) % 64 != 0
    maps, cams = _frustum_scene()
    cost, world = _frustum(dev, maps[:, :V, :, :C], cams, V, FR_H, FR_W, FR_D)
    assert torch.equal(world, z["fr_world_V%d" % V]), "world points"
    want = z["fr_cost_V%d" % V][:, :C]
    assert torch.equal(cost, want), ("cost volume", int((cost != want).sum()), float((cost - want).abs().max()))
    assert _lib.status() == 0
    report("frustum_cl_parent_bits_V%d_C%d" % (V, C), mismatches=0.0)


# ---------------------------------------------------------------------------------------------
# feature assembly
# ---------------------------------------------------------------------------------------------
def _features(dev, levels, widths, V, h, w, depth, interval, cam, ratio, want=PF_OK):
    """levels: three (V, h w, c) tensors -> feature (G Ng, ctot), xyz (G, 3, Ng)"""
    G, Ng = ratio * ratio, 5 * (h // ratio) * (w // ratio)
    ctot = sum(widths) + 24
    d_lv = [m[:V].contiguous().to(dev) for m in levels]
    feat, xyz = _guarded(G * Ng * ctot, dev), _guarded(G * 3 * Ng, dev)
    d = [x.contiguous().to(dev) for x in (depth, interval, cam[:27 + 21 * V])]
    code = _raw("pf_flow_features_f32", _lib.ptr(d_lv[0]), _lib.ptr(d_lv[1]), _lib.ptr(d_lv[2]), widths[0], widths[1], widths[2],
                V, h, w, _lib.ptr(d[0]), int(depth.shape[0]), int(depth.shape[1]), _lib.ptr(d[1]), _lib.ptr(d[2]), ratio,
                _lib.ptr(feat), _lib.ptr(xyz))
    assert code == want, code
    f, x = _take(feat, G * Ng * ctot, "feature").view(G * Ng, ctot), _take(xyz, G * 3 * Ng, "xyz").view(G, 3, Ng)
    assert not bool(torch.isnan(f).any()) and not bool(torch.isnan(x).any()), "an element of feature / xyz was not written"
    return f, x


def _feature_scene():
    z = _fixture()
    return [z["pool%d" % l] for l in range(3)], (z["ft_depth"], z["ft_interval"], z["ft_cam"])


@pytest.mark.parametrize("ratio", [1, 2])
@pytest.mark.parametrize("widths", [(16, 32, 64), (36, 4, 68)])
@pytest.mark.parametrize("V", [1, 3, 8])
def test_flow_features_keep_the_parents_bits(dev, V, widths, ratio):
    """6 x 10: the 4 x 8 patches are partial in both directions.  (16, 32, 64) is the model's pyramid (the 16-channel level
    uses four of a point's eight lanes); (36, 4, 68) has a second chunk with one live lane, a level of one lane and a third
    chunk.  Level l holds the first widths[l] channels of the fixture's pool l; the expected columns are the recorded
    block's, row-permuted into the sub-grid order for ratio 2, followed by xyz eight times."""
    z = _fixture()
    h, w = FT_H, FT_W
    pools, (depth, interval, cam) = _feature_scene()
    levels = [p[:, :, :c] for p, c in zip(pools, widths)]
    feat, xyz = _features(dev, levels, widths, V, h, w, depth, interval, cam, ratio)
    block, x1 = z["ft_var_V%d" % V], z["ft_xyz_V%d" % V]                              # (5 h w, 136), (3, 5 h w): ratio-1 order
    cols = [block[:, sum(FT_POOL[:l]):sum(FT_POOL[:l]) + c] for l, c in enumerate(widths)]
    want = torch.cat(cols + [x1.t()] * 8, dim=1)
    d, y, x = torch.meshgrid(torch.arange(5), torch.arange(h), torch.arange(w), indexing="ij")
    hs, ws = h // ratio, w // ratio
    gi = ((y % ratio) * ratio + x % ratio).reshape(-1)
    loc = (d * hs * ws + (y // ratio) * ws + x // ratio).reshape(-1)
    got = feat.view(ratio * ratio, 5 * hs * ws, -1)[gi, loc]                          # the ratio-1 rows in order
    assert torch.equal(xyz[gi, :, loc], x1.t()), "xyz"
    assert torch.equal(got, want), ("feature rows", int((got != want).sum()), float((got - want).abs().max()))
    assert _lib.status() == 0
    report("flow_features_parent_bits_V%d_c%d_%d_%d_r%d" % ((V,) + tuple(widths) + (ratio,)), mismatches=0.0)


# ---------------------------------------------------------------------------------------------
# the addressing bound
# ---------------------------------------------------------------------------------------------
# texels < 2^24, 4 C < 2^24, 4 C texels < 2^32: (H, W, C) just beyond each term and just inside it
_BEYOND = [(4096, 4096, 4), (1024, 1024, 1024), (2, 2, 1 << 22)]
_INSIDE = [(4096, 4095, 4), (1024, 1023, 1024), (2, 2, (1 << 22) - 4), (65536, 255, 64)]


def test_frustum_variance_cl_rejects_maps_beyond_the_bound_before_launching(dev):
    """Sizes beyond the bound with small real buffers: PF_ERR_UNSUPPORTED and the outputs keep their fill.  The check
    stands before the entry point's empty-volume return, so D = 0 shows its arithmetic from both sides without memory: PF_OK
    just inside each term, PF_ERR_UNSUPPORTED just beyond.  The device stays usable: the fixture's V = 3, C = 4 case follows."""
    maps, cams = _frustum_scene()
    kinv, rinv, t, depths, K, E = [x.contiguous().to(dev) for x in cams]
    d_maps = maps.contiguous().to(dev)
    out, world = torch.full((4096,), SENT).to(dev), torch.full((4096,), SENT).to(dev)

    def code(H, W, C, D):
        return _raw("pf_frustum_variance_cl_f32", _lib.ptr(d_maps), _lib.ptr(kinv), _lib.ptr(rinv), _lib.ptr(t), _lib.ptr(depths),
                    _lib.ptr(K), _lib.ptr(E), _lib.ptr(out), _lib.ptr(world), 2, 3, C, H, W, D)

    for H, W, C in _BEYOND:
        assert not (H * W < 2 ** 24 and 4 * C < 2 ** 24 and 4 * C * H * W < 2 ** 32)
        assert code(H, W, C, 3) == PF_ERR_UNSUPPORTED, (H, W, C)
        assert code(H, W, C, 0) == PF_ERR_UNSUPPORTED, (H, W, C)
    for H, W, C in _INSIDE:
        assert H * W < 2 ** 24 and 4 * C < 2 ** 24 and 4 * C * H * W < 2 ** 32
        assert code(H, W, C, 0) == PF_OK, (H, W, C)
    assert bool((out.cpu() == SENT).all()) and bool((world.cpu() == SENT).all())
    assert _lib.status() == 0
    cost, _ = _frustum(dev, maps[:, :3, :, :4], cams, 3, FR_H, FR_W, FR_D)
    assert torch.equal(cost, _fixture()["fr_cost_V3"][:, :4])
    report("frustum_cl_bound_rejections", launched=0.0)


def test_flow_features_reject_maps_beyond_the_bound_before_launching(dev):
    """The same three terms per non-empty level (in turn the first, second and third level is the one beyond): PF_ERR_UNSUPPORTED,
    outputs untouched; then the fixture's V = 3 ratio-1 case runs and gives its bits."""
    pools, (depth, interval, cam) = _feature_scene()
    d_map = pools[2][:3].contiguous().to(dev)
    d = [x.contiguous().to(dev) for x in (depth, interval, cam[:27 + 21 * 3])]
    feat, xyz = torch.full((4096,), SENT).to(dev), torch.full((4096,), SENT).to(dev)
    for i, (h, w, c) in enumerate(_BEYOND):
        widths = [4, 4, 4]
        widths[i] = c
        got = _raw("pf_flow_features_f32", _lib.ptr(d_map), _lib.ptr(d_map), _lib.ptr(d_map), widths[0], widths[1], widths[2], 3, h, w,
                   _lib.ptr(d[0]), FT_H, FT_W, _lib.ptr(d[1]), _lib.ptr(d[2]), 1, _lib.ptr(feat), _lib.ptr(xyz))
        assert got == PF_ERR_UNSUPPORTED, (h, w, widths)
    assert bool((feat.cpu() == SENT).all()) and bool((xyz.cpu() == SENT).all())
    assert _lib.status() == 0
    widths = (16, 32, 64)
    f, _ = _features(dev, [p[:, :, :c] for p, c in zip(pools, widths)], widths, 3, FT_H, FT_W, depth, interval, cam, 1)
    block = _fixture()["ft_var_V3"]
    assert torch.equal(f[:, :16], block[:, :16]) and torch.equal(f[:, 48:112], block[:, 68:132])
    report("flow_features_bound_rejections", launched=0.0)


_WIDE = 8192                  # channels of the wide texel: 32 KB per texel, 1.1 MB (5 x 7) and 1.9 MB (6 x 10) per view


def test_wide_texels_inside_the_bound_address_every_channel(dev):
    """Texels of 8192 channels (the byte offset of a tap reaches 2^21, the second factor of the 24-bit product 2^15) on the
    fixture's cameras: a channel's bits do not depend on the width of its map, so the first and the last 64 channels of
    the wide call equal the calls on those 64 channels alone -- the coarse warp with V = 2 (128 rounds of 64 channels on the
    parked taps), feature assembly with V = 1 and the wide map as third level (256 chunks)."""
    g = torch.Generator().manual_seed(77)
    _, cams = _frustum_scene()
    maps = torch.randn((1, 2, FR_H * FR_W, _WIDE), generator=g)
    cams1 = [x[:1] for x in cams]
    cost, world = _frustum(dev, maps, cams1, 2, FR_H, FR_W, FR_D)
    for sl in (slice(0, 64), slice(_WIDE - 64, _WIDE)):
        part, wpart = _frustum(dev, maps[..., sl], cams1, 2, FR_H, FR_W, FR_D)
        assert torch.equal(cost[:, sl], part) and torch.equal(world, wpart), sl
    pools, (depth, interval, cam) = _feature_scene()
    wide = torch.randn((1, FT_H * FT_W, _WIDE), generator=g)
    small = [pools[0][:1, :, :4], pools[1][:1, :, :4]]
    f, x = _features(dev, small + [wide], (4, 4, _WIDE), 1, FT_H, FT_W, depth, interval, cam, 1)
    for sl in (slice(0, 64), slice(_WIDE - 64, _WIDE)):
        fp, xp = _features(dev, small + [wide[..., sl]], (4, 4, 64), 1, FT_H, FT_W, depth, interval, cam, 1)
        assert torch.equal(f[:, 8 + sl.start:8 + sl.stop], fp[:, 8:72]) and torch.equal(x, xp), sl
        assert torch.equal(f[:, :8], fp[:, :8]) and torch.equal(f[:, 8 + _WIDE:], fp[:, 72:])
    assert _lib.status() == 0
    report("warp_fwd_wide_texels", mismatches=0.0)
