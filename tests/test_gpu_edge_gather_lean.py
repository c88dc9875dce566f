"""The lean form of the EdgeConv gather passes (csrc/edgeconv.hip, edge_stats_lean_kernel / edge_apply_lean_kernel)
against the general kernels, bit for bit.

The lean form runs when pf_edge_lean_supported says so: window codes, k = 16, C = 32 | 64, ldle == 2C.  The general
kernels stay in the library and are reached here with int64 indices of the same kNN call, or with the same codes and a
row stride the lean form refuses (ldle = 2C + 4): the second is the comparison on identical neighbour decoding.  Every
comparison is torch.equal.
"""
import pytest
import torch

from pointmvsnet_amd import _lib, pointflow, synthetic
from pointmvsnet_amd.networks import EdgeConv, EdgeConvNoC
from pointmvsnet_amd.utils.torch_utils import knn_lattice

# (G, D, H, W): a ragged last tile with the clamp acting at both ends of each group and no band; a plane of 8 tiles
# (XCD band order live); one wave mostly idle with nearly every neighbour clamped
LATTICES = [(3, 5, 9, 14), (2, 5, 16, 32), (1, 5, 2, 3)]
_cache = {}


def _knn(dev, lattice):
    """idx, codes of ONE knn_lattice call per lattice, shared by the tests (never modified)."""
    if lattice not in _cache:
        G, D, H, W = lattice
        gen = torch.Generator().manual_seed(7 * H + W)
        xyz = torch.randn(G, 3, D, H, W, generator=gen).to(dev)   # random cloud: neighbours all over the window
        _cache[lattice] = knn_lattice(xyz, 5, 16, with_codes=True)
    return _cache[lattice]


def _lean(C, ldle, Ng, has_codes=1, k=16):
    return int(_lib.load().pf_edge_lean_supported(C, k, ldle, Ng, has_codes))


def test_lean_predicate():
    for C in (32, 64):
        for Ng in (25600, 96000, 144000):                          # group sizes of cfg 2, 3 and 5
            assert _lean(C, 2 * C, Ng) == 1
            assert _lean(C, 2 * C, Ng, k=8) == 0
            assert _lean(C, 2 * C + 4, Ng) == 0
            assert _lean(C, 2 * C, Ng, has_codes=0) == 0
        first = (1 << 32) // (2 * C * 4)                           # first Ng with Ng * ldle * 4 >= 2^32
        assert _lean(C, 2 * C, first - 1) == 1 and _lean(C, 2 * C, first) == 0
    assert _lean(128, 256, 25600) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("C,concat", [(32, False), (32, True), (64, True)])
@pytest.mark.parametrize("lattice", LATTICES)
def test_layer_codes_equal_indices(dev, lattice, C, concat):
    G, D, H, W = lattice
    Ng, K = D * H * W, 40
    idx, codes = _knn(dev, lattice)
    assert _lean(C, 2 * C, Ng) == 1
    X = torch.randn(G * Ng, K, generator=torch.Generator().manual_seed(C)).to(dev)
    outs = []
    for use_codes in (False, True):
        mod = (EdgeConv if concat else EdgeConvNoC)(K, C)
        synthetic.seed_weights(mod, seed=2)
        mod = mod.to(dev).train()
        width = (2 if concat else 1) * C
        Y = torch.empty((G * Ng, width), device=dev)
        with torch.no_grad():
            pointflow.edge_conv_fused(X, True, K, K, G, Ng, None if use_codes else idx, mod.conv1.weight,
                                      mod.conv2.weight, mod.bn, concat, Y, width,
                                      codes=codes if use_codes else None, lattice=(5, H, W) if use_codes else None)
            pointflow.flush_counters()
        outs.append((Y, mod.bn.running_mean.clone(), mod.bn.running_var.clone()))
    torch.cuda.synchronize()
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert _lib.status() == 0


def _rows(dev, G, Ng, C):
    """Random rows [l | e], dense (ldle = 2C) and the same rows in a buffer with ldle = 2C + 4 (NaN in the padding)."""
    LE = torch.randn(G * Ng, 2 * C, generator=torch.Generator().manual_seed(Ng + C)).to(dev)
    wide = torch.full((G * Ng, 2 * C + 4), float("nan"), device=dev)
    wide[:, :2 * C] = LE
    return LE, wide


@pytest.mark.gpu
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("lattice", LATTICES)
def test_stats_direct(dev, lattice, C):
    G, D, H, W = lattice
    Ng = D * H * W
    idx, codes = _knn(dev, lattice)
    LE, wide = _rows(dev, G, Ng, C)
    T = pointflow.stat_blocks(G, Ng)
    assert _lean(C, 2 * C, Ng) == 1 and _lean(C, 2 * C + 4, Ng) == 0

    def run(le, ldle, use_codes):
        part = torch.full((G, T, C, 2), float("nan"), dtype=torch.float64, device=dev)
        _lib.call("pf_edge_stats_f32", _lib.ptr(le), ldle, C, None if use_codes else _lib.ptr(idx), 16, G, Ng,
                  _lib.ptr(part), _lib.ptr(codes) if use_codes else None, 5 if use_codes else 0, H, W, _lib.stream())
        return part

    lean = run(LE, 2 * C, True)
    by_idx = run(LE, 2 * C, False)
    by_stride = run(wide, 2 * C + 4, True)          # the refused stride: the general kernel on the same codes
    torch.cuda.synchronize()
    assert not torch.isnan(lean).any()
    assert torch.equal(lean, by_idx)
    assert torch.equal(lean, by_stride)
    assert _lib.status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("concat", [0, 1])
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("lattice", LATTICES)
def test_apply_direct(dev, lattice, C, concat):
    G, D, H, W = lattice
    Ng = D * H * W
    idx, codes = _knn(dev, lattice)
    LE, wide = _rows(dev, G, Ng, C)
    cols = (2 if concat else 1) * C
    ldy = cols + 8                                   # a strided output: the columns behind a row must stay untouched
    gen = torch.Generator().manual_seed(3 * C + concat)
    for gps in sorted({1, G}):
        S = G // gps
        scale = (torch.rand(S, 2 * C, generator=gen) + 0.5).to(dev)
        shift = (torch.randn(S, 2 * C, generator=gen) * 0.3).to(dev)

        def run(le, ldle, use_codes):
            Y = torch.full((G * Ng, ldy), -7.0, device=dev)
            _lib.call("pf_edge_apply_f32", _lib.ptr(le), ldle, C, None if use_codes else _lib.ptr(idx), 16, G, Ng,
                      _lib.ptr(scale), _lib.ptr(shift), 2 * C, gps, concat, _lib.ptr(Y), ldy,
                      _lib.ptr(codes) if use_codes else None, 5 if use_codes else 0, H, W, _lib.stream())
            return Y

        lean = run(LE, 2 * C, True)
        by_idx = run(LE, 2 * C, False)
        by_stride = run(wide, 2 * C + 4, True)      # the refused stride: the general kernel on the same codes
        torch.cuda.synchronize()
        assert bool((lean[:, cols:] == -7.0).all()) and not torch.isnan(lean).any()
        assert bool((lean[:, :cols] != -7.0).all())
        assert torch.equal(lean, by_idx)
        assert torch.equal(lean, by_stride)
    assert _lib.status() == 0
