"""Case tables and float64 checkers of the forward arms that only large shapes select: tests/test_gpu_conv_fwd_arms.py
runs them on an MI355X, tests/test_emulated_kernels.py the cheapest on the CPU emulator (tests/hipemu).  A plain module,
not a conftest.

csrc/conv3d.hip takes the deepest tile TD in {4, 2, 1} that still leaves >= 512 tiles, walks several tiles per block above
2048 tiles and opts in to > 64 KiB of LDS at stride 2 with two channel tiles; csrc/deconv3d.hip picks its channel group
(4 / 2 / 1) and its matrix-core form by the number of blocks; pf_gemm_blocks / pf_stat_blocks cap the blocks of the GEMM
and of the EdgeConv gather passes; csrc/knn_lattice.hip picks a kernel by window, k and lattice size.  A unit-test-sized
shape reaches none of these, so every case here names the arm it exists for and asserts it -- through pf_conv3d_plan /
pf_deconv3d_plan (computed by the function the launch calls), pf_conv3d_pair_blocks, pf_gemm_blocks, pf_stat_blocks --
BEFORE it compares numbers: a case that stops reaching its arm fails instead of passing vacuously.

References: float64 F.conv3d / F.conv_transpose3d / matmul on the CPU, a float64 composition of EdgeConv on the device,
oracle/bruteforce.py for the kNN.  Gates are those of tests/test_gpu_ops.py for the same entry points; every result is
produced twice, bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import report
from oracle import bruteforce as BF
from pointmvsnet_amd import _lib, pointflow, synthetic
from pointmvsnet_amd.networks import EdgeConv, EdgeConvNoC
from pointmvsnet_amd.utils.torch_utils import knn_lattice


def _maxabs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def _cdiv(a, b):
    return -(-a // b)


def tag_of(case):
    return "_".join(str(v) for v in case)


# ---------------------------------------------------------------------------------------------
# 1. pf_conv3d_k3_f32: (Cin, Cout, Di, Hi, Wi, stride) -> the plan pf_conv3d_plan must report
#    (NT, TD, tiles, tiles per block, blocks, LDS bytes), what the case exists for.
#
# Every row of CONV_K3 has Do % TD, Ho % 4 and Wo % 16 != 0 (asserted).  The arms (NT, stride, TD): (2,1,4), (2,1,2),
# (1,1,2), (1,2,2), (2,2,2); tiles per block >= 2 under each TD; lds > 65536 (the opt-in to big dynamic LDS).
# conv3d_k3_kernel<1, 1, 4, .> is instantiated but never launched: pick_td starts at TD 2 for one channel tile (with
# <= 16 output channels TD 2 at twice the occupancy beats TD 4), so no shape reaches it.
# ---------------------------------------------------------------------------------------------
CONV_K3 = [
    ((4, 32, 13, 30, 250, 1), (2, 4, 512, 1, 512, 49696), "TD 4, last depth tile 1 of 4"),
    ((8, 17, 13, 30, 250, 1), (2, 4, 512, 1, 512, 49728), "one live column in the second channel tile, two channel groups"),
    ((4, 32, 13, 126, 270, 1), (2, 4, 2176, 2, 1088, 49696), "TD 4, several tiles per block"),
    ((12, 20, 7, 30, 250, 1), (2, 2, 512, 1, 512, 42592), "TD 2 under NT 2, odd number of channel groups"),
    ((4, 16, 7, 30, 250, 1), (1, 2, 512, 1, 512, 28704), "TD 2 stride 1"),
    ((4, 9, 7, 126, 270, 1), (1, 2, 2176, 2, 1088, 28704), "TD 2, several tiles per block, Cout 9"),
    ((4, 16, 13, 59, 499, 2), (1, 2, 512, 1, 512, 63552), "stride 2, odd input extents"),
    ((4, 16, 14, 60, 500, 2), (1, 2, 512, 1, 512, 63552), "stride 2, even extents: the last halo plane inside the tensor"),
    ((4, 32, 13, 59, 499, 2), (2, 2, 512, 1, 512, 77376), "> 64 KiB LDS opt-in"),
    ((4, 17, 13, 251, 539, 2), (2, 2, 2176, 2, 1088, 77376), "opt-in and several tiles per block"),
]
# the rows that also run with a pending BatchNorm + ReLU (aff_mode 1 and 2) on two samples
CONV_K3_AFFINE = [CONV_K3[i] for i in (0, 3, 4, 6, 8)]
# their TD-1 twins: the same channel counts and strides on a volume of a few tiles (also on the CPU emulator)
CONV_K3_TD1 = [
    ((4, 32, 5, 6, 19, 1), (2, 1, 20, 1, 20, 39456), "TD 1 twin, NT 2"),
    ((8, 17, 5, 6, 19, 1), (2, 1, 20, 1, 20, 39488), "TD 1 twin, one live column in the second channel tile"),
    ((12, 20, 3, 6, 19, 1), (2, 1, 12, 1, 12, 39520), "TD 1 twin, odd number of channel groups"),
    ((4, 16, 5, 6, 19, 1), (1, 1, 20, 1, 20, 25632), "TD 1 twin, NT 1"),
    ((4, 16, 5, 11, 35, 2), (1, 1, 12, 1, 12, 44096), "TD 1 twin, stride 2, odd extents"),
    ((4, 16, 6, 12, 36, 2), (1, 1, 12, 1, 12, 44096), "TD 1 twin, stride 2, even extents"),
    ((4, 32, 5, 11, 35, 2), (2, 1, 12, 1, 12, 57920), "TD 1 twin, stride 2, NT 2"),
]
CONV_PLAN_FIELDS = ("NT", "TD", "tiles", "tiles_per_block", "blocks", "lds_bytes")

# Seeds of the pending-BatchNorm runs, keyed by the INPUT (Cin, Di, Hi, Wi) and the form: those for which no
# pre-activation of the float64 reference lies within 1e-6 of zero, so that no ReLU of the comparison rests on a sign
# tie (asserted on the reference; found by counting upwards from 0).
AFFINE_SEEDS = {
    ((2, 4, 13, 30, 250), "rows"): 0, ((2, 4, 13, 30, 250), "lazy"): 2,
    ((2, 12, 7, 30, 250), "rows"): 0, ((2, 12, 7, 30, 250), "lazy"): 1,
    ((2, 4, 7, 30, 250), "rows"): 0, ((2, 4, 7, 30, 250), "lazy"): 0,
    ((2, 4, 13, 59, 499), "rows"): 21, ((2, 4, 13, 59, 499), "lazy"): 13,
    ((2, 4, 5, 6, 19), "rows"): 0, ((2, 4, 5, 6, 19), "lazy"): 0,
    ((2, 8, 5, 6, 19), "rows"): 0, ((2, 8, 5, 6, 19), "lazy"): 0,
    ((2, 12, 3, 6, 19), "rows"): 0, ((2, 12, 3, 6, 19), "lazy"): 0,
    ((2, 4, 5, 11, 35), "rows"): 0, ((2, 4, 5, 11, 35), "lazy"): 0,
    ((2, 4, 6, 12, 36), "rows"): 0, ((2, 4, 6, 12, 36), "lazy"): 0,
    ((1, 12, 11, 31, 49), "rows"): 0, ((1, 12, 11, 31, 49), "lazy"): 0,
    ((2, 4, 7, 31, 77), "rows"): 0, ((2, 4, 7, 31, 77), "lazy"): 0,
}


def conv_plan(case):
    plan = (ctypes.c_int * 8)()
    _lib.check(_lib.load().pf_conv3d_plan(*[int(v) for v in case], plan), "pf_conv3d_plan")
    assert plan[6] == 0 and plan[7] == 0
    return dict(zip(CONV_PLAN_FIELDS, list(plan)[:6]))


def assert_conv_plan(case, want, ragged=True):
    Cin, Cout, Di, Hi, Wi, stride = case
    plan = conv_plan(case)
    assert tuple(plan[f] for f in CONV_PLAN_FIELDS) == tuple(want), (case, plan, want)
    assert plan["blocks"] == int(_lib.load().pf_conv3d_blocks(*[int(v) for v in case]))
    assert plan["blocks"] * plan["tiles_per_block"] >= plan["tiles"] > plan["blocks"] * (plan["tiles_per_block"] - 1)
    if ragged:
        Do, Ho, Wo = ((v - 1) // stride + 1 for v in (Di, Hi, Wi))
        assert Do % plan["TD"] != 0 and Ho % 4 != 0 and Wo % 16 != 0, (case, plan)
    return plan


def _k_gate(Cin):
    return max(1.0, (27 * Cin / 256.0) ** 0.5)         # float32 fmaf chain of length 27 * Cin


def check_conv3d_plain(dev, case, want, prefix, ragged=True):
    """One sample, plain input, with statistics: y against float64, one statistics row per block of the plan, the
    rows' sums against the reference's, and a second run without statistics equal bit for bit."""
    Cin, Cout, Di, Hi, Wi, stride = case
    plan = assert_conv_plan(case, want, ragged)
    gen = torch.Generator().manual_seed(1000 + Cin + Cout + Di * Hi * Wi)
    x = torch.randn(1, Cin, Di, Hi, Wi, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=gen) / (27 * Cin) ** 0.5
    ref = F.conv3d(x.double(), w.double(), None, stride, 1)
    xd, wd = x.to(dev), w.to(dev)
    y, part = pointflow.conv3d_k3(xd, wd, stride, True)
    assert y.shape == ref.shape and part.shape == (1, plan["blocks"], Cout, 2)
    scale = float(ref.abs().max())
    err = _maxabs(y, ref)
    report("%s_%s" % (prefix, tag_of(case)), err=err, scale=scale, rel=err / scale, **plan)
    assert err < 3e-6 * scale * _k_gate(Cin), (err, scale)
    sums = part.sum(dim=1).cpu()
    assert torch.allclose(sums[..., 0], ref.sum(dim=(2, 3, 4)), rtol=1e-5, atol=1e-4 * scale)
    assert torch.allclose(sums[..., 1], (ref ** 2).sum(dim=(2, 3, 4)), rtol=1e-5)
    y2, none = pointflow.conv3d_k3(xd, wd, stride, False)
    assert none is None and torch.equal(y2, y)
    y3, part3 = pointflow.conv3d_k3(xd, wd, stride, True)
    assert torch.equal(y3, y) and torch.equal(part3, part)
    assert _lib.status() == 0
    return err / scale


def _statistics_rows(xd, T):
    """(N, T, C, 2) float64 (sum, sum of squares) of xd (N, C, ...) in T chunks: what a producer's epilogue leaves."""
    N, C = xd.shape[:2]
    part = torch.zeros((N, T, C, 2), dtype=torch.float64, device=xd.device)
    for t, ch in enumerate(torch.chunk(xd.double().reshape(N, C, -1), T, dim=2)):
        part[:, t, :, 0] = ch.sum(dim=2)
        part[:, t, :, 1] = (ch * ch).sum(dim=2)
    return part


def pending_batchnorm_input(shape, form, seed):
    """x (N, C, D, H, W) float32 on the CPU with a pending BatchNorm + ReLU in ``form`` "rows" -- one (scale, shift) row
    per sample, all different -- or "lazy" -- a train-mode BatchNorm over all N samples.  Returns (x, what the form needs,
    the float64 pre-activation, the generator)."""
    N, C = shape[:2]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=gen)
    view = (N, C) + (1,) * (len(shape) - 2)
    if form == "rows":
        sc = torch.rand(N, C, generator=gen) + 0.5
        sh = torch.randn(N, C, generator=gen) * 0.3
        return x, (sc, sh), x.double() * sc.double().view(view) + sh.double().view(view), gen
    gamma, beta = torch.linspace(0.5, 1.5, C), torch.linspace(-0.3, 0.3, C)
    pre = F.batch_norm(x.double(), None, None, gamma.double(), beta.double(), True, 0.0, 1e-5)
    return x, (gamma, beta), pre, gen


def tie_free_seed(shape, form):
    """The first seed for which no pre-activation lies within 1e-6 of zero (how AFFINE_SEEDS was filled)."""
    seed = 0
    while float(pending_batchnorm_input(shape, form, seed)[2].abs().min()) <= 1e-6:
        seed += 1
    return seed


def _pending_on_device(dev, x, extra, pre, form):
    """The ``in_affine`` argument and samples_per_stat of ``form`` for x on ``dev``; asserts the reference is tie-free."""
    assert float(pre.abs().min()) > 1e-6, "a ReLU of the reference rests on a sign tie: choose another seed"
    N, C = x.shape[:2]
    xd = x.to(dev)
    if form == "rows":
        return xd, (extra[0].to(dev), extra[1].to(dev)), 1
    bn = torch.nn.BatchNorm3d(C).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(extra[0])
        bn.bias.copy_(extra[1])
    assert bn.eps == 1e-5
    aff = pointflow.bn_affine_rows(xd, bn, N, _statistics_rows(xd, 5), lazy=True)
    assert isinstance(aff, pointflow.LazyAffine)
    return xd, aff, N


def check_conv3d_pending_batchnorm(dev, case, want, form, prefix, ragged=True):
    """Two samples with the input's BatchNorm + ReLU pending: form "rows" = two DIFFERENT (scale, shift) rows,
    samples_per_stat 1 (sample n reads row n); form "lazy" = a LazyAffine over both samples, samples_per_stat 2, resolved
    by every block from the producer's statistics rows.  Against BatchNorm -> ReLU -> float64 convolution."""
    Cin, Cout, Di, Hi, Wi, stride = case
    plan = assert_conv_plan(case, want, ragged)
    shape = (2, Cin, Di, Hi, Wi)
    x, extra, pre, gen = pending_batchnorm_input(shape, form, AFFINE_SEEDS[(shape, form)])
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=gen) / (27 * Cin) ** 0.5
    ref = F.conv3d(torch.relu(pre), w.double(), None, stride, 1)
    xd, aff, sps = _pending_on_device(dev, x, extra, pre, form)
    wd = w.to(dev)
    y, part = pointflow.conv3d_k3(xd, wd, stride, True, in_affine=aff, samples_per_stat=sps)
    assert y.shape == ref.shape and part.shape == (2, plan["blocks"], Cout, 2)
    scale = float(ref.abs().max())
    err = _maxabs(y, ref)
    report("%s_%s_%s" % (prefix, tag_of(case), form), err=err, scale=scale, rel=err / scale, **plan)
    assert err < (2e-5 if form == "lazy" else 4e-6) * scale * _k_gate(Cin), (err, scale)
    sums = part.sum(dim=1).cpu()
    assert torch.allclose(sums[..., 0], ref.sum(dim=(2, 3, 4)), rtol=1e-4, atol=2e-4 * scale * ref[0, 0].numel() ** 0.5)
    y2, none = pointflow.conv3d_k3(xd, wd, stride, False, in_affine=aff, samples_per_stat=sps)
    assert none is None and torch.equal(y2, y)
    pointflow.flush_counters()
    assert _lib.status() == 0
    return err / scale


# ---------------------------------------------------------------------------------------------
# 2. pf_conv3d_k3_pair_f32 (stride 1, <= 8 output channels): (Cin, Cout, D, H, W) -> (tiles, tiles per block, blocks)
# ---------------------------------------------------------------------------------------------
CONV_PAIR = [
    ((8, 5, 3, 262, 1001), (4158, 3, 1386)),       # odd D under TD 2, H % 8 != 0, W % 16 != 0, Cout < 8
    ((4, 8, 1, 262, 1001), (2079, 2, 1040)),
]


def check_conv3d_pair(dev, case, want, prefix):
    Cin, Cout, D, H, W = case
    tiles, per, blocks = want
    assert tiles == _cdiv(D, 2) * _cdiv(H, 8) * _cdiv(W, 16) and D % 2 != 0 and H % 8 != 0 and W % 16 != 0
    T = int(_lib.load().pf_conv3d_pair_blocks(Cin, Cout, D, H, W))
    assert T == blocks < tiles and _cdiv(tiles, T) == per >= 2, (T, want)
    gen = torch.Generator().manual_seed(Cin + Cout + D * H * W)
    x = torch.randn(1, Cin, D, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=gen) / (27 * Cin) ** 0.5
    ref = F.conv3d(x.double(), w.double(), None, 1, 1)
    xd, wd = x.to(dev), w.to(dev)
    y, part = pointflow.conv3d_k3(xd, wd, 1, True)
    assert y.shape == ref.shape and part.shape == (1, T, Cout, 2)
    scale = float(ref.abs().max())
    err = _maxabs(y, ref)
    report("%s_%s" % (prefix, tag_of(case)), err=err, scale=scale, rel=err / scale, tiles=tiles, blocks=T)
    assert err < 3e-6 * scale * _k_gate(Cin), (err, scale)
    sums = part.sum(dim=1).cpu()
    assert torch.allclose(sums[..., 0], ref.sum(dim=(2, 3, 4)), rtol=1e-5, atol=1e-4 * scale)
    assert torch.allclose(sums[..., 1], (ref ** 2).sum(dim=(2, 3, 4)), rtol=1e-5)
    y2, none = pointflow.conv3d_k3(xd, wd, 1, False)
    assert none is None and torch.equal(y2, y)
    y3, part3 = pointflow.conv3d_k3(xd, wd, 1, True)
    assert torch.equal(y3, y) and torch.equal(part3, part)
    assert _lib.status() == 0
    return err / scale


# ---------------------------------------------------------------------------------------------
# 3. pf_deconv3d_k3s2_f32 by its shape rule, no environment switch: (N, Cin, Cout, D, H, W) -> (form, CG)
# ---------------------------------------------------------------------------------------------
DECONV = [
    ((1, 12, 16, 11, 31, 49), (0, 4), "CG 4; Cin % 8 != 0: the unroll's tail"),
    ((1, 36, 32, 11, 31, 49), (0, 4), "CG 4 at Cout 32: Cin > 32 keeps the matrix-core form out"),
    ((1, 5, 6, 11, 31, 65), (0, 2), "CG 2"),
    ((2, 4, 32, 7, 31, 77), (1, 16), "matrix-core form by the shape rule, two samples"),
]
DECONV_AFFINE = [DECONV[0], DECONV[3]]


def deconv_plan(case):
    plan = (ctypes.c_int * 4)()
    _lib.check(_lib.load().pf_deconv3d_plan(*[int(v) for v in case], plan), "pf_deconv3d_plan")
    return dict(form=plan[0], CG=plan[1], blocks_x=plan[2])


def assert_deconv_plan(case, want, monkeypatch):
    N, Cin, Cout, D, H, W = case
    monkeypatch.delenv("PF_DECONV_MFMA", raising=False)
    monkeypatch.delenv("PF_DECONV_VALU", raising=False)
    plan = deconv_plan(case)
    assert (plan["form"], plan["CG"]) == tuple(want), (case, plan)
    assert plan["blocks_x"] == _cdiv(D * H * W, 128) == int(_lib.load().pf_deconv3d_blocks(D, H, W))
    assert (D * H * W) % 128 != 0                   # a partial last block of cells
    return plan


def check_deconv_plan_honours_the_switches(monkeypatch):
    """PF_DECONV_MFMA / PF_DECONV_VALU move the query as they move the launch (one selection function)."""
    case = (2, 32, 16, 12, 16, 20)
    monkeypatch.delenv("PF_DECONV_MFMA", raising=False)
    monkeypatch.delenv("PF_DECONV_VALU", raising=False)
    assert deconv_plan(case)["form"] == 0
    monkeypatch.setenv("PF_DECONV_MFMA", "1")
    assert deconv_plan(case) == dict(form=1, CG=16, blocks_x=30)
    assert deconv_plan((1, 36, 32, 11, 31, 49))["form"] == 0        # not admissible: stays lane-per-cell
    monkeypatch.setenv("PF_DECONV_VALU", "1")
    assert deconv_plan(case)["form"] == 0
    monkeypatch.delenv("PF_DECONV_MFMA")
    assert deconv_plan((2, 4, 32, 7, 31, 77))["form"] == 0 and deconv_plan((1, 16, 64, 24, 32, 40)) == dict(form=0, CG=4, blocks_x=240)


def check_deconv(dev, case, want, skip, monkeypatch, prefix):
    N, Cin, Cout, D, H, W = case
    plan = assert_deconv_plan(case, want, monkeypatch)
    gen = torch.Generator().manual_seed(Cin * 100 + D * H * W + int(skip))
    xa = torch.randn(N, Cin, D, H, W, generator=gen)
    xb = torch.randn(N, Cin, D, H, W, generator=gen) if skip else None
    w = torch.randn(Cin, Cout, 3, 3, 3, generator=gen) / (4 * Cin) ** 0.5
    ref = F.conv_transpose3d((xa + xb if skip else xa).double(), w.double(), None, stride=2, padding=1, output_padding=1)
    xad, xbd, wd = xa.to(dev), None if xb is None else xb.to(dev), w.to(dev)
    y, part = pointflow.deconv3d_k3s2(xad, xbd, wd, True)
    assert y.shape == ref.shape == (N, Cout, 2 * D, 2 * H, 2 * W) and part.shape == (N, plan["blocks_x"], Cout, 2)
    scale = float(ref.abs().max())
    err = _maxabs(y, ref)
    report("%s_%s_skip%d" % (prefix, tag_of(case), int(skip)), err=err, scale=scale, rel=err / scale, **plan)
    assert err < 3e-6 * scale, (err, scale)
    sums = part.sum(dim=1).cpu()
    assert torch.allclose(sums[..., 0], ref.sum(dim=(2, 3, 4)), rtol=1e-4, atol=1e-3 * scale)
    assert torch.allclose(sums[..., 1], (ref ** 2).sum(dim=(2, 3, 4)), rtol=1e-5)
    y2, none = pointflow.deconv3d_k3s2(xad, xbd, wd, False)
    assert none is None and torch.equal(y2, y)
    y3, part3 = pointflow.deconv3d_k3s2(xad, xbd, wd, True)
    assert torch.equal(y3, y) and torch.equal(part3, part)
    assert _lib.status() == 0
    return err / scale


def check_deconv_pending_batchnorm(dev, case, want, skip, form, monkeypatch, prefix):
    """y = deconv(relu(bn(xa)) + xb) with the BatchNorm + ReLU of xa pending, in the form the shape rule picks."""
    N, Cin, Cout, D, H, W = case
    plan = assert_deconv_plan(case, want, monkeypatch)
    shape = (N, Cin, D, H, W)
    xa, extra, pre, gen = pending_batchnorm_input(shape, form, AFFINE_SEEDS[(shape, form)])
    xb = torch.randn(N, Cin, D, H, W, generator=gen) if skip else None
    w = torch.randn(Cin, Cout, 3, 3, 3, generator=gen) / (4 * Cin) ** 0.5
    ref = F.conv_transpose3d(torch.relu(pre) + (xb.double() if skip else 0.0), w.double(), None, 2, 1, 1)
    xad, aff, sps = _pending_on_device(dev, xa, extra, pre, form)
    xbd, wd = None if xb is None else xb.to(dev), w.to(dev)
    y, part = pointflow.deconv3d_k3s2(xad, xbd, wd, True, in_affine=aff, samples_per_stat=sps)
    assert part.shape == (N, plan["blocks_x"], Cout, 2)
    scale = float(ref.abs().max())
    err = _maxabs(y, ref)
    report("%s_%s_skip%d_%s" % (prefix, tag_of(case), int(skip), form), err=err, scale=scale, rel=err / scale, **plan)
    assert err < (2e-5 if form == "lazy" else 4e-6) * scale, (err, scale)
    sums = part.sum(dim=1).cpu()
    assert torch.allclose(sums[..., 0], ref.sum(dim=(2, 3, 4)), rtol=1e-4, atol=2e-4 * scale * ref[0, 0].numel() ** 0.5)
    y2, none = pointflow.deconv3d_k3s2(xad, xbd, wd, False, in_affine=aff, samples_per_stat=sps)
    assert none is None and torch.equal(y2, y)
    pointflow.flush_counters()
    assert _lib.status() == 0
    return err / scale


# ---------------------------------------------------------------------------------------------
# 4. pointwise GEMM with several tiles per block: (G, Ng) -> (T, tiles per block); (point_major, K, cout, ldx)
# ---------------------------------------------------------------------------------------------
GEMM_GROUPS = [((32, 17 * 128 + 5), (9, 2)), ((40, 33 * 128 + 1), (12, 3))]
GEMM_ARMS = [(True, 64, 64, 64),          # the direct-A kernel (point-major, K % 4 == 0, W in LDS)
             (True, 7, 32, 11),           # the generic kernel, point-major
             (False, 7, 32, 0)]           # ... channel-major


def check_gemm(dev, groups, want, arm, prefix):
    (G, Ng), (T_want, per) = groups, want
    point_major, K, cout, ldx = arm
    tiles = _cdiv(Ng, 128)
    T = int(_lib.load().pf_gemm_blocks(G, Ng))
    assert T == T_want < tiles and _cdiv(tiles, T) == per and Ng % 128 != 0
    gen = torch.Generator().manual_seed(G * Ng + K)
    w = torch.randn(cout, K, 1, generator=gen)
    if point_major:
        x = torch.randn(G * Ng, ldx, generator=gen)
        xm = x[:, :K].view(G, Ng, K)
    else:
        x = torch.randn(G, K, Ng, generator=gen)
        xm = x.transpose(1, 2)
    sc = torch.rand(G, K, generator=gen) + 0.5
    sh = torch.randn(G, K, generator=gen) * 0.3
    Wt, _ = pointflow.pack_weight_t(w.to(dev))
    xd = x.to(dev)
    worst = 0.0
    for affine in (None, (sc, sh)):
        a = xm.double()
        if affine is not None:
            a = torch.relu(a * sc.double().unsqueeze(1) + sh.double().unsqueeze(1))
        ref = a @ w[:, :, 0].double().t()
        aff = None if affine is None else (sc.to(dev), sh.to(dev))
        runs = []
        for _ in range(2):
            Y = torch.full((G * Ng, cout + 4), -7.0, device=dev)
            part = pointflow.pointwise_gemm(xd, point_major, ldx, Wt, Y, cout + 4, G, Ng, K, cout, in_affine=aff,
                                            want_stats=True)
            runs.append((Y, part))
        (Y, part), (Y2, part2) = runs
        assert torch.equal(Y, Y2) and torch.equal(part, part2) and part.shape[:2] == (G, T)
        scale = float(ref.abs().max())
        err = _maxabs(Y[:, :cout].view(G, Ng, cout), ref)
        worst = max(worst, err / scale)
        report("%s_G%d_Ng%d_K%d_c%d_pm%d_aff%d" % (prefix, G, Ng, K, cout, int(point_major), int(affine is not None)),
               err=err, scale=scale, rel=err / scale, T=T, tiles=tiles)
        assert err < 2e-6 * scale * max(1.0, (K / 32.0) ** 0.5), (err, scale)
        assert float((Y[:, cout:] + 7.0).abs().max()) == 0.0                 # padding columns untouched
        sums = part.sum(dim=1).cpu()
        assert torch.allclose(sums[:, :cout, 0], ref.sum(dim=1), rtol=1e-5, atol=1e-4 * scale)
        assert torch.allclose(sums[:, :cout, 1], (ref ** 2).sum(dim=1), rtol=1e-5)
    assert _lib.status() == 0
    return worst


# ---------------------------------------------------------------------------------------------
# 5. the EdgeConv gather passes with several tiles per block
# ---------------------------------------------------------------------------------------------
EDGE_G, EDGE_NG, EDGE_T = 128, 33 * 64 - 7, 17
# (C, k, groups_per_stat, concat)
EDGE_CASES = [(32, 16, 1, True), (32, 5, 2, True), (32, 16, 2, False), (32, 5, 1, False),
              (64, 16, 2, True), (64, 5, 1, True), (64, 16, 1, False), (64, 5, 2, False)]


def edge_reference(le, idx, gamma, beta, concat, gps, eps):
    """EdgeConv from its definition in float64 on le's device: le (G, Ng, 2C) = [l | e], idx (G, Ng, k) group-local;
    batch statistics over the gps groups of a statistic group, all points and all neighbours, biased variance."""
    G, Ng, C2 = le.shape
    C = C2 // 2
    out = torch.empty((G, Ng, C2 if concat else C), dtype=torch.float64, device=le.device)
    for s0 in range(0, G, gps):
        l, e = le[s0:s0 + gps, :, :C].double(), le[s0:s0 + gps, :, C:].double()
        nb = torch.stack([e[g][idx[s0 + g]] for g in range(gps)])          # (gps, Ng, k, C)
        d = nb - l.unsqueeze(2)
        t = torch.cat([l.unsqueeze(2).expand_as(d), d], dim=3) if concat else d
        mean = t.mean(dim=(0, 1, 2))
        var = t.var(dim=(0, 1, 2), unbiased=False)
        t = (t - mean) / torch.sqrt(var + eps) * gamma + beta
        out[s0:s0 + gps] = torch.relu(t).mean(dim=2)
    return out


def check_edge_fused(dev, C, k, gps, concat, prefix, G=EDGE_G, Ng=EDGE_NG, T_want=EDGE_T):
    """pointflow.edge_conv_fused (GEMM, pf_edge_stats_f32, finalize, pf_edge_apply_f32) on int64 indices against the
    float64 composition, from the same float32 input and weights."""
    K = 32
    tiles = _cdiv(Ng, 64)
    T = pointflow.stat_blocks(G, Ng)
    if T_want is not None:
        assert T == T_want < tiles and Ng % 64 != 0
    gen = torch.Generator().manual_seed(C + k + gps)
    X = torch.randn(G * Ng, K, generator=gen).to(dev)
    idx = torch.randint(0, Ng, (G, Ng, k), generator=gen).to(dev)
    mod = (EdgeConv if concat else EdgeConvNoC)(K, C)
    synthetic.seed_weights(mod, seed=4)
    mod = mod.to(dev).train()
    width = (2 if concat else 1) * C
    w1, w2 = mod.conv1.weight[:, :, 0].detach().double(), mod.conv2.weight[:, :, 0].detach().double()
    le = torch.cat([X.double() @ w1.t(), X.double() @ w2.t()], dim=1).view(G, Ng, 2 * C)
    ref = edge_reference(le, idx, mod.bn.weight.detach().double(), mod.bn.bias.detach().double(), concat, gps, mod.bn.eps)
    outs = []
    for _ in range(2):
        Y = torch.empty((G * Ng, width), device=dev)
        with torch.no_grad():
            pointflow.edge_conv_fused(X, True, K, K, G, Ng, idx, mod.conv1.weight, mod.conv2.weight, mod.bn, concat, Y,
                                      width, groups_per_stat=gps)
        outs.append(Y)
    pointflow.flush_counters()
    assert torch.equal(outs[0], outs[1])
    err = float((outs[0].double().view(G, Ng, width) - ref).abs().max())
    report("%s_C%d_k%d_gps%d_cat%d_G%d_Ng%d" % (prefix, C, k, gps, int(concat), G, Ng), err=err, T=T, tiles=tiles)
    assert err < 3e-5, err
    assert _lib.status() == 0
    return err


def check_edge_passes_c128(dev, k, prefix):
    """edge_stats_kernel<128, .> / edge_apply_kernel<128, .> behind the C ABI (no module reaches 128 channels: the GEMM
    in front of them stops at 128 columns): the two passes on random rows LE, statistics rows and output against the
    float64 definition."""
    G, Ng, C, gps = 3, 200, 128, 1
    gen = torch.Generator().manual_seed(128 + k)
    le = torch.randn(G * Ng, 2 * C, generator=gen).to(dev)
    idx = torch.randint(0, Ng, (G, Ng, k), generator=gen).to(dev)
    sc = (torch.rand(G, 2 * C, generator=gen) + 0.5).to(dev)
    sh = (torch.randn(G, 2 * C, generator=gen) * 0.3).to(dev)
    T = pointflow.stat_blocks(G, Ng)
    l, e = le.view(G, Ng, 2 * C)[:, :, :C].double(), le.view(G, Ng, 2 * C)[:, :, C:].double()
    d = torch.stack([e[g][idx[g]] for g in range(G)]) - l.unsqueeze(2)              # (G, Ng, k, C)
    worst = 0.0
    for concat in (True, False):
        runs = []
        for _ in range(2):
            part = torch.empty((G, T, C, 2), dtype=torch.float64, device=dev)
            _lib.call("pf_edge_stats_f32", _lib.ptr(le), 2 * C, C, _lib.ptr(idx), k, G, Ng, _lib.ptr(part), None, 0, 1, 1,
                      _lib.stream())
            width = (2 if concat else 1) * C
            Y = torch.empty((G * Ng, width), device=dev)
            _lib.call("pf_edge_apply_f32", _lib.ptr(le), 2 * C, C, _lib.ptr(idx), k, G, Ng, _lib.ptr(sc), _lib.ptr(sh),
                      2 * C, gps, int(concat), _lib.ptr(Y), width, None, 0, 1, 1, _lib.stream())
            runs.append((part, Y))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        part, Y = runs[0]
        sums = part.sum(dim=1)
        assert torch.allclose(sums[..., 0], d.sum(dim=(1, 2)), rtol=1e-5, atol=1e-4 * float(d.abs().max()))
        assert torch.allclose(sums[..., 1], (d * d).sum(dim=(1, 2)), rtol=1e-5)
        scd, shd = sc.double().unsqueeze(1), sh.double().unsqueeze(1)
        if concat:
            ref = torch.cat([torch.relu(l * scd[..., :C] + shd[..., :C]),
                             torch.relu(d * scd[..., C:].unsqueeze(2) + shd[..., C:].unsqueeze(2)).mean(dim=2)], dim=2)
        else:
            ref = torch.relu(d * scd[..., :C].unsqueeze(2) + shd[..., :C].unsqueeze(2)).mean(dim=2)
        err = float((Y.double().view(G, Ng, width) - ref).abs().max())
        worst = max(worst, err)
        report("%s_C128_k%d_cat%d" % (prefix, k, int(concat)), err=err, scale=float(ref.abs().max()))
        assert err < 3e-5, err
    assert _lib.status() == 0
    return worst


# ---------------------------------------------------------------------------------------------
# 6. lattice kNN: (window, k, (B, D, H, W), samples compared, the kernel csrc/knn_lattice.hip picks)
# ---------------------------------------------------------------------------------------------
_BIG = (16, 4, 32, 33)             # B * D * H * W = 67 584 >= 65 536: the whole-window scan, one lane per point
KNN_CASES = [
    (7, 16, (2, 3, 9, 35), (0, 1), "split"), (7, 5, (2, 3, 9, 35), (0, 1), "split"),
    (7, 8, _BIG, (0, 15), "scan8"), (7, 12, _BIG, (0, 15), "scan16"),
    (7, 20, (2, 3, 9, 35), (0, 1), "scan32"),
    (1, 1, (2, 3, 9, 35), (0, 1), "scan8"),
    (3, 27, (2, 3, 9, 35), (0, 1), "scan32"),        # every candidate ranked, the zero-padded ones and the clamp included
    (5, 1, (2, 3, 9, 35), (0, 1), "network"), (5, 7, (2, 3, 9, 35), (0, 1), "network"),
]
KNN_EMULATED = [(7, 16, (1, 3, 9, 35), (0,), "split"), (7, 5, (1, 3, 9, 35), (0,), "split"),
                (7, 20, (1, 3, 9, 35), (0,), "scan32")]


def knn_kernel(window, k, shape):
    """The kernel pf_knn_lattice_f32's dispatch (csrc/knn_lattice.hip) launches for this call."""
    B, D, H, W = shape
    if k <= 16 and window in (3, 5):
        return "network"
    if k <= 16 and window ** 3 >= 64 and B * D * H * W < 65536:
        return "split"
    return "scan8" if k <= 8 else ("scan16" if k <= 16 else "scan32")


def knn_id(case):
    return "w%d_k%d_%s" % (case[0], case[1], "x".join(str(v) for v in case[2]))


def check_knn(dev, window, k, shape, samples, kernel):
    assert knn_kernel(window, k, shape) == kernel
    B, D, H, W = shape
    g = torch.Generator().manual_seed(B * H + window + k)
    base = torch.stack(torch.meshgrid(torch.arange(W).float(), torch.arange(H).float(), torch.arange(D).float(),
                                      indexing="xy"), 0).permute(0, 3, 1, 2)
    xyz = base.unsqueeze(0).repeat(B, 1, 1, 1, 1) * 0.07 - 1.0 + 0.02 * torch.randn(B, 3, D, H, W, generator=g)
    xyz[:, :, :, :2, :3] = xyz[:, :, :, 2:4, :3]                  # exact duplicates: ties resolved by the code order
    xd = xyz.to(dev)
    idx = knn_lattice(xd, window, k)
    assert idx.dtype == torch.int64 and idx.shape == (B, D * H * W, k)
    assert torch.equal(knn_lattice(xd, window, k), idx)
    for b in samples:
        bf_idx, _ = BF.knn_window(xyz[b].numpy(), window, k)
        assert np.array_equal(idx[b].cpu().numpy(), bf_idx), (window, k, b)
    if window == 1:
        assert torch.equal(idx.cpu(), torch.arange(D * H * W).view(1, -1, 1).expand(B, -1, 1))
    assert _lib.status() == 0


def check_knn_window7_has_no_codes(dev):
    """343 window codes do not fit a byte: asking for them is PF_ERR_UNSUPPORTED (-2), nothing is launched."""
    xyz = torch.randn(1, 3, 3, 9, 35, generator=torch.Generator().manual_seed(7)).to(dev)
    with pytest.raises(RuntimeError, match=r"pf_knn_lattice_f32 failed \(-2\)"):
        knn_lattice(xyz, 7, 16, with_codes=True)
    assert _lib.status() == 0
