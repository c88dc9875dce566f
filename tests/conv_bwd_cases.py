"""Case tables and float64 checkers of the convolution-backward edge tests: tests/test_gpu_conv_bwd_edges.py runs them on
an MI355X, tests/test_emulated_conv_bwd.py a subset on the CPU emulator (tests/hipemu).  A plain module, not a conftest.

The three backward families of the training step -- weight gradients (csrc/conv_wgrad.hip, whose launch plan is a
function of the shape AND of the occupancy the runtime reports), 2-D data gradients (pf_conv2d_wide_f32 on flipped
weights, pf_deconv2d_k5s2_f32) and the 3-D data gradients train_ops.py builds from forward kernels -- at extents that are
no multiple of a tile: tests/test_gpu_train_ops.py has even maps under the smallest tile only, and
tests/test_gpu_zz_train_cfg4.py reaches the large tiles at extents that divide by them.

Every reference is float64 autograd of F.conv2d / F.conv3d / F.conv_transpose3d on the same device; the gates are the
project's: weight gradient < 2e-5 of the largest entry, data gradient < 1e-5; every result is computed twice, bit-equal.
"""
import ctypes

import torch
import torch.nn.functional as F

from conftest import report
from pointmvsnet_amd import _lib, train_ops
from test_gpu_train_ops import _rel, _seeded
from test_gpu_zz_train_cfg4 import _PLAN_FIELDS, _plan_conv, _report_plan

WGRAD_GATE, DGRAD_GATE = 2e-5, 1e-5


def _out(sp, stride):
    return tuple((s - 1) // stride + 1 for s in sp)


def sp_tag(sp):
    return "x".join(str(s) for s in sp)


def case_id(case):
    N, Cout, Cin, sp, k, stride, affine = case[:7]
    return "%dx%dto%d_%s_k%ds%d%s" % (N, Cin, Cout, sp_tag(sp), k, stride, "_aff" if affine else "")


# ---------------------------------------------------------------------------------------------
# 1. weight gradients: (N, Cout, Cin, input size, k, stride, affine, the plan features the case exists for)
#
# A feature is one of
#   MT, TD, TH, CBP, stride       the exported plan number equals the value
#   per_split_ge, cblocks_ge      ... is at least the value
#   lds_gt                        lds_bytes exceeds the value (65536: the big-LDS opt-in)
#   last_cblock_partial           more than one channel block and Cx no multiple of a block's CBLK x CBP channels
#   swapped                       conv_wgrad exchanges the operands (stride 1, <= 8 output channels)
#   ragged                        letters of the extents that must NOT divide: D (Do % TD), H (Ho % TH), W (Wo % 16),
#                                 I (Wi % 4, the 16-byte staging of a patch row)
# asserted on the GPU through pf_conv_wgrad_plan, so that a case which stops reaching its branch fails instead of passing
# vacuously (the emulator's fallback occupancy gives other plans: there they are reported only).
# ---------------------------------------------------------------------------------------------
WGRAD_3D = [
    ((1, 8, 64, (10, 14, 50), 3, 1, False), dict(swapped=True, TD=4, TH=4, CBP=8, stride=1, ragged="DHWI")),
    ((1, 32, 32, (10, 18, 35), 3, 1, True), dict(TD=4, TH=4, MT=1, CBP=16, lds_gt=65536, ragged="DHWI")),
    ((1, 32, 32, (10, 18, 35), 3, 1, False), dict(TD=4, TH=4, lds_gt=65536, ragged="DHWI")),
    ((1, 24, 20, (10, 14, 35), 3, 1, True), dict(TD=4, TH=4, cblocks_ge=2, last_cblock_partial=True, ragged="DHWI")),
    ((1, 16, 16, (13, 18, 67), 3, 1, False), dict(TD=2, TH=4, ragged="DHWI")),
    ((1, 16, 16, (13, 18, 67), 3, 1, True), dict(TD=2, TH=4, ragged="DHWI")),
    ((1, 64, 64, (10, 14, 35), 3, 1, True), dict(MT=2, TD=2, TH=4, ragged="HWI")),
    ((1, 64, 64, (9, 14, 50), 3, 1, False), dict(MT=2, TD=2, TH=4, per_split_ge=2, ragged="DHWI")),
    ((1, 1, 8, (13, 18, 67), 3, 1, False), dict(swapped=True, CBP=4, ragged="DHWI")),
    ((1, 16, 64, (22, 26, 70), 3, 2, False), dict(stride=2, per_split_ge=2, TD=1, TH=4, lds_gt=65536, ragged="HWI")),
    ((1, 32, 16, (18, 22, 70), 3, 2, False), dict(stride=2, TD=1, TH=4, ragged="HWI")),
    ((1, 24, 20, (5, 9, 17), 3, 1, True), dict(TD=1, TH=4, cblocks_ge=2, last_cblock_partial=True, ragged="HWI")),
    ((1, 24, 20, (5, 9, 17), 3, 1, False), dict(TD=1, TH=4, ragged="HWI")),
    ((1, 16, 40, (3, 5, 7), 3, 1, False), dict(TD=1, TH=4, cblocks_ge=3, last_cblock_partial=True, ragged="HWI")),
    ((1, 16, 40, (3, 5, 7), 3, 1, True), dict(TD=1, TH=4, ragged="HWI")),
    ((1, 64, 32, (1, 3, 5), 3, 2, False), dict(stride=2, MT=1, ragged="HWI")),        # one deep, three depth taps
    ((1, 64, 64, (1, 1, 2), 3, 1, False), dict(TD=1, TH=8, ragged="HWI")),
    ((1, 32, 64, (1, 35, 53), 3, 1, True), dict(TD=1, TH=8, ragged="HWI")),           # one deep: the 2-D tiles, 27 taps
    ((1, 32, 64, (1, 35, 53), 3, 1, False), dict(TD=1, TH=8, ragged="HWI")),
]
WGRAD_2D = [
    ((3, 64, 64, (35, 52), 3, 1, True), dict(TD=1, TH=8, ragged="HW")),
    ((3, 64, 64, (35, 53), 3, 1, False), dict(TD=1, TH=8, ragged="HWI")),
    ((3, 64, 64, (70, 83), 3, 1, True), dict(MT=2, TD=1, TH=8, ragged="HWI")),
    ((3, 64, 64, (70, 83), 3, 1, False), dict(MT=2, TD=1, TH=8, ragged="HWI")),
    ((3, 16, 16, (90, 115), 3, 1, True), dict(MT=1, TD=1, TH=16, ragged="HWI")),
    ((3, 16, 16, (90, 115), 3, 1, False), dict(MT=1, TD=1, TH=16, ragged="HWI")),
    ((3, 32, 16, (66, 90), 5, 2, True), dict(stride=2, TD=1, TH=4, ragged="HWI")),
    ((3, 64, 32, (66, 90), 5, 2, True), dict(stride=2, TD=1, TH=8, cblocks_ge=2, ragged="HWI")),
    ((3, 16, 8, (70, 100), 5, 2, True), dict(stride=2, CBP=8, ragged="HW")),
    ((3, 16, 16, (50, 83), 3, 1, True), dict(TD=1, TH=4, MT=1, ragged="HWI")),
    ((2, 8, 3, (5, 3), 3, 1, False), dict(CBP=4, TD=1, TH=4, ragged="HWI")),
    ((2, 8, 6, (5, 3), 3, 1, True), dict(CBP=8, TD=1, TH=4, ragged="HWI")),
    ((1, 64, 64, (1, 1), 3, 1, False), dict(TD=1, TH=8, ragged="HWI")),
    ((1, 32, 16, (9, 13), 5, 2, True), dict(stride=2, TD=1, TH=4, ragged="HWI")),
    ((1, 32, 16, (9, 13), 5, 2, False), dict(stride=2, TD=1, TH=4, ragged="HWI")),
]
# the transposed form on a ragged coarse grid: (Cin, Cout, coarse size) -> fine = 2 x coarse
WGRAD_TRANSPOSED = [((32, 16, (3, 5, 7)), dict(stride=2, ragged="HWI"))]


def wgrad_plan(N, Cout, Cin, sp, k, stride, affine):
    """The plan of the launch conv_wgrad(dy, x, ...) makes for this layer, and whether it exchanges the operands."""
    nd = len(sp)
    osp = _out(sp, stride)
    go, xi, k3 = (1,) * (3 - nd) + osp, (1,) * (3 - nd) + tuple(sp), (1,) * (3 - nd) + (k,) * nd
    swapped = bool(train_ops.WGRAD_SWAP and stride == 1 and not affine and Cout <= 8 and Cout < Cin)
    if swapped:
        return _plan_conv(N, Cin, Cout, xi, go, k3, 1), True
    return _plan_conv(N, Cout, Cin, go, xi, k3, stride), False


def plan_misses(plan, swapped, want, geom):
    """The features of ``want`` the exported plan does not have (empty: the case reaches the branch it exists for).
    ``geom``: (Cx, (Do, Ho, Wo), Wi) of the LAUNCH."""
    p = dict(zip(_PLAN_FIELDS, plan))
    Cx, (Do, Ho, Wo), Wi = geom
    miss = []
    for key, val in want.items():
        if key in ("MT", "TD", "TH", "CBP", "stride"):
            ok = p[key] == val
        elif key == "per_split_ge":
            ok = p["per_split"] >= val
        elif key == "cblocks_ge":
            ok = p["cblocks"] >= val
        elif key == "lds_gt":
            ok = p["lds_bytes"] > val
        elif key == "last_cblock_partial":
            ok = p["cblocks"] > 1 and Cx % (p["CBLK"] * p["CBP"]) != 0
        elif key == "swapped":
            ok = swapped == val
        elif key == "ragged":
            checks = dict(D=Do % p["TD"], H=Ho % p["TH"], W=Wo % 16, I=Wi % 4)
            ok = all(checks[c] != 0 for c in val)
        else:
            raise KeyError(key)
        if not ok:
            miss.append((key, val))
    return miss


def check_wgrad(dev, case, want, tag, assert_plan):
    """conv_wgrad against float64 autograd of F.conv2d / F.conv3d, x raw with its pending BatchNorm + ReLU rows where
    ``affine``; twice, bit for bit; error and the twelve plan numbers to the parity report."""
    N, Cout, Cin, sp, k, stride, affine = case
    nd = len(sp)
    conv = F.conv2d if nd == 2 else F.conv3d
    osp = _out(sp, stride)
    x = _seeded((N, Cin) + tuple(sp), dev, 5)
    dy = _seeded((N, Cout) + osp, dev, 6)
    aff, xin = None, x.double()
    if affine:
        sc = (1.0 + 0.3 * _seeded((N, Cin), dev, 7)).contiguous()
        sh = (0.2 * _seeded((N, Cin), dev, 8)).contiguous()
        aff = (sc, sh)
        view = (N, Cin) + (1,) * nd
        xin = torch.relu(xin * sc.double().view(view) + sh.double().view(view))
    w = torch.zeros((Cout, Cin) + (k,) * nd, dtype=torch.float64, device=dev, requires_grad=True)
    conv(xin, w, None, stride, k // 2).backward(dy.double())
    run = lambda: train_ops.conv_wgrad(dy, x, (k,) * nd, stride, (k // 2,) * nd, aff, 1)    # noqa: E731
    dw = run()
    assert torch.equal(dw, run())
    err = _rel(dw, w.grad)
    plan, swapped = wgrad_plan(N, Cout, Cin, sp, k, stride, affine)
    _report_plan(tag, plan, rel=err, swapped=float(swapped))
    assert dw.shape == w.shape and err < WGRAD_GATE, (err, plan)
    if assert_plan:
        o3, i3 = (1,) * (3 - nd) + osp, (1,) * (3 - nd) + tuple(sp)
        geom = (Cout, i3, osp[-1]) if swapped else (Cin, o3, sp[-1])
        miss = plan_misses(plan, swapped, want, geom)
        assert not miss, (miss, dict(zip(_PLAN_FIELDS, plan)))
    return err, plan


def check_wgrad_transposed(dev, case, want, tag, assert_plan):
    """ConvTranspose3d(3, stride 2, padding 1, output_padding 1): the layer input on the coarse grid is the launch's
    ``gr``, dL/dy on the fine grid its ``x``; against autograd of F.conv_transpose3d, (Cin, Cout, 3, 3, 3) order."""
    Cin, Cout, sp = case
    fine = tuple(2 * s for s in sp)
    x = _seeded((1, Cin) + tuple(sp), dev, 9)
    dy = _seeded((1, Cout) + fine, dev, 10)
    w = torch.zeros((Cin, Cout, 3, 3, 3), dtype=torch.float64, device=dev, requires_grad=True)
    F.conv_transpose3d(x.double(), w, None, 2, 1, 1).backward(dy.double())
    run = lambda: train_ops.conv_wgrad(x, dy, (3, 3, 3), 2, (1, 1, 1))                      # noqa: E731
    dw = run()
    assert torch.equal(dw, run())
    err = _rel(dw, w.grad)
    plan = _plan_conv(1, Cin, Cout, sp, fine, (3, 3, 3), 2)
    _report_plan(tag, plan, rel=err)
    assert dw.shape == w.shape and err < WGRAD_GATE, (err, plan)
    if assert_plan:
        miss = plan_misses(plan, False, want, (Cout, tuple(sp), fine[-1]))
        assert not miss, (miss, dict(zip(_PLAN_FIELDS, plan)))
    return err, plan


def check_wgrad_two_samples_per_stat(dev, tag):
    """pf_conv_wgrad_f32's x_samples_per_stat = 2: four samples, two rows of pending BatchNorm + ReLU, sample n takes
    row n // 2."""
    N, Cout, Cin, sp, k = 4, 16, 16, (7, 19), 3
    x = _seeded((N, Cin) + sp, dev, 5)
    dy = _seeded((N, Cout) + sp, dev, 6)
    sc = (1.0 + 0.3 * _seeded((2, Cin), dev, 7)).contiguous()
    sh = (0.2 * _seeded((2, Cin), dev, 8)).contiguous()
    rows = torch.arange(N, device=dev) // 2
    xin = torch.relu(x.double() * sc.double()[rows].view(N, Cin, 1, 1) + sh.double()[rows].view(N, Cin, 1, 1))
    w = torch.zeros((Cout, Cin, k, k), dtype=torch.float64, device=dev, requires_grad=True)
    F.conv2d(xin, w, None, 1, 1).backward(dy.double())
    run = lambda: train_ops.conv_wgrad(dy, x, (k, k), 1, (1, 1), (sc, sh), 2)               # noqa: E731
    dw = run()
    assert torch.equal(dw, run())
    err = _rel(dw, w.grad)
    # the same rows, one per sample, must give the same bits (the row index is the only thing sps changes)
    per_sample = train_ops.conv_wgrad(dy, x, (k, k), 1, (1, 1), (sc[rows].contiguous(), sh[rows].contiguous()), 1)
    plan, _ = wgrad_plan(N, Cout, Cin, sp, k, 1, True)
    _report_plan(tag, plan, rel=err)
    assert err < WGRAD_GATE, (err, plan)
    assert torch.equal(dw, per_sample)
    return err


# ---------------------------------------------------------------------------------------------
# 2. the queue's capacity limits
# ---------------------------------------------------------------------------------------------
def check_queue(dev, layers, tag):
    """``layers``: [(N, Cout, Cin, size, k, stride)], each with tensors and an ``into`` slot of its own, pre-filled with a
    constant; queued inside direct_grads(True) and flushed once through flush_late() and once through
    queue.flush_node().  Every slot minus its constant equals the stand-alone conv_wgrad of that layer to 2e-6 (the
    batched launch runs the same plan; the difference is the float32 add into the pre-filled slot), the stand-alone
    result meets the float64 gate, and the two flush routes agree bit for bit."""
    queue = train_ops.wgrad_queue
    tensors, alone = [], []
    for i, (N, Cout, Cin, sp, k, stride) in enumerate(layers):
        nd = len(sp)
        x = _seeded((N, Cin) + tuple(sp), dev, 100 + 2 * i)
        dy = _seeded((N, Cout) + _out(sp, stride), dev, 101 + 2 * i)
        tensors.append((dy, x, (k,) * nd, stride, (k // 2,) * nd))
        alone.append(train_ops.conv_wgrad(dy, x, (k,) * nd, stride, (k // 2,) * nd))
    # float64 autograd of the first, the ninth (first of the second launch of an instantiation), the seventeenth (first
    # of the second reduce launch) and the last layer
    worst64 = 0.0
    for i in sorted(set((0, 8, 16, len(layers) - 1)) & set(range(len(layers)))):
        dy, x, kk, stride, pad = tensors[i]
        w = torch.zeros(alone[i].shape, dtype=torch.float64, device=dev, requires_grad=True)
        (F.conv2d if len(kk) == 2 else F.conv3d)(x.double(), w, None, stride, pad[0]).backward(dy.double())
        worst64 = max(worst64, _rel(alone[i], w.grad))
    got = {}
    for route in ("late", "node"):
        consts = [0.25 + 0.125 * (i % 5) for i in range(len(layers))]
        slots = [torch.full(a.shape, c, dtype=torch.float32, device=dev) for a, c in zip(alone, consts)]
        torch.cuda.synchronize()
        with train_ops.direct_grads(True):
            with torch.cuda.stream(torch.cuda.current_stream() if route == "late" else torch.cuda.Stream()):
                for (dy, x, kk, stride, pad), slot in zip(tensors, slots):
                    assert train_ops.conv_wgrad(dy, x, kk, stride, pad, into=slot) is None
                waiting, other = (queue.late, queue.node) if route == "late" else (queue.node, queue.late)
                assert len(waiting) == len(layers) and not other
                if route == "late":
                    train_ops.flush_late()
                else:
                    queue.flush_node()
                assert not queue.late and not queue.node
        torch.cuda.synchronize()
        got[route] = [s - c for s, c in zip(slots, consts)]
    worst = max(_rel(g, a) for g, a in zip(got["late"], alone))
    report(tag, rel_vs_alone=worst, rel_alone_vs_float64=worst64, layers=len(layers))
    assert worst < 2e-6 and worst64 < WGRAD_GATE, (worst, worst64)
    for a, b in zip(got["late"], got["node"]):
        assert torch.equal(a, b)
    return worst


QUEUE_ONE = [(2, 16, 16, (7, 19), 3, 1)] * 19
# two instantiations interleaved (stride 1 / stride 2): the grouping loop of pf_conv_wgrad_batch_f32 skips the other
# instantiation's entries, flushes at eight and returns to them
QUEUE_MIXED = [(2, 16, 16, (7, 19), 3, 1) if i % 2 == 0 else (2, 16, 16, (7, 19), 5, 2) for i in range(19)]


# ---------------------------------------------------------------------------------------------
# 3. data gradients
# ---------------------------------------------------------------------------------------------
# 3-D: rows of tests/test_gpu_zz_train_cfg4.py's VOLUME table (name, kind, Cout, Cin, _, stride) -- the name selects the
# helper _VolumeTrain.backward uses -- at small layer-input sizes
_SIZES_C1 = [(1, 1, 1), (3, 5, 7), (8, 8, 16), (2, 9, 70)]
_SIZES_CONV = [(1, 1, 1), (2, 3, 5), (1, 4, 17), (4, 4, 8), (3, 5, 40)]
_SIZES_DECONV = [(2, 2, 2), (2, 2, 4), (4, 6, 10), (2, 8, 34)]
DGRAD_3D = [("conv6_2", "conv", 1, 8, sp, 1) for sp in _SIZES_C1]                      # pf_conv3d_k3_c1_f32
for _sp in _SIZES_CONV:
    DGRAD_3D += [("conv6_0", "deconv", 8, 16, _sp, 2), ("conv5_0", "deconv", 16, 32, _sp, 2),   # _conv3d_k3_w / 2
                 ("conv4_0", "deconv", 32, 64, _sp, 2),                                         # _conv3d_bottom_w / 2
                 ("conv3_1", "conv", 64, 64, _sp, 1),                                           # _conv3d_bottom_w(flip_t)
                 ("conv2_1", "conv", 32, 32, _sp, 1), ("conv1_1", "conv", 16, 16, _sp, 1),      # conv3d_dgrad_flip
                 ("conv0_1", "conv", 8, 64, _sp, 1)]                                            # ... in two halves
for _sp in _SIZES_DECONV:
    DGRAD_3D += [("conv3_0", "conv", 64, 32, _sp, 2),                                           # _deconv3d_bottom_w
                 ("conv2_0", "conv", 32, 16, _sp, 2), ("conv1_0", "conv", 16, 64, _sp, 2)]      # deconv3d_k3s2
# pf_deconv3d_k3s2_f32 as a gradient has two forms (csrc/deconv3d.hip): lane-per-cell and matrix-core.  Its shape rule
# takes the matrix-core form from 508 blocks of 128 coarse cells x 16 output channels on (conv1_0 at >= 16 257 coarse
# cells: a 33 MB gradient), so at these sizes it is selected through PF_DECONV_MFMA=1, the switch the rule itself reads.
DGRAD_3D_FORCED_MFMA = [("conv2_0", "conv", 32, 16, sp, 2) for sp in _SIZES_DECONV[2:]] + \
                       [("conv1_0", "conv", 16, 64, sp, 2) for sp in _SIZES_DECONV[2:]]


def deconv_form(Cin, Cout, coarse, forced):
    """Which form pf_deconv3d_k3s2_f32 runs (its dispatch, csrc/deconv3d.hip): 1.0 matrix-core, 0.0 lane-per-cell."""
    cells = coarse[0] * coarse[1] * coarse[2]
    ok = Cin % 4 == 0 and Cin <= 32
    pays = Cout >= 32 and -(-cells // 128) * -(-Cout // 16) >= 512
    return 1.0 if ok and (pays or forced) else 0.0


def dgrad3d_id(row):
    return "%s_%s" % (row[0], sp_tag(row[4]))


def check_dgrad3d(dev, row, prefix, forced_mfma=False):
    """One row through the dispatch of test_volume_data_gradient_at_cfg4_shape (float64 autograd of F.conv3d /
    F.conv_transpose3d, output shape, < 1e-5, twice bit for bit, under no_pack_cache())."""
    import test_gpu_zz_train_cfg4 as Z
    name, kind, Cout, Cin, sp, stride = row
    tag = "%s_%s_%s%s" % (prefix, name, sp_tag(sp), "_mfma" if forced_mfma else "")
    extra = None
    if name in ("conv2_0", "conv1_0"):          # the launch: Cin' = the layer's Cout, Cout' = its Cin, on the coarse grid
        extra = dict(deconv_mfma_form=deconv_form(Cout, Cin, _out(sp, 2), forced_mfma))
    return Z.test_volume_data_gradient_at_cfg4_shape(dev, name, kind, Cout, Cin, tuple(sp), stride, tag=tag, extra=extra)


# 2-D: (N, Cout, Cin, input size, k, stride); stride 2 writes (2 Ho, 2 Wo), so inputs are even there
DGRAD_2D = [(1, 8, 8, (1, 1), 3, 1), (2, 64, 64, (9, 13), 3, 1), (1, 16, 16, (5, 3), 3, 1), (3, 32, 32, (7, 33), 3, 1),
            (1, 16, 8, (2, 2), 5, 2), (2, 32, 16, (10, 14), 5, 2), (1, 64, 32, (18, 26), 5, 2)]


def check_dgrad2d(dev, case, prefix):
    N, Cout, Cin, sp, k, stride = case
    x = torch.zeros((N, Cin) + tuple(sp), dtype=torch.float64, device=dev, requires_grad=True)
    w = _seeded((Cout, Cin, k, k), dev, 15, 0.2)
    dy = _seeded((N, Cout) + _out(sp, stride), dev, 16)
    F.conv2d(x, w.double(), None, stride, k // 2).backward(dy.double())
    dx = train_ops.conv2d_dgrad(dy, w, stride)
    assert torch.equal(dx, train_ops.conv2d_dgrad(dy, w, stride))
    err = _rel(dx, x.grad)
    report("%s_%dx%dto%d_%s_k%ds%d" % (prefix, N, Cin, Cout, sp_tag(sp), k, stride), rel=err)
    assert dx.shape == x.shape and err < DGRAD_GATE, err
    return err


# ---------------------------------------------------------------------------------------------
# the support predicates
# ---------------------------------------------------------------------------------------------
def check_predicates_reject_single_value_batchnorm(dev):
    """An (8, 8, 8) volume and an (8, 8) view leave the bottom BatchNorms one value per channel and statistic group: the
    reference raises there (F.batch_norm), so the fused nodes must not take such a size."""
    from pointmvsnet_amd import networks
    vc = networks.VolumeConv(64, 8).to(dev).train()
    tower = networks.ImageConv(8).to(dev).train()
    vol = lambda *s: torch.zeros((1, 64) + s, device=dev)        # noqa: E731
    img = lambda *s: torch.zeros((3, 3) + s, device=dev)         # noqa: E731
    assert not train_ops.volume_supported(vc, vol(8, 8, 8))
    assert train_ops.volume_supported(vc, vol(8, 8, 16)) and train_ops.volume_supported(vc, vol(16, 8, 8))
    assert not train_ops.tower_supported(tower, img(8, 8))
    assert train_ops.tower_supported(tower, img(8, 16)) and train_ops.tower_supported(tower, img(16, 8))
