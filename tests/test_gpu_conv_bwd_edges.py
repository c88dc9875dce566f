"""The convolution backward of the training step at its edges (pointmvsnet_amd/train_ops.py; csrc/conv_wgrad.hip,
csrc/conv_dgrad.hip and the forward kernels the 3-D data gradients re-use): extents that are no multiple of the tile under
EVERY launch plan of the weight-gradient kernel, the capacity limits of its batched launch and batched reduce, and the
data-gradient helpers at small and ragged sizes.  tests/test_gpu_train_ops.py has even maps under the smallest tile,
tests/test_gpu_zz_train_cfg4.py the large tiles at extents they divide: a large tile had not met a partial tile in D, H or
W, a patch row leaving the tensor, or Wi % 4 != 0 under the 16-byte staging.

Tables and checkers: tests/conv_bwd_cases.py (tests/test_emulated_conv_bwd.py runs a subset on the CPU emulator).  Every
reference is float64 autograd of F.conv2d / F.conv3d / F.conv_transpose3d on the same device; gates: weight gradient
< 2e-5 of the largest entry, data gradient < 1e-5; every result twice, bit for bit.  The weight-gradient plan depends on
the occupancy the runtime reports, so a case names the plan features it exists for and asserts them through
pf_conv_wgrad_plan: a case that stops reaching its branch fails instead of passing vacuously.
"""
import pytest

import conv_bwd_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,want", C.WGRAD_3D, ids=[C.case_id(c) for c, _ in C.WGRAD_3D])
def test_volume_weight_gradient_on_ragged_extents(dev, case, want):
    """3x3x3 layers, stride 1 and 2: the tiles 4x4x16, 2x4x16, 1x8x16, 1x4x16, MT = 1 and 2, per_split >= 2, CBP 4 / 8 / 16,
    a partial last channel block, Cg no multiple of 16, lds_bytes > 64 KB, the swapped-operand form, a depth of one under
    three depth taps -- with and without the pending BatchNorm + ReLU of x (the patch's interior fast path is skipped under
    it) -- each with Do % TD, Ho % TH, Wo % 16 and Wi % 4 != 0 as the case's ``ragged`` says."""
    C.check_wgrad(dev, case, want, "edge_wgrad3d_" + C.case_id(case), True)


@pytest.mark.parametrize("case,want", C.WGRAD_2D, ids=[C.case_id(c) for c, _ in C.WGRAD_2D])
def test_tower_weight_gradient_on_ragged_extents(dev, case, want):
    """3x3 / 1 and 5x5 / 2 layers on three views: the tiles 1x16x16, 1x8x16, 1x4x16, MT = 2, CBP 4 / 8 / 16, odd maps down to
    1x1 (what a 520x648 image leaves at the bottom is 65x81)."""
    C.check_wgrad(dev, case, want, "edge_wgrad2d_" + C.case_id(case), True)


@pytest.mark.parametrize("case,want", C.WGRAD_TRANSPOSED, ids=["%dto%d_%s" % (c[0], c[1], C.sp_tag(c[2]))
                                                               for c, _ in C.WGRAD_TRANSPOSED])
def test_transposed_weight_gradient_on_a_ragged_coarse_grid(dev, case, want):
    C.check_wgrad_transposed(dev, case, want, "edge_deconv_wgrad_%dto%d_%s" % (case[0], case[1], C.sp_tag(case[2])), True)


def test_weight_gradient_with_two_samples_per_statistic_group(dev):
    """x_samples_per_stat = 2 of pf_conv_wgrad_f32 (shipped ABI, the step calls it with 1): sample n reads affine row
    n // 2."""
    C.check_wgrad_two_samples_per_stat(dev, "edge_wgrad2d_two_samples_per_stat")


@pytest.mark.parametrize("layers,name", [(C.QUEUE_ONE, "one_instantiation"), (C.QUEUE_MIXED, "two_instantiations")])
def test_nineteen_queued_weight_gradients_cross_both_batch_limits(dev, layers, name):
    """pf_conv_wgrad_batch_f32 flushes at 8 entries of one instantiation, pf_wgrad_reduce_batch_f32 takes 16 per launch:
    19 queued layers need three launches of the first and two of the second; with two instantiations interleaved the
    grouping loop also skips entries and returns to them."""
    C.check_queue(dev, layers, "edge_wgrad_queue_19_" + name)


@pytest.mark.parametrize("row", C.DGRAD_3D, ids=[C.dgrad3d_id(r) for r in C.DGRAD_3D])
def test_volume_data_gradient_at_small_and_ragged_sizes(dev, row):
    """Every data-gradient helper of _VolumeTrain.backward through the dispatch of the cfg-4 test, at layer-input sizes from
    one cell to a W that crosses a tile."""
    C.check_dgrad3d(dev, row, "edge_dgrad3d")


@pytest.mark.parametrize("row", C.DGRAD_3D_FORCED_MFMA, ids=[C.dgrad3d_id(r) for r in C.DGRAD_3D_FORCED_MFMA])
def test_deconv_data_gradient_matrix_core_form_at_ragged_sizes(dev, row, monkeypatch):
    """pf_deconv3d_k3s2_f32 as a gradient in its matrix-core form (PF_DECONV_MFMA=1: the shape rule takes it from ~16 000
    coarse cells on); the rows above ran the lane-per-cell form the rule picks at these sizes."""
    monkeypatch.setenv("PF_DECONV_MFMA", "1")
    C.check_dgrad3d(dev, row, "edge_dgrad3d", forced_mfma=True)


@pytest.mark.parametrize("case", C.DGRAD_2D, ids=["%dx%dto%d_%s_k%ds%d" % (c[0], c[2], c[1], C.sp_tag(c[3]), c[4], c[5])
                                                  for c in C.DGRAD_2D])
def test_tower_data_gradient_at_small_and_odd_maps(dev, case):
    """conv2d_dgrad (pf_conv2d_wide_f32 on the flipped weight, pf_deconv2d_k5s2_f32) on the 5x3 .. 9x13 maps the step itself
    produces for a 40x56 or 72x104 image, and on one cell."""
    C.check_dgrad2d(dev, case, "edge_dgrad2d")


def test_support_predicates_reject_single_value_batchnorm_sizes(dev):
    C.check_predicates_reject_single_value_batchnorm(dev)
