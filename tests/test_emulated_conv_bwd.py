"""A subset of the convolution-backward edge tables (tests/conv_bwd_cases.py; the whole of them runs on an MI355X in
tests/test_gpu_conv_bwd_edges.py) EXECUTED on the CPU through tests/hipemu: the unchanged kernel sources against float64
autograd with the same checkers and the same gates, so that the indexing at ragged extents -- partial tiles in D, H and W,
patch rows that leave the tensor, Wi % 4 != 0 under the 16-byte staging, one-cell layers -- is checked wherever the package
builds, before hardware.  The emulator models neither races nor wave-level hazards nor the compiler's gfx950 code: those
are the GPU file's.

No plan-feature assertions here: without a device the plan's occupancy comes from the fallback arithmetic
(csrc/conv_wgrad.hip resident_blocks), which gives other splits and sometimes other tiles than the runtime's answer; the
plan that ran goes to the parity report.  The cases are those that take a few seconds on the host.

At the end: the cheapest rows of the forward-arm tables (tests/conv_fwd_cases.py) in the same manner.
"""
import os
import sys

import pytest
import torch

import conv_bwd_cases as _C

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cpu(lib_built):
    """The CPU as the device, tests/hipemu behind the C ABI (tests/hipemu/on_cpu.py)."""
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    from on_cpu import emulated_gpu
    with emulated_gpu():
        yield torch.device("cpu")


def _work(case):
    N, Cout, Cin, sp, k, stride, _ = case
    out = 1
    for s_ in sp:
        out *= (s_ - 1) // stride + 1
    return N * Cout * Cin * out * k ** len(sp)


# the weight-gradient cases of at most 1.1e8 multiply-adds (a few seconds each on the host): every tile of the fallback
# plans -- 4x4x16, 2x4x16, 1x16x16, 1x8x16, 1x4x16 --, stride 1 and 2, 3x3 / 5x5 / 3x3x3, CBP 4 / 8 / 16, partial channel
# blocks, the swapped form, affine and plain.  Left to the GPU: the 64 -> 64 layers (MT = 2) and the > 64 KB plans.
_EMU_3D = [(c, w) for c, w in _C.WGRAD_3D if _work(c) <= 1.1e8]
_EMU_2D = [(c, w) for c, w in _C.WGRAD_2D if _work(c) <= 1.1e8]
_EMU_DGRAD_3D = [r for r in _C.DGRAD_3D if r[4] in ((1, 1, 1), (3, 5, 7), (2, 3, 5), (1, 4, 17), (3, 5, 40), (2, 2, 4), (4, 6, 10))]


@pytest.mark.parametrize("case,want", _EMU_3D, ids=[_C.case_id(c) for c, _ in _EMU_3D])
def test_emulated_volume_weight_gradient_on_ragged_extents(cpu, case, want):
    _C.check_wgrad(cpu, case, want, "emulated_edge_wgrad3d_" + _C.case_id(case), False)


@pytest.mark.parametrize("case,want", _EMU_2D, ids=[_C.case_id(c) for c, _ in _EMU_2D])
def test_emulated_tower_weight_gradient_on_ragged_extents(cpu, case, want):
    _C.check_wgrad(cpu, case, want, "emulated_edge_wgrad2d_" + _C.case_id(case), False)


def test_emulated_transposed_weight_gradient_and_two_samples_per_statistic_group(cpu):
    for case, want in _C.WGRAD_TRANSPOSED:
        _C.check_wgrad_transposed(cpu, case, want, "emulated_edge_deconv_wgrad_%dto%d_%s" % (case[0], case[1],
                                                                                            _C.sp_tag(case[2])), False)
    _C.check_wgrad_two_samples_per_stat(cpu, "emulated_edge_wgrad2d_two_samples_per_stat")


@pytest.mark.parametrize("row", _EMU_DGRAD_3D, ids=[_C.dgrad3d_id(r) for r in _EMU_DGRAD_3D])
def test_emulated_volume_data_gradient_at_small_and_ragged_sizes(cpu, row):
    _C.check_dgrad3d(cpu, row, "emulated_edge_dgrad3d")


@pytest.mark.parametrize("row", _C.DGRAD_3D_FORCED_MFMA[:1] + _C.DGRAD_3D_FORCED_MFMA[2:3],
                         ids=[_C.dgrad3d_id(r) for r in _C.DGRAD_3D_FORCED_MFMA[:1] + _C.DGRAD_3D_FORCED_MFMA[2:3]])
def test_emulated_deconv_data_gradient_matrix_core_form(cpu, row, monkeypatch):
    monkeypatch.setenv("PF_DECONV_MFMA", "1")
    _C.check_dgrad3d(cpu, row, "emulated_edge_dgrad3d", forced_mfma=True)


@pytest.mark.parametrize("case", _C.DGRAD_2D, ids=["%dx%dto%d_%s_k%ds%d" % (c[0], c[2], c[1], _C.sp_tag(c[3]), c[4], c[5])
                                                   for c in _C.DGRAD_2D])
def test_emulated_tower_data_gradient_at_small_and_odd_maps(cpu, case):
    _C.check_dgrad2d(cpu, case, "emulated_edge_dgrad2d")


def test_support_predicates_reject_single_value_batchnorm_sizes(cpu):
    """train_ops.volume_supported / tower_supported at (8, 8, 8) and (8, 8): False (the predicates look at shapes only)."""
    _C.check_predicates_reject_single_value_batchnorm(cpu)


# ---------------------------------------------------------------------------------------------
# The cheapest rows of the forward-arm tables (tests/conv_fwd_cases.py; all of them run on an MI355X in
# tests/test_gpu_conv_fwd_arms.py), with the same checkers, plan assertions (those plans are pure functions of the shape)
# and gates.  Left to the GPU: the 512-block TD-4 and stride-2 rows and the > 2048-tile rows (tens of seconds each here),
# the matrix-core deconvolution by its shape rule (7 s), the GEMM and EdgeConv cases above their block caps, and the
# 67 584-point lattices of knn_lattice_kernel<8> / <16>.
# ---------------------------------------------------------------------------------------------
import conv_fwd_cases as _F     # noqa: E402


@pytest.mark.parametrize("case,want,why", _F.CONV_K3_TD1, ids=[_F.tag_of(c) for c, _, _ in _F.CONV_K3_TD1])
def test_emulated_conv3d_k3_td1_twins(cpu, case, want, why):
    _F.check_conv3d_plain(cpu, case, want, "emulated_arm_conv3d_td1", ragged=False)
    for form in ("rows", "lazy"):
        _F.check_conv3d_pending_batchnorm(cpu, case, want, form, "emulated_arm_conv3d_td1_bn", ragged=False)


def test_emulated_conv3d_k3_td2_last_depth_tile_partial(cpu):
    """The one deep-tile row that fits here: (4, 16, 7, 30, 250) stride 1, TD 2 on 512 blocks, 1 of 2 planes live in the
    last depth tile."""
    case, want, _ = _F.CONV_K3[4]
    _F.check_conv3d_plain(cpu, case, want, "emulated_arm_conv3d")


@pytest.mark.parametrize("case,want,why", _F.DECONV[:3], ids=[_F.tag_of(c) for c, _, _ in _F.DECONV[:3]])
def test_emulated_deconv3d_channel_groups_picked_by_the_shape_rule(cpu, case, want, why, monkeypatch):
    _F.check_deconv(cpu, case, want, True, monkeypatch, "emulated_arm_deconv3d")
    if (case, want, why) in _F.DECONV_AFFINE:
        for form in ("rows", "lazy"):
            _F.check_deconv_pending_batchnorm(cpu, case, want, False, form, monkeypatch, "emulated_arm_deconv3d_bn")


@pytest.mark.parametrize("case", _F.KNN_EMULATED, ids=[_F.knn_id(c) for c in _F.KNN_EMULATED])
def test_emulated_knn_lattice_window_7(cpu, case):
    _F.check_knn(cpu, *case)


def test_emulated_knn_window_7_reports_unsupported_for_codes(cpu):
    _F.check_knn_window7_has_no_codes(cpu)


@pytest.mark.parametrize("k", [16, 5])
def test_emulated_edgeconv_gather_passes_at_128_channels(cpu, k):
    _F.check_edge_passes_c128(cpu, k, "emulated_arm_edgeconv")


def test_composed_volume_path_raises_as_the_reference_does():
    """What model._run_autograd calls when volume_supported() is False -- ``self.coarse_vol_conv(cost)`` with an autograd
    graph, the ATen composition of VolumeConv.forward -- raises F.batch_norm's ValueError for an (8, 8, 8) volume, as the
    reference's networks.py does; (8, 8, 16) goes through.  No device work is involved: the raise needs no GPU."""
    from pointmvsnet_amd import networks
    vc = networks.VolumeConv(64, 8).train()
    cost = torch.zeros((1, 64, 8, 8, 8)).requires_grad_(True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        vc(cost)
    assert vc(torch.zeros((1, 64, 8, 8, 16)).requires_grad_(True)).shape == (1, 1, 8, 8, 16)
    tower = networks.ImageConv(8).train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        tower(torch.zeros((1, 3, 8, 8)).requires_grad_(True))
