"""The forward arms that only large shapes select (tables and checkers: tests/conv_fwd_cases.py): the deep tiles, the
several-tiles-per-block loop and the > 64 KiB LDS opt-in of pf_conv3d_k3_f32, the same loop of pf_conv3d_k3_pair_f32, the
channel groups and the matrix-core form of pf_deconv3d_k3s2_f32 as its shape rule picks them, the pointwise GEMM and the
EdgeConv gather passes above their block caps, and the lattice-kNN kernels of window 7 and window 1.  The operator tests
of tests/test_gpu_ops.py run TD 1, one tile per block and the kernels of window 3 / 5 only; the deep tiles were otherwise
reached at config sizes under composite tolerances.

Every case asserts the arm it exists for through the library's own plan query before it compares numbers; references are
float64; gates are those of tests/test_gpu_ops.py for the same entry point; every result is produced twice, bit for bit.
"""
import pytest

import conv_fwd_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,want,why", C.CONV_K3, ids=[C.tag_of(c) for c, _, _ in C.CONV_K3])
def test_conv3d_k3_deep_tiles_on_ragged_extents(dev, case, want, why):
    """(NT, stride, TD) in (2,1,4), (2,1,2), (1,1,2), (1,2,2), (2,2,2) with a partial last tile in D, H and W; two tiles
    per block under each TD; 77 376 bytes of LDS."""
    C.check_conv3d_plain(dev, case, want, "arm_conv3d")


@pytest.mark.parametrize("form", ["rows", "lazy"])
@pytest.mark.parametrize("case,want,why", C.CONV_K3_AFFINE, ids=[C.tag_of(c) for c, _, _ in C.CONV_K3_AFFINE])
def test_conv3d_k3_deep_tiles_apply_pending_batchnorm(dev, case, want, why, form):
    """aff_mode 1 (two different rows, sample n reads row n) and aff_mode 2 (resolved by every block, two samples per
    statistic) under TD 4 and TD 2."""
    C.check_conv3d_pending_batchnorm(dev, case, want, form, "arm_conv3d_bn")


@pytest.mark.parametrize("case,want,why", C.CONV_K3_TD1, ids=[C.tag_of(c) for c, _, _ in C.CONV_K3_TD1])
def test_conv3d_k3_td1_twins(dev, case, want, why):
    """The same channel counts and strides where pick_td leaves TD 1: what the deep-tile rows are twins of."""
    C.check_conv3d_plain(dev, case, want, "arm_conv3d_td1", ragged=False)
    for form in ("rows", "lazy"):
        C.check_conv3d_pending_batchnorm(dev, case, want, form, "arm_conv3d_td1_bn", ragged=False)


@pytest.mark.parametrize("case,want", C.CONV_PAIR, ids=[C.tag_of(c) for c, _ in C.CONV_PAIR])
def test_conv3d_pair_several_tiles_per_block(dev, case, want):
    C.check_conv3d_pair(dev, case, want, "arm_conv3d_pair")


def test_deconv3d_plan_honours_the_environment_switches(monkeypatch):
    C.check_deconv_plan_honours_the_switches(monkeypatch)


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("case,want,why", C.DECONV, ids=[C.tag_of(c) for c, _, _ in C.DECONV])
def test_deconv3d_forms_picked_by_the_shape_rule(dev, case, want, why, skip, monkeypatch):
    """CG 4, CG 2 and the matrix-core form with cells % 128 != 0, no environment switch."""
    C.check_deconv(dev, case, want, skip, monkeypatch, "arm_deconv3d")


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("form", ["rows", "lazy"])
@pytest.mark.parametrize("case,want,why", C.DECONV_AFFINE, ids=[C.tag_of(c) for c, _, _ in C.DECONV_AFFINE])
def test_deconv3d_forms_apply_pending_batchnorm(dev, case, want, why, form, skip, monkeypatch):
    C.check_deconv_pending_batchnorm(dev, case, want, skip, form, monkeypatch, "arm_deconv3d_bn")


@pytest.mark.parametrize("arm", C.GEMM_ARMS, ids=["pm%d_K%d_c%d" % (int(a[0]), a[1], a[2]) for a in C.GEMM_ARMS])
@pytest.mark.parametrize("groups,want", C.GEMM_GROUPS, ids=["G%d_Ng%d" % g for g, _ in C.GEMM_GROUPS])
def test_pointwise_gemm_several_tiles_per_block(dev, groups, want, arm):
    """The persistent loop of the direct-A and of the generic GEMM: two and three tiles per block, the last one partial,
    with affine rows and with statistics."""
    C.check_gemm(dev, groups, want, arm, "arm_gemm")


@pytest.mark.parametrize("Cc,k,gps,concat", C.EDGE_CASES,
                         ids=["C%d_k%d_gps%d_cat%d" % (c[0], c[1], c[2], int(c[3])) for c in C.EDGE_CASES])
def test_edgeconv_gather_passes_several_tiles_per_block(dev, Cc, k, gps, concat):
    """tile += T of edge_stats_kernel / edge_apply_kernel: 33 tiles on 17 blocks per group, the last tile partial."""
    C.check_edge_fused(dev, Cc, k, gps, concat, "arm_edgeconv")


@pytest.mark.parametrize("k", [16, 5])
def test_edgeconv_gather_passes_at_128_channels(dev, k):
    C.check_edge_passes_c128(dev, k, "arm_edgeconv")


@pytest.mark.parametrize("case", C.KNN_CASES, ids=[C.knn_id(c) for c in C.KNN_CASES])
def test_knn_lattice_kernels_of_window_7_and_1_and_small_k(dev, case):
    """knn_lattice_split_kernel, knn_lattice_kernel<8> / <16> / <32> and the sorting network below k = 16 against the brute
    force with the stated tie rule, exact duplicates planted."""
    C.check_knn(dev, *case)


def test_knn_window_7_reports_unsupported_for_codes(dev):
    C.check_knn_window7_has_no_codes(dev)
