"""The batched confidence filter (pointmvsnet_amd/scan.py, csrc/scan_filter.hip).

Yardsticks: the project's own host functions for what is pinned to the reference (``eval_file_logger_host`` +
``probability_filter(..., "NEAREST")`` and ``AsyncEvalWriter(filter_thresholds=...)``: bit for bit), and for the
interpolating modes a float64 statement of the resampling specification in scan.py's docstring, written here from the
formulas (``statement_weights`` / ``statement_resize``: scalar Python, a direct non-separable double sum; it does not call
``resize_taps``).  OpenCV is not installed: parity with ``cv2.resize`` is neither claimed nor tested.

The tolerance of the GPU comparison
-----------------------------------
The kernel sums T products per axis in float32 with float32 weights.  Per output pixel: every weight is rounded once
(1 eps relative, eps = 2^-24), every product once, the T - 1 additions of a pass once each relative to a partial sum that
is at most sum|w| max|src|: at most T + 1 roundings per pass on top of the rounded input of the second pass, 2 T + 2 in
all; rounded up to ``(2 T + 4) eps sum|wy| sum|wx| max|src|`` per pixel, derived from the statement's own float64 weights.
The keep / zero decision must equal the statement's wherever the statement's confidence is further than that bound from
its threshold; inside the band either answer is accepted, and the band may hold at most 0.1 % of the pixels (asserted on
the statement alone, also in the host test below; measured there: at most 1 pixel of 55 296 per case).
"""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, report
from pointmvsnet_amd import scan as S
from pointmvsnet_amd.utils import eval_file_logger as EL
from pointmvsnet_amd.utils import io as IO

EPS32 = 2.0 ** -24
BAND_CAP = 1e-3
INIT_THR, FLOW_THR = 0.2, 0.1
MODES = ("NEAREST", "BILINEAR", "CUBIC", "LANCZOS4")
TAPS = {"NEAREST": 1, "BILINEAR": 2, "CUBIC": 4, "LANCZOS4": 8}
V3, H, W = 3, 96, 192
COARSE = ((H // 2, W // 2), (H // 4, W // 4), (37, 53))             # 1/2, 1/4 and a non-integer ratio
PAIRS = [(8, 8), (8, 16), (8, 32), (16, 8), (7, 19), (19, 7), (53, 192), (37, 96), (100, 33), (1, 5), (5, 1), (3, 64),
         (24, 48), (200, 640), (641, 160)]


# ---------------------------------------------------------------------------------------------------------------------
# the float64 statement
# ---------------------------------------------------------------------------------------------------------------------
def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)


def statement_weights(s, n, mode):
    """[(source indices, weights)] per destination index, from the formulas of the specification (scalar Python)."""
    out = []
    for i in range(n):
        if mode == "NEAREST":
            out.append(([min(int(math.floor(i * (s / float(n)))), s - 1)], [1.0]))
            continue
        f = (i + 0.5) * (s / float(n)) - 0.5
        i0 = math.floor(f)
        t = f - i0
        if mode == "BILINEAR":
            ks, ws = [0, 1], [1.0 - t, t]
        elif mode == "CUBIC":
            A = -0.75
            w0 = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A
            w1 = ((A + 2) * t - (A + 3)) * t * t + 1
            w2 = ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1
            ks, ws = [-1, 0, 1, 2], [w0, w1, w2, 1.0 - w0 - w1 - w2]
        else:
            ks = list(range(-3, 5))
            if t == 0.0:
                ws = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
            else:
                raw = [_sinc(t - k) * _sinc((t - k) / 4.0) if abs(t - k) < 4.0 else 0.0 for k in ks]
                total = sum(raw)
                ws = [r / total for r in raw]
        out.append(([min(max(int(i0) + k, 0), s - 1) for k in ks], ws))
    return out


def statement_resize(src, h, w, mode):
    """``(resized (h, w) float64, sum|wy| (h,), sum|wx| (w,))``: out[y, x] = sum_ky sum_kx wy wx src[iy, ix], directly."""
    src = np.asarray(src, np.float64)
    rows, cols = statement_weights(src.shape[0], h, mode), statement_weights(src.shape[1], w, mode)
    iy = np.array([r[0] for r in rows])                                      # (h, T)
    wy = np.array([r[1] for r in rows])
    ix = np.array([c[0] for c in cols])                                      # (w, T)
    wx = np.array([c[1] for c in cols])
    out = np.zeros((h, w))
    for ky in range(iy.shape[1]):
        for kx in range(ix.shape[1]):
            out += (wy[:, ky][:, None] * wx[:, kx][None, :]) * src[iy[:, ky]][:, ix[:, kx]]
    return out, np.abs(wy).sum(axis=1), np.abs(wx).sum(axis=1)


def bound_of(src, h, w, mode):
    """``(statement's resized map, per-pixel bound)`` of the module docstring."""
    out, ay, ax = statement_resize(src, h, w, mode)
    return out, (2 * TAPS[mode] + 4) * EPS32 * ay[:, None] * ax[None, :] * float(np.abs(src).max())


def separable_f64(src, h, w, mode):
    """The tables of resize_taps evaluated in float64: horizontally first, then vertically, ascending taps."""
    src = np.asarray(src, np.float64)
    ys, wy = S.resize_taps(src.shape[0], h, mode)
    xs, wx = S.resize_taps(src.shape[1], w, mode)
    T = wy.shape[1]
    strip = sum(src[:, np.clip(xs + k, 0, src.shape[1] - 1)] * wx[:, k][None, :] for k in range(T))
    return sum(strip[np.clip(ys + k, 0, src.shape[0] - 1)] * wy[:, k][:, None] for k in range(T))


def operator_of(s, n, mode):
    start, weights = S.resize_taps(s, n, mode)
    M = np.zeros((n, s))
    for i in range(n):
        for k in range(weights.shape[1]):
            M[i, min(max(int(start[i]) + k, 0), s - 1)] += weights[i, k]
    return M


def make_predictions(coarse_hw, seed, flow_hw=None):
    """Random predictions of a 3-view scan: depths, 5 hypothesis probabilities that sum to 1, coarse confidences."""
    g = torch.Generator().manual_seed(seed)
    depths = 400.0 + 300.0 * torch.rand(V3, H, W, generator=g)
    flow = torch.rand(V3, 5, H, W, generator=g) ** 2
    flow = flow / flow.sum(dim=1, keepdim=True)
    init = torch.rand(V3, coarse_hw[0], coarse_hw[1], generator=g)
    made = None if flow_hw is None else 0.5 * torch.rand(V3, flow_hw[0], flow_hw[1], generator=g)
    return depths, flow, init, made


def flow_confidence_of(flow):
    return np.stack([EL.flow_confidence_np(f.permute(1, 2, 0).numpy()) for f in flow])


def statement_decision(depths, flow_conf, flow_resize, init, mode):
    """``(keep (V, h, w) bool, band (V, h, w) bool, resized init, init bound, resized flow, flow bound)`` in float64;
    ``flow_resize``: the flow confidence is a made map that the filter resizes (else it is compared as it is)."""
    keep, band, ri, bi, rf, bf = [], [], [], [], [], []
    for v in range(depths.shape[0]):
        a, ba = bound_of(init[v].numpy(), H, W, mode)
        if flow_resize:
            f, bfv = bound_of(flow_conf[v], H, W, mode)
        else:
            f, bfv = flow_conf[v].astype(np.float64), np.zeros((H, W))
        keep.append(~(f < FLOW_THR) & ~(a < INIT_THR))
        band.append((np.abs(a - INIT_THR) <= ba) | ((np.abs(f - FLOW_THR) <= bfv) & flow_resize))
        ri.append(a), bi.append(ba), rf.append(f), bf.append(bfv)
    return tuple(np.stack(t) for t in (keep, band, ri, bi, rf, bf))


# ---------------------------------------------------------------------------------------------------------------------
# 1. without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_tables_are_a_partition_of_unity():
    for mode in MODES:
        for s, n in PAIRS:
            start, weights = S.resize_taps(s, n, mode)
            assert start.shape == (n,) and weights.shape == (n, TAPS[mode]) and weights.dtype == np.float64
            assert np.abs(weights.sum(axis=1) - 1.0).max() <= 1e-15, (mode, s, n)
            assert (np.diff(start) >= 0).all()                              # what the kernel's LDS footprint relies on
            for tile in (8, 32):                                            # the first taps of a tile lie this close
                for first in range(0, n, tile):
                    last = min(first + tile - 1, n - 1)
                    assert start[last] - start[first] <= (tile - 1) * s // n + 1, (mode, s, n, first)
    with pytest.raises(ValueError):
        S.resize_taps(4, 8, "AREA")
    with pytest.raises(ValueError):
        S.resize_taps(0, 8, "CUBIC")


def test_equal_sizes_give_the_identity_exactly():
    for mode in MODES:
        for s in (1, 2, 7, 64, 193):
            assert np.array_equal(operator_of(s, s, mode), np.eye(s)), (mode, s)
            start, weights = S.resize_taps(s, s, mode)
            assert set(np.unique(weights)) <= {0.0, 1.0}
    w = S.resize_taps(16, 32, "LANCZOS4")[1]
    assert not np.array_equal(w[0], np.eye(8)[3]) and abs(w[0].sum() - 1) < 1e-15      # t = 0.25: a real kernel


def test_nearest_indices_are_those_of_the_file_route():
    for s, n in PAIRS:
        start, weights = S.resize_taps(s, n, "NEAREST")
        want = EL._resize_nearest(np.arange(s)[:, None].repeat(2, 1), n, 2)[:, 0]
        assert np.array_equal(start, want) and np.array_equal(weights, np.ones((n, 1)))


def test_tables_agree_with_the_independent_statement():
    rng = np.random.default_rng(0)
    worst = 0.0
    for mode in MODES:
        for (sh, sw), (h, w) in (((24, 48), (96, 192)), ((48, 96), (96, 192)), ((37, 53), (96, 192)), ((50, 70), (20, 33)),
                                 ((9, 11), (9, 40)), ((1, 6), (5, 13))):
            src = rng.uniform(-1.0, 1.0, (sh, sw))
            want, _, _ = statement_resize(src, h, w, mode)
            err = float(np.abs(separable_f64(src, h, w, mode) - want).max())
            worst = max(worst, err)
            assert err <= 1e-12, (mode, sh, sw, h, w, err)
    print("largest |tables - statement|", worst)
    # a closed form: bilinear 2x of a ramp is the ramp sampled at the half-pixel centres, clamped at the border
    ramp = np.arange(8.0)[None, :].repeat(2, 0)
    got, _, _ = statement_resize(ramp, 2, 16, "BILINEAR")
    assert np.allclose(got[0], np.clip((np.arange(16) + 0.5) / 2 - 0.5, 0, 7), atol=1e-15)
    # cubic and Lanczos reproduce a constant
    for mode in ("CUBIC", "LANCZOS4"):
        assert np.abs(statement_resize(np.full((9, 9), 3.5), 31, 17, mode)[0] - 3.5).max() < 1e-14


def test_statement_band_stays_under_the_cap():
    """The share of pixels whose float64 confidence lies within the kernel's error bound of its threshold, for the very
    inputs of the GPU test, on the statement alone."""
    shares = {}
    for mode in MODES[1:]:
        for c, coarse in enumerate(COARSE):
            for made in (None, coarse):
                depths, flow, init, flow_made = make_predictions(coarse, 10 + c, made)
                conf = flow_made.numpy() if made else flow_confidence_of(flow)
                keep, band, _, bi, _, _ = statement_decision(depths.numpy(), conf, made is not None, init, mode)
                shares[(mode, coarse, made is not None)] = float(band.mean())
                assert band.mean() <= BAND_CAP and 0.05 < keep.mean() < 0.95
                assert bi.max() < 1e-5
    print("band shares", shares)


def _header_params(name):
    text = open(os.path.join(ROOT, "include", "pointflow_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def test_abi_declares_binds_and_builds_the_scan_filter(lib_built):
    import ctypes
    import test_abi
    test_abi.test_header_library_and_bindings_agree(lib_built)
    from pointmvsnet_amd import _lib, build
    assert {"pf_scan_filter_f32", "pf_scan_filter_supported"} <= set(_lib.PROTOTYPES) and "scan_filter.hip" in build.SOURCES
    for name in ("pf_scan_filter_f32", "pf_scan_filter_supported"):
        params, (argtypes, restype) = _header_params(name), _lib.PROTOTYPES[name]
        assert len(params) == len(argtypes) and restype is ctypes.c_int
        for p, a in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else ctypes.c_float if p.startswith("float ") else ctypes.c_int
            assert a is want, (name, p)
    usage = json.load(open(build.USAGE_FILE))["scan_filter.hip"]
    kernels = [k for k in usage if "scan_filter_kernel" in k]
    assert len(kernels) == 4                                                # 1, 2, 4 and 8 taps
    for k in kernels:
        assert usage[k]["scratch_bytes_per_lane"] == 0, k
    header = open(os.path.join(ROOT, "include", "pointflow_hip.h")).read()
    for mode, (code, taps) in S.MODES.items():
        assert "#define PF_SCAN_%s %d" % (mode, code) in header and taps == TAPS[mode]
    # the *_supported rule: the four modes, upsampling by any factor, a shrink whose LDS tile exceeds 48 KiB is refused
    lib = _lib.load()
    for code, _ in S.MODES.values():
        assert lib.pf_scan_filter_supported(code, 288, 400, 288, 400, 36, 50) == 1
        assert lib.pf_scan_filter_supported(code, 8, 8, 8, 8, 4000, 4000) == 0
        assert lib.pf_scan_filter_supported(code, 96, 192, 37, 53, 200, 300) == 1
    assert lib.pf_scan_filter_supported(3, 96, 192, 96, 192, 48, 96) == 0 and lib.pf_scan_filter_supported(0, 0, 4, 1, 1, 1, 1) == 0


def test_filter_has_no_cpu_path_and_checks_its_arguments():
    depths, flow, init, _ = make_predictions(COARSE[0], 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.filter_depth_maps(depths, flow, init)
    with pytest.raises(ValueError):
        S.filter_depth_maps(depths, flow, init, mode="AREA")
    with pytest.raises(ValueError):
        S.filter_depth_maps(depths[0], flow, init)
    with pytest.raises(ValueError):
        S.filter_depth_maps(depths, flow[:, :4], init)
    with pytest.raises(ValueError):
        S.filter_depth_maps(depths, flow[:, :, :-1], init)
    with pytest.raises(ValueError):
        S.filter_depth_maps(depths, flow, init[:2])
    with pytest.raises(ValueError):
        S.filter_depth_maps(depths, flow[:2, 0], init)


# ---------------------------------------------------------------------------------------------------------------------
# 2. on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _views(depths, flow, init, cams):
    for v in range(depths.shape[0]):
        yield {"coarse_depth_map": depths[v][None, None, ::4, ::4].contiguous(), "coarse_prob_map": init[v][None, None],
               "flow1_prob": flow[v][None], "flow1": depths[v][None, None]}, \
              {"cam_params_list": cams, "cam_params_list_host": cams, "img_list": torch.zeros(1, 1, 3, H, W)}


@pytest.mark.gpu
@pytest.mark.isolated
def test_nearest_equals_the_file_route_bit_for_bit(dev, tmp_path):
    """eval_file_logger_host -> probability_filter(NEAREST) on files, AsyncEvalWriter(filter_thresholds=...) from the device
    and filter_depth_maps(mode="NEAREST") give the same ``_prob_filtered`` maps, bit for bit."""
    from pointmvsnet_amd import synthetic
    cams = synthetic.make_scene(H, W, 1, 48)["cam_params_list"][:, :1]
    for c, coarse in enumerate(COARSE):
        depths, flow, init, _ = make_predictions(coarse, c)
        init[1, 3, 5] = float("nan")                                        # a NaN confidence keeps the depth
        root = tmp_path / ("case%d" % c)
        # (the writer packs on a real device only: the host emulation of the kernels checks the other two)
        writer = EL.AsyncEvalWriter(filter_thresholds=(INIT_THR, FLOW_THR), write_points=False) if dev.type == "cuda" else None
        for v, (preds, batch) in enumerate(_views(depths, flow, init, cams)):
            path = str(root / "Eval" / "Rectified" / "scan1" / ("rect_%03d_3_r5000.png" % (v + 1)))
            EL.eval_file_logger_host(batch, preds, path, "host")
            if writer is not None:
                writer.submit({k: (t.to(dev) if k == "cam_params_list" else t) for k, t in batch.items()},
                              {k: t.to(dev) for k, t in preds.items()}, path, "device")
        if writer is not None:
            writer.close()
        host = str(root / "Eval" / "host" / "scan1")
        EL.probability_filter(host, INIT_THR, FLOW_THR, "flow1", V3, "NEAREST")
        got, kept = S.filter_depth_maps(depths.to(dev), flow.to(dev), init.to(dev), INIT_THR, FLOW_THR, mode="NEAREST",
                                        return_kept=True)
        assert got.shape == (V3, H, W) and got.dtype == torch.float32 and got.is_contiguous()
        got = got.cpu().numpy()
        for v in range(V3):
            want = IO.load_pfm(os.path.join(host, "%08d_flow1_prob_filtered.pfm" % v))[0]
            assert np.ascontiguousarray(want).tobytes() == got[v].tobytes(), (coarse, v)
            device_file = os.path.join(str(root / "Eval" / "device" / "scan1"), "%08d_flow1_prob_filtered.pfm" % v)
            if writer is not None:
                assert open(device_file, "rb").read() == open(os.path.join(host, "%08d_flow1_prob_filtered.pfm" % v),
                                                              "rb").read()
        share = float((got != 0).mean())
        assert 0.2 < share < 0.95
        assert kept.dtype == torch.int32 and kept.cpu().tolist() == [int((got[v] != 0).sum()) for v in range(V3)]
        # a made confidence of the depth maps' size is the same filter
        made = torch.from_numpy(flow_confidence_of(flow)).to(dev)
        again = S.filter_depth_maps(depths.to(dev), made, init.to(dev), INIT_THR, FLOW_THR, mode="NEAREST")
        assert again.cpu().numpy().tobytes() == got.tobytes()
        report("scan_filter_nearest_%dx%d" % coarse, kept_share=share, mismatches=0)


@pytest.mark.gpu
@pytest.mark.isolated
@pytest.mark.parametrize("mode", MODES[1:])
def test_interpolating_modes_match_the_float64_statement(dev, mode):
    """Bound, band rule and cap: module docstring.  The measured errors go to parity_report.jsonl."""
    for c, coarse in enumerate(COARSE):
        for made in (None, coarse):
            depths, flow, init, flow_made = make_predictions(coarse, 10 + c, made)
            conf = flow_made.numpy() if made else flow_confidence_of(flow)
            keep, band, ri, bi, rf, bf = statement_decision(depths.numpy(), conf, made is not None, init, mode)
            assert band.mean() <= BAND_CAP                                   # on the statement alone
            got, kept, st = S.filter_depth_maps(depths.to(dev), (flow_made if made else flow).to(dev), init.to(dev), INIT_THR,
                                                FLOW_THR, mode=mode, return_kept=True, return_stages=True)
            got, g_init, g_flow = got.cpu().numpy(), st["init_conf"].cpu().numpy(), st["flow_conf"].cpu().numpy()
            err_i = np.abs(g_init.astype(np.float64) - ri)
            err_f = np.abs(g_flow.astype(np.float64) - rf)
            g_keep = got != 0
            flips = int((g_keep != keep)[band].sum())
            name = "scan_filter_%s_%dx%d%s" % (mode.lower(), coarse[0], coarse[1], "_made" if made else "")
            print(name, "init err", err_i.max(), "of bound", (err_i / bi).max(), "flow err", err_f.max(), "band share",
                  band.mean(), "flipped inside the band", flips)
            report(name, init_err_max=err_i.max(), init_err_over_bound_max=(err_i / bi).max(), flow_err_max=err_f.max(),
                   bound_max=bi.max(), band_share=band.mean(), band_flips=flips,
                   mismatches_outside_band=int((g_keep != keep)[~band].sum()))
            assert (err_i <= bi).all()
            if made:
                assert (err_f <= bf).all()
            else:
                assert np.array_equal(g_flow, conf)                          # the rule of eval_file_logger, exactly
            assert np.array_equal(g_keep[~band], keep[~band])
            assert np.array_equal(got[g_keep], depths.numpy()[g_keep])      # kept depths are the depths themselves
            assert kept.cpu().tolist() == [int(g_keep[v].sum()) for v in range(V3)]


@pytest.mark.gpu
@pytest.mark.isolated
def test_maps_of_the_depth_maps_size_pass_through_in_every_mode(dev):
    depths, flow, init, made = make_predictions((H, W), 5, (H, W))
    init[0, 0, 0], made[2, 5, 5] = float("inf"), float("nan")
    want = {}
    for mode in MODES:
        for key, f in (("raw", flow), ("made", made)):
            got, st = S.filter_depth_maps(depths.to(dev), f.to(dev), init.to(dev), INIT_THR, FLOW_THR, mode=mode,
                                          return_stages=True)
            assert st["init_conf"].cpu().numpy().tobytes() == init.numpy().tobytes()
            if key == "made":                                                # the NaN confidence keeps its depth
                assert st["flow_conf"].cpu().numpy().tobytes() == made.numpy().tobytes()
                assert float(got[2, 5, 5]) == float(depths[2, 5, 5]) or float(init[2, 5, 5]) < INIT_THR
            want.setdefault(key, got.cpu().numpy().tobytes())               # NEAREST comes first
            assert got.cpu().numpy().tobytes() == want[key], (mode, key)
    assert want["raw"] != want["made"]


@pytest.mark.gpu
@pytest.mark.isolated
def test_one_launch_equals_view_by_view_and_repeats_identically(dev):
    for mode in MODES:
        depths, flow, init, made = make_predictions(COARSE[2], 20, (41, 77))
        d, f, i, m = depths.to(dev), flow.to(dev), init.to(dev), made.to(dev)
        for fl in (f, m):
            got, kept = S.filter_depth_maps(d, fl, i, mode=mode, return_kept=True)
            again, kept2 = S.filter_depth_maps(d, fl, i, mode=mode, return_kept=True)
            assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes() and torch.equal(kept.cpu(), kept2.cpu())
            for v in range(V3):
                one, k1 = S.filter_depth_maps(d[v:v + 1], fl[v:v + 1], i[v:v + 1], mode=mode, return_kept=True)
                assert one.cpu().numpy().tobytes() == got[v].cpu().numpy().tobytes(), (mode, v)
                assert int(k1[0]) == int(kept[v])
    # sizes that are no multiple of the tile, one view, a single row; an empty scan
    g = torch.Generator().manual_seed(1)
    for h, w, ih, iw in ((5, 7, 3, 2), (1, 70, 1, 9), (33, 31, 33, 8), (9, 65, 4, 65)):
        d = 1.0 + torch.rand(1, h, w, generator=g)
        f = torch.rand(1, h, w, generator=g)
        i = torch.rand(1, ih, iw, generator=g)
        for mode in MODES:
            got, st = S.filter_depth_maps(d.to(dev), f.to(dev), i.to(dev), INIT_THR, FLOW_THR, mode=mode, return_stages=True)
            ri, bi = bound_of(i[0].numpy(), h, w, mode)
            assert (np.abs(st["init_conf"][0].cpu().numpy() - ri) <= bi).all(), (mode, h, w)
            keep = ~(f[0].numpy() < FLOW_THR) & ~(st["init_conf"][0].cpu().numpy() < INIT_THR)
            assert np.array_equal(got[0].cpu().numpy(), np.where(keep, d[0].numpy(), 0.0).astype(np.float32))
    empty = S.filter_depth_maps(torch.zeros(0, 4, 4).to(dev), torch.zeros(0, 5, 4, 4).to(dev), torch.zeros(0, 2, 2).to(dev))
    assert empty.shape == (0, 4, 4)
    with pytest.raises(ValueError):                                          # outside pf_scan_filter_supported
        S.filter_depth_maps(torch.ones(1, 8, 8).to(dev), torch.ones(1, 8, 8).to(dev), torch.ones(1, 4000, 4000).to(dev))
