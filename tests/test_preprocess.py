"""DTU scene input: pointmvsnet_amd/utils/preprocess.py, pointmvsnet_amd/dataset.py and csrc/preprocess.hip.

What is pinned to what
----------------------
* scale 1 (no resize): the reference's own NumPy chain, tests/golden/preprocess.npz (make_preprocess_golden.py).  The host
  path equals it bit for bit.  The kernels standardise from exact integer sums in float64, the reference in float32 NumPy,
  so the GPU is held to the float64 statement (``statement_standardise``: Python integers -> one float64 expression) within
  ONE float32 ulp -- the statement rounded once to float32 is within half an ulp; the other half allows a reciprocal
  instead of a quotient -- and therefore to ``|gpu - golden| <= |golden - statement| + 1 ulp`` pointwise.
* scale != 1: the resize is the project's own specification (OpenCV's fixed-point kernel is not restated and OpenCV is
  not installed here); the yardstick is ``utils.preprocess.blend_tables``, the float64 blend with the float32 tables.  The
  kernel evaluates the same expression in float32: six roundings ((1-wx), two products and a sum per row pair, ...) of
  magnitudes <= 255, so its value is within 6 x 2^-24 x 255 of the statement's; ``TIE`` is 4 x that (3.6e-4).  The uint8
  images must be EQUAL except at ties -- statement values within TIE of k + 0.5 -- where they may differ by one level.
  Where both weights of a pixel are multiples of 2^-8 every product and sum is exact in float32 too and both sides round
  half-to-even alike: such pixels are never ties.  That covers EVERY pixel at 0.8 (weights n/8, 1.6 % exact halves) and
  at 512/1200 (the step 75/32 gives weights n/64, 0.03 % exact halves): there the images must be equal throughout.  Ties
  are capped at 1 % of the values; measured with the statement alone on the seeded images below: 0 % at both scales on
  1200 x 1600 and on 151 x 203 (test_statement_tie_share_stays_under_the_cap keeps that asserted), 0.076 % at the scale
  1.37 of test_gpu_shapes_views_and_repeatability, whose weights are not dyadic.
  ``img_list`` is then checked as at scale 1 against the statement evaluated on the kernel's own uint8 image.
"""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, report
from pointmvsnet_amd import synthetic
from pointmvsnet_amd.utils import io as IO
from pointmvsnet_amd.utils import preprocess as P

TIE = 4 * 6 * 2.0 ** -24 * 255
TIE_CAP = 0.01
CASES = ("a", "b", "c")
SCALES = (0.8, 512.0 / 1200.0)

PAIR_TXT = """3
0
10 10 2346.41 1 2036.53 9 1243.89 12 1052.87 11 1000.84 13 703.583 2 604.456 8 439.759 14 327.419 27 249.278
1
10 9 2850.87 10 2583.94 2 2105.59 0 2052.84 8 1868.24 13 1184.23 14 1017.51 12 961.966 7 670.208 15 657.218
2
10 8 2501.24 1 2106.88 7 2015.46 9 1807.74 3 1605.71 15 1157.57 14 969.3 16 848.6 10 806.1 13 694.3
"""


# ---------------------------------------------------------------------------------------------------------------------
# statements
# ---------------------------------------------------------------------------------------------------------------------
def statement_standardise(ref_u8):
    """(V, h, w, 3) uint8 -> (V, 3, h, w) float64: mean and population variance from exact integers, one expression."""
    ref = np.asarray(ref_u8).astype(np.int64)
    V, h, w, _ = ref.shape
    n = h * w
    out = np.empty((V, 3, h, w))
    for v in range(V):
        for c in range(3):
            s1, s2 = int(ref[v, :, :, c].sum()), int((ref[v, :, :, c] ** 2).sum())
            mean, var = s1 / n, (n * s2 - s1 * s1) / (n * n)
            out[v, c] = (ref[v, :, :, c] - mean) / (np.sqrt(var) + 1e-7)
    return out


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def statement_resize_crop(views, scale, height, width, base):
    """Per view the float64 blend values and their uint8 rounding, the tie mask, the crop offsets."""
    (yi, yw, xi, xw), offsets, _, _ = P._tables(views.shape[1], views.shape[2], float(scale), height, width, base)
    exact = ((yw.astype(np.float64) * 256) % 1 == 0)[:, None, None] & ((xw.astype(np.float64) * 256) % 1 == 0)[None, :, None]
    vals, imgs, ties = [], [], []
    for v in views:
        val, q = P.blend_tables(v, yi, yw, xi, xw)
        near = np.abs(val - np.floor(val) - 0.5) <= TIE
        vals.append(val)
        imgs.append(q)
        ties.append(near & ~exact)
    return np.stack(vals), np.stack(imgs), np.stack(ties), offsets


def seeded_views(V, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (V, h, w, 3), dtype=np.uint8)


def check_against_statement(views, scale, height, width, base, dev, tag):
    """The whole GPU comparison of one configuration; returns the GPU results."""
    _, q, ties, offsets = statement_resize_crop(views, scale, height, width, base)
    img_list, ref_img, got_offsets = P.preprocess_views(torch.from_numpy(views).to(dev), scale, height, width, base)
    assert got_offsets == offsets
    assert img_list.dtype == torch.float32 and tuple(img_list.shape) == (q.shape[0], 3) + q.shape[1:3]
    assert ref_img.dtype == torch.uint8 and tuple(ref_img.shape) == q.shape
    got_u8 = ref_img.cpu().numpy()
    diff = got_u8.astype(np.int64) - q.astype(np.int64)
    tie_share = float(ties.mean())
    print("%s: ties %.4f %% of the values, %d values differ, largest difference %d"
          % (tag, 100 * tie_share, int((diff != 0).sum()), int(np.abs(diff).max())))
    assert tie_share <= TIE_CAP
    assert not (diff != 0)[~ties].any(), "uint8 image differs from the statement away from a tie"
    assert np.abs(diff).max() <= 1
    st = statement_standardise(got_u8)
    err = np.abs(img_list.cpu().numpy().astype(np.float64) - st) / ulp32(st)
    print("%s: img_list within %.3f ulp of the float64 statement" % (tag, float(err.max())))
    report("preprocess_" + tag, tie_share=tie_share, differing=float((diff != 0).sum()), img_list_ulp=float(err.max()))
    assert err.max() <= 1.0
    return img_list, ref_img


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_host_path_equals_the_reference_at_scale_1(case):
    g = {k: v.numpy() for k, v in load_golden("preprocess").items()}
    height, width, base = (int(a) for a in g["case_%s_args" % case])
    img_list, ref_img, (sy, sx) = P.preprocess_views(g["images"], 1, height, width, base)
    assert img_list.dtype == torch.float32 and ref_img.dtype == torch.uint8
    assert np.array_equal(ref_img.numpy(), g["case_%s_crop" % case])
    assert np.array_equal(img_list.numpy(), g["case_%s_norm" % case].transpose(0, 3, 1, 2))
    # a list of views and no crop at all (the training split) go the same way
    whole, _, off = P.preprocess_views([v for v in g["images"]])
    assert off == (0, 0) and np.array_equal(whole[1].numpy(), P.norm_image(g["images"][1]).transpose(2, 0, 1))
    cams = np.stack([P.crop_camera(P.scale_camera(c, 1), sy, sx) for c in g["cams"]])
    assert cams.dtype == np.float64 and np.array_equal(cams, g["case_%s_cams" % case])
    assert (sy, sx) == {"a": (4, 2), "b": (0, 2), "c": (4, 2)}[case]


def test_camera_arithmetic_equals_the_reference():
    g = {k: v.numpy() for k, v in load_golden("preprocess").items()}
    scaled = np.stack([P.scale_camera(c, 0.8) for c in g["cams"]])
    assert np.array_equal(scaled, g["scaled_cams_0p8"])
    assert not np.array_equal(scaled, g["cams"]) and np.array_equal(P.scale_camera(g["cams"][0]), g["cams"][0])
    assert P.crop_window(72, 64, 32) == (4, 64) and P.crop_window(100, 128, 24) == (2, 96)
    assert P.crop_window(72, 72, 16) == (4, 64) and P.crop_window(75, None, 16) == (0, 75)


def test_resize_tables_follow_the_specification():
    idx, wgt = P.resize_tables(10, 0.5)                     # (d + 0.5) * 2 - 0.5 = 0.5, 2.5, ..., 8.5
    assert idx.dtype == np.int32 and wgt.dtype == np.float32
    assert idx.tolist() == [0, 2, 4, 6, 8] and wgt.tolist() == [0.5] * 5
    idx, wgt = P.resize_tables(4, 2.0)                      # -0.25, 0.25, 0.75, ..., 3.25, 3.75: both ends clamp
    assert idx.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and wgt.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.0]
    assert P.scaled_size(5, 0.5) == 2 and P.scaled_size(7, 0.5) == 4 and P.scaled_size(1200, 512 / 1200) == 512
    img = np.arange(4 * 6 * 3, dtype=np.uint8).reshape(4, 6, 3)
    assert np.array_equal(P.resize_linear(img, 1), img)
    half = P.resize_linear(img, 0.5)                        # the mean of each 2 x 2 block; .5 values round to even
    blocks = img.astype(np.float64).reshape(2, 2, 3, 2, 3).mean(axis=(1, 3))
    assert np.array_equal(half, np.rint(blocks).astype(np.uint8))


def test_path_lists_for_all_splits(tmp_path):
    from pointmvsnet_amd.dataset import DTUDataset
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "Cameras"))
    with open(os.path.join(root, "Cameras", "pair.txt"), "w") as f:
        f.write(PAIR_TXT)
    train = DTUDataset(root, "train", num_view=3)
    assert len(train) == 79 * 7 * 3
    assert train.path_list[0] == {
        "view_image_paths": [root + "/Rectified/scan2_train/rect_001_0_r5000.png",
                             root + "/Rectified/scan2_train/rect_011_0_r5000.png",
                             root + "/Rectified/scan2_train/rect_002_0_r5000.png"],
        "view_cam_paths": [root + "/Cameras/train/00000000_cam.txt", root + "/Cameras/train/00000010_cam.txt",
                           root + "/Cameras/train/00000001_cam.txt"],
        "view_depth_paths": [root + "/Depths/scan2_train/depth_map_0000.pfm", root + "/Depths/scan2_train/depth_map_0010.pfm",
                             root + "/Depths/scan2_train/depth_map_0001.pfm"]}
    # entry 1 under lighting 1 of the first scan, the last entry of the last scan
    assert train.path_list[4]["view_image_paths"] == [root + "/Rectified/scan2_train/rect_002_1_r5000.png",
                                                      root + "/Rectified/scan2_train/rect_010_1_r5000.png",
                                                      root + "/Rectified/scan2_train/rect_011_1_r5000.png"]
    assert train.path_list[-1]["view_depth_paths"] == [root + "/Depths/scan128_train/depth_map_0002.pfm",
                                                       root + "/Depths/scan128_train/depth_map_0008.pfm",
                                                       root + "/Depths/scan128_train/depth_map_0001.pfm"]
    valid = DTUDataset(root, "valid", num_view=5)
    assert len(valid) == 18 * 1 * 3
    assert valid.path_list[2]["view_image_paths"] == [root + "/Rectified/scan3_train/rect_%03d_3_r5000.png" % i
                                                      for i in (3, 9, 2, 8, 10)]
    assert valid.path_list[2]["view_cam_paths"] == [root + "/Cameras/train/%08d_cam.txt" % i for i in (2, 8, 1, 7, 9)]
    test = DTUDataset(root, "test", num_view=3, depth_folder="/depths")
    assert len(test) == 22 * 1 * 3
    assert test.path_list[1] == {
        "view_image_paths": [root + "/Eval/Rectified/scan1/rect_%03d_3_r5000.png" % i for i in (2, 10, 11)],
        "view_cam_paths": [root + "/Cameras/%08d_cam.txt" % i for i in (1, 9, 10)],
        "view_depth_paths": ["/depths/scan1/depth_map_%04d.pfm" % i for i in (1, 9, 10)]}
    assert test.path_list[-1]["view_image_paths"][0] == root + "/Eval/Rectified/scan118/rect_003_3_r5000.png"
    with pytest.raises(ValueError):
        DTUDataset(root, "val")


def test_mask_depth_image_at_the_bounds():
    lo, hi = np.float32(427.5), np.float32(440.0)
    below = lambda x: np.nextafter(x, np.float32(0))
    above = lambda x: np.nextafter(x, np.float32(1e6))
    d = np.array([[lo, below(lo), above(lo)], [hi, below(hi), above(hi)]], dtype=np.float32)
    out = P.mask_depth_image(d, float(lo), float(hi))
    assert out.shape == (2, 3, 1) and out.dtype == np.float32
    assert np.array_equal(out[:, :, 0], np.array([[0, 0, above(lo)], [hi, below(hi), 0]], dtype=np.float32))


def _write_png(path, bgr):
    try:
        import cv2
        cv2.imwrite(path, bgr)
    except ImportError:
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(path)


def _need_decoder():
    try:
        import cv2  # noqa: F401
    except ImportError:
        try:
            import PIL  # noqa: F401
        except ImportError:
            pytest.skip("neither OpenCV nor Pillow is installed")


def make_dtu_folder(root, split, scan, h, w, depth_hw=None, depths=None, cams=None, seed=0):
    """A DTU-layout folder with the views 0, 1, 2, 8, 9, 10 of one scan under lighting 3; returns the BGR images by view."""
    rng = np.random.default_rng(seed)
    train = split != "test"
    img_dir = os.path.join(root, "Rectified/scan%d_train" % scan if train else "Eval/Rectified/scan%d" % scan)
    cam_dir = os.path.join(root, "Cameras/train" if train else "Cameras")
    depth_dir = os.path.join(root, "Depths/scan%d_train" % scan if train else "depths/scan%d" % scan)
    for d in (img_dir, cam_dir, depth_dir):
        os.makedirs(d, exist_ok=True)
    with open(os.path.join(root, "Cameras", "pair.txt"), "w") as f:
        f.write(PAIR_TXT)
    images = {}
    for k, view in enumerate((0, 1, 2, 8, 9, 10)):
        images[view] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        _write_png(os.path.join(img_dir, "rect_%03d_3_r5000.png" % (view + 1)), images[view])
        cam = np.zeros((2, 4, 4))
        cam[0] = np.eye(4)
        cam[0, :3, 3] = (10.0 * view, -3.0, 1.0)
        cam[1, :3, :3] = [[300.0 + view, 0.0, 31.25], [0.0, 299.0, 20.5], [0.0, 0.0, 1.0]]
        cam[1, 3] = (425.0, 2.5, 8.0, 442.5)
        if cams is not None:
            cam = cams[k % len(cams)]
        IO.write_cam_dtu(os.path.join(cam_dir, "%08d_cam.txt" % view), cam)
        if depth_hw is not None:
            dm = depths if depths is not None else (425.0 + 17.0 * rng.random(depth_hw)).astype(np.float32)
            IO.write_pfm(os.path.join(depth_dir, "depth_map_%04d.pfm" % view), dm)
    return images


def test_getitem_test_split(tmp_path):
    _need_decoder()
    from pointmvsnet_amd.dataset import DTUDataset
    root = str(tmp_path)
    images = make_dtu_folder(root, "test", 1, 40, 64, depth_hw=(40, 64))
    ds = DTUDataset(root, "test", num_view=3, height=32, width=48, num_virtual_plane=8, interval_scale=1.0,
                    base_image_size=16, depth_folder=os.path.join(root, "depths"))
    item = ds[1]                                            # entry 1: views 1, 9, 10
    assert set(item) == {"img_list", "cam_params_list", "gt_depth_img", "depth_list", "ref_img_path", "ref_img", "mean", "std"}
    views = np.stack([images[v] for v in (1, 9, 10)])       # BGR, as cv2.imread gives them
    # scale = max(32/40, 48/64) = 0.8 -> 32 x 51, cropped to 32 x 48 from column 1
    want_img, want_ref, offsets = P.preprocess_views(views, 0.8, 32, 48, 16)
    assert offsets == (0, 1)
    assert item["img_list"].dtype == torch.float32 and tuple(item["img_list"].shape) == (3, 3, 32, 48)
    assert torch.equal(item["img_list"], want_img)
    assert isinstance(item["ref_img"], np.ndarray) and item["ref_img"].dtype == np.uint8
    assert np.array_equal(item["ref_img"], want_ref[0].numpy()) and item["ref_img"].shape == (32, 48, 3)
    cams = item["cam_params_list"]
    assert cams.dtype == torch.float32 and tuple(cams.shape) == (3, 2, 4, 4)
    assert cams[0, 1, 0, 0] == np.float32(301.0 * 0.8) and cams[0, 1, 1, 1] == np.float32(299.0 * 0.8)
    assert cams[0, 1, 0, 2] == np.float32(31.25 * 0.8 - 1) and cams[0, 1, 1, 2] == np.float32(20.5 * 0.8 - 0)
    assert cams[2, 0, 0, 3] == 100.0 and cams[0, 1, 3].tolist() == [425.0, 2.5, 8.0, 442.5]
    assert tuple(item["depth_list"].shape) == (3, 1, 40, 64) and item["depth_list"].dtype == torch.float32
    depth = IO.load_pfm(ds.path_list[1]["view_depth_paths"][0])[0]
    rows = np.minimum(np.floor(np.arange(32) * (40 / 32.0)).astype(int), 39)
    cols = np.minimum(np.floor(np.arange(51) * (64 / 51.0)).astype(int), 63)
    assert np.array_equal(item["gt_depth_img"], depth[rows][:, cols][:, 1:49])
    assert item["ref_img_path"].endswith("Eval/Rectified/scan1/rect_002_3_r5000.png")
    assert torch.equal(item["mean"], ds.mean) and item["std"].shape == (3,)
    # without a depth folder: zeros of the target size
    blank = DTUDataset(root, "test", num_view=2, height=32, width=48, num_virtual_plane=8, base_image_size=16)[0]
    assert tuple(blank["depth_list"].shape) == (2, 1, 32, 48) and not blank["depth_list"].any()
    assert tuple(blank["img_list"].shape) == (2, 3, 32, 48)
    with pytest.raises(ValueError):
        DTUDataset(root, "test", num_view=3, height=64, width=48, base_image_size=16)[0]


def test_getitem_train_split_and_depth_range_masks(tmp_path):
    _need_decoder()
    from pointmvsnet_amd.dataset import DTUDataset
    root = str(tmp_path)
    # start = 425 + 2.5 = 427.5, end = 425 + (8 - 2) * 2.5 = 440: both exact in float32
    lo, hi = np.float32(427.5), np.float32(440.0)
    below = lambda x: np.nextafter(x, np.float32(0))
    above = lambda x: np.nextafter(x, np.float32(1e6))
    depths = np.array([[lo, below(lo), above(lo), 430.0], [hi, below(hi), above(hi), 0.0]], dtype=np.float32)
    images = make_dtu_folder(root, "train", 2, 24, 36, depth_hw=(2, 4), depths=depths)
    ds = DTUDataset(root, "train", num_view=3, num_virtual_plane=8, interval_scale=1.0, scans=[2], lightings=[3])
    assert len(ds) == 3
    item = ds[2]                                            # entry 2: views 2, 8, 1
    assert set(item) == {"img_list", "cam_params_list", "gt_depth_img", "depth_list", "ref_img_path", "mean", "std"}
    assert item["img_list"].dtype == torch.float32 and tuple(item["img_list"].shape) == (3, 3, 24, 36)
    for k, view in enumerate((2, 8, 1)):                    # BGR order, the reference's float32 standardisation
        assert np.array_equal(item["img_list"][k].numpy(), P.norm_image(images[view]).transpose(2, 0, 1))
    assert tuple(item["cam_params_list"].shape) == (3, 2, 4, 4) and item["cam_params_list"][1, 1, 0, 0] == 308.0
    gt = item["gt_depth_img"]
    assert gt.dtype == torch.float32 and tuple(gt.shape) == (1, 2, 4)
    assert np.array_equal(gt[0].numpy(), np.array([[0, 0, above(lo), 430.0], [hi, below(hi), 0, 0]], dtype=np.float32))
    dl = item["depth_list"]
    assert dl.dtype == torch.float32 and tuple(dl.shape) == (3, 1, 2, 4)
    for k in range(3):
        assert np.array_equal(dl[k, 0].numpy(), np.array([[0, 0, above(lo), 430.0], [0, below(hi), 0, 0]], dtype=np.float32))


def test_statement_tie_share_stays_under_the_cap():
    """The share of values the GPU comparison lets differ by one level, measured with the float64 statement alone."""
    for tag, views, crops in (("1200x1600", seeded_views(1, 1200, 1600, 11), ((960, 1280, 64), (512, 640, 64))),
                              ("151x203", seeded_views(2, 151, 203, 12), ((None, None, 64), (None, None, 64)))):
        for scale, (height, width, base) in zip(SCALES, crops):
            val, q, ties, _ = statement_resize_crop(views, scale, height, width, base)
            halves = float((val - np.floor(val) == 0.5).mean())
            print("%s scale %.4f -> %s: ties %.4f %%, exact halves %.4f %%" % (tag, scale, q.shape[1:3], 100 * ties.mean(),
                                                                               100 * halves))
            assert ties.mean() <= TIE_CAP


def test_preprocess_rejects_what_it_cannot_do():
    with pytest.raises(ValueError):
        P.preprocess_views([np.zeros((4, 4, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)])
    with pytest.raises(ValueError):
        P.preprocess_views(np.zeros((1, 4, 4, 3), np.float32))
    with pytest.raises(RuntimeError):
        P.preprocess_views_gpu(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))       # no CPU route behind the kernels


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_gpu_scale_1_against_the_reference_golden(dev, case):
    g = {k: v.numpy() for k, v in load_golden("preprocess").items()}
    height, width, base = (int(a) for a in g["case_%s_args" % case])
    img_list, ref_img, offsets = P.preprocess_views(g["images"], 1, height, width, base, device=dev)
    assert img_list.device.type == dev.type and ref_img.device.type == dev.type
    assert np.array_equal(ref_img.cpu().numpy(), g["case_%s_crop" % case])
    assert offsets == P.preprocess_views(g["images"], 1, height, width, base)[2]
    got = img_list.cpu().numpy().astype(np.float64)
    golden = g["case_%s_norm" % case].transpose(0, 3, 1, 2).astype(np.float64)
    st = statement_standardise(g["case_%s_crop" % case])
    ulp = ulp32(st)
    err = np.abs(got - st) / ulp
    to_golden = np.abs(got - golden)
    print("case %s: |gpu - statement| <= %.3f ulp, |gpu - golden| <= %.3e, |golden - statement| <= %.3e"
          % (case, err.max(), to_golden.max(), np.abs(golden - st).max()))
    report("preprocess_scale1_" + case, gpu_vs_golden_max=to_golden.max(), gpu_vs_statement_ulp=err.max(),
           golden_vs_statement_max=np.abs(golden - st).max())
    assert err.max() <= 1.0
    assert (to_golden <= np.abs(golden - st) + ulp).all()


@pytest.mark.gpu
@pytest.mark.parametrize("size,seed,crops", [((1200, 1600), 11, ((960, 1280, 64), (512, 640, 64))),
                                             ((151, 203), 12, ((None, None, 64), (None, None, 64)))])
@pytest.mark.parametrize("which", [0, 1])
def test_gpu_resize_against_the_float64_statement(dev, size, seed, crops, which):
    views = seeded_views(1 if size[0] > 1000 else 2, size[0], size[1], seed)
    height, width, base = crops[which]
    check_against_statement(views, SCALES[which], height, width, base, dev, "%dx%d_s%d" % (size[0], size[1], which))


@pytest.mark.gpu
@pytest.mark.parametrize("V,h,w,scale,height,width,base", [
    (1, 151, 203, 0.8, None, None, 64),          # 121 x 162: a width that is not a multiple of 4, h * w odd
    (3, 151, 203, 0.8, 117, 159, 1),             # odd crop offsets (2, 1), odd sizes
    (7, 90, 132, 1, 77, 101, 1),                 # scale 1 with odd offsets (6, 15) and an odd width
    (3, 100, 300, 512.0 / 1200.0, 32, 64, 32),   # 43 x 128 -> 32 x 64 from (5, 32)
    (7, 64, 600, 1, 64, 576, 64),                # three column tiles, offsets (0, 12)
    (1, 70, 90, 1.37, None, None, 1),            # enlarging: both ends of the tables clamp; weights that are not dyadic
])
def test_gpu_shapes_views_and_repeatability(dev, V, h, w, scale, height, width, base):
    views = seeded_views(V, h, w, 100 + V)
    tag = "V%d_%dx%d_%s" % (V, h, w, ("%.3f" % scale).replace(".", "p"))
    img_a, ref_a = check_against_statement(views, scale, height, width, base, dev, tag)
    img_b, ref_b, _ = P.preprocess_views(views, scale, height, width, base, device=dev)
    assert torch.equal(ref_a, ref_b)
    assert torch.equal(img_a.view(torch.int32), img_b.view(torch.int32)), "two runs differ in their bits"
    # every view is standardised on its own: view 0 alone gives view 0 of the batch
    img_0, _, _ = P.preprocess_views(views[:1], scale, height, width, base, device=dev)
    assert torch.equal(img_0[0].view(torch.int32), img_a[0].view(torch.int32))


@pytest.mark.gpu
def test_gpu_dataset_item_feeds_the_model(dev, tmp_path):
    _need_decoder()
    from pointmvsnet_amd.dataset import DTUDataset
    from pointmvsnet_amd.model import PointMVSNet
    root = str(tmp_path)
    data, img_scales, inter_scales = synthetic.make_config("tiny")          # 3 views of 128 x 192, 8 planes
    cams = data["cam_params_list"][0].double().numpy().copy()
    cams[:, 1, :2, :3] /= 0.8                                                 # intrinsics of the 160 x 240 sources
    images = make_dtu_folder(root, "test", 1, 160, 240, cams=list(cams))
    kw = dict(num_view=3, height=128, width=192, num_virtual_plane=8, interval_scale=1.0, base_image_size=64)
    item = DTUDataset(root, "test", device=dev, **kw)[0]                      # entry 0: views 0, 10, 1
    views = np.stack([images[v] for v in (0, 10, 1)])
    want_img, want_ref, _ = P.preprocess_views(torch.from_numpy(views).to(dev), 0.8, 128, 192, 64)
    assert item["img_list"].device.type == dev.type and tuple(item["img_list"].shape) == (3, 3, 128, 192)
    assert torch.equal(item["img_list"].view(torch.int32), want_img.view(torch.int32))
    assert item["ref_img"].dtype == torch.uint8 and torch.equal(item["ref_img"], want_ref[0])
    host = DTUDataset(root, "test", **kw)[0]
    assert torch.equal(host["cam_params_list"], item["cam_params_list"])
    assert np.abs(host["ref_img"].astype(int) - item["ref_img"].cpu().numpy().astype(int)).max() <= 1
    batch = {"img_list": item["img_list"][None], "cam_params_list": item["cam_params_list"][None].to(dev),
             "mean": item["mean"][None].to(dev), "std": item["std"][None].to(dev)}
    net = PointMVSNet()
    synthetic.seed_weights(net, seed=0)
    net = net.to(dev).train()
    with torch.no_grad():
        preds = net(batch, img_scales, inter_scales, isFlow=True, isTest=True)
    assert tuple(preds["coarse_depth_map"].shape) == (1, 1, 16, 24)
    assert tuple(preds["flow2"].shape) == (1, 1, 32, 48) and bool(torch.isfinite(preds["flow2"]).all())
