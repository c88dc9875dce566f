"""The DTU scenes as a ``torch.utils.data.Dataset``: a folder -> the ``data_batch`` entries ``PointMVSNet.forward`` takes.

One class for the three splits of reference dataset.py (its ``DTU_Train_Val_Set`` and ``DTU_Test_Set`` differ in folders
and in the preprocessing only): the same folder layout, file-name patterns, ``Cameras/pair.txt`` indexing, scan and
lighting lists, ``mean`` / ``std`` constants and keys of the returned dict.

============  =====================================  ================================  ==========================
split         images                                 cameras                           depth maps
============  =====================================  ================================  ==========================
train, valid  Rectified/scan<N>_train/rect_*.png     Cameras/train/<view>_cam.txt      Depths/scan<N>_train/*.pfm
test          Eval/Rectified/scan<N>/rect_*.png      Cameras/<view>_cam.txt            <depth_folder>/scan<N>/*.pfm
============  =====================================  ================================  ==========================

``pair.txt`` is read as whitespace-separated words: word 0 is the number of entries; entry ``p`` has its reference view
at word ``22 p + 1`` and its ``v``-th partner at word ``22 p + 2 v + 3`` (10 partners with their scores per entry).

train / valid: the images are standardised only; ``gt_depth_img`` is the reference view's depth kept where
``start < d <= end`` and ``depth_list`` every view's depth kept where ``start < d < end``, with ``start = depth_min +
interval`` and ``end = depth_min + (num_virtual_plane - 2) * interval``.

test: the images are resized by ``max(height / h, width / w)`` (a target larger than the source is a ``ValueError``),
centre-cropped and standardised (utils/preprocess.py states how); the cameras are scaled and then shifted by the crop
offsets in float64; the reference view's depth map is nearest-resized and cropped alike; ``ref_img`` is the reference
view's resized and cropped uint8 image.

``device``: None (default) preprocesses on the host with NumPy and returns CPU tensors.  With a GPU device the item's
decoded uint8 images are uploaded (3 bytes per pixel instead of 12) and csrc/preprocess.hip resizes, crops and
standardises them there: ``img_list`` and ``ref_img`` are then tensors on that device.  The kernels are launched from
``__getitem__``, so use such a dataset with ``DataLoader(..., num_workers=0)`` (worker processes must not touch the GPU).
"""
import os.path as osp

import numpy as np
import torch
from torch.utils.data import Dataset

from .utils import io
from .utils.eval_file_logger import _resize_nearest
from .utils.preprocess import crop_camera, crop_window, mask_depth_image, preprocess_views, scale_camera, scaled_size

TRAINING_SET = [2, 6, 7, 8, 14, 16, 18, 19, 20, 22, 30, 31, 36, 39, 41, 42, 44, 45, 46, 47, 50, 51, 52, 53, 55, 57, 58, 60,
                61, 63, 64, 65, 68, 69, 70, 71, 72, 74, 76, 83, 84, 85, 87, 88, 89, 90, 91, 92, 93, 94, 95, 96, 97, 98, 99,
                100, 101, 102, 103, 104, 105, 107, 108, 109, 111, 112, 113, 115, 116, 119, 120, 121, 122, 123, 124, 125,
                126, 127, 128]
VALIDATION_SET = [3, 5, 17, 21, 28, 35, 37, 38, 40, 43, 56, 59, 66, 67, 82, 86, 106, 117]
TEST_SET = [1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118]
SPLITS = {                 # split -> (scans, lightings)
    "train": (TRAINING_SET, [0, 1, 2, 3, 4, 5, 6]),
    "valid": (VALIDATION_SET, [3]),
    "test": (TEST_SET, [3]),
}
PAIR_WORDS = 22            # words per entry of pair.txt: the view, the partner count, 10 x (partner, score)


def imread_bgr(path):
    """The image file as (h, w, 3) uint8 in BGR order, what ``cv2.imread`` returns: OpenCV if importable, else Pillow."""
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        img = cv2.imread(path)
        if img is None:
            raise IOError("cannot read image %s" % path)
        return img
    try:
        from PIL import Image
    except ImportError:
        raise ImportError("pointmvsnet_amd.dataset needs an image decoder: install OpenCV (cv2) or Pillow (PIL)")
    with Image.open(path) as f:
        return np.ascontiguousarray(np.asarray(f.convert("RGB"))[:, :, ::-1])


class DTUDataset(Dataset):
    mean = torch.tensor([1.97145182, -1.52387525, 651.07223895])
    std = torch.tensor([84.45612252, 93.22252387, 80.08551226])
    cluster_file_path = "Cameras/pair.txt"

    def __init__(self, root_dir, split, num_view=3, height=1152, width=1600, num_virtual_plane=128, interval_scale=1.6,
                 base_image_size=64, depth_folder="", device=None, scans=None, lightings=None):
        if split not in SPLITS:
            raise ValueError("Unknown split: {} (one of train, valid, test)".format(split))
        self.root_dir = root_dir
        self.split = split
        self.num_view = num_view
        self.height = height
        self.width = width
        self.num_virtual_plane = num_virtual_plane
        self.interval_scale = interval_scale
        self.base_image_size = base_image_size
        self.depth_folder = depth_folder
        self.device = None if device is None else torch.device(device)
        with open(osp.join(root_dir, self.cluster_file_path)) as f:
            self.cluster_list = f.read().split()
        self.data_set = list(SPLITS[split][0] if scans is None else scans)
        self.lighting_set = list(SPLITS[split][1] if lightings is None else lightings)
        self.path_list = self._load_dataset(self.data_set, self.lighting_set)

    def _folders(self, scan):
        if self.split == "test":
            return (osp.join(self.root_dir, "Eval/Rectified/scan{}".format(scan)), osp.join(self.root_dir, "Cameras"),
                    osp.join(self.depth_folder, "scan{}".format(scan)))
        return (osp.join(self.root_dir, "Rectified/scan{}_train".format(scan)), osp.join(self.root_dir, "Cameras/train"),
                osp.join(self.root_dir, "Depths/scan{}_train".format(scan)))

    def _load_dataset(self, dataset, lighting_set):
        words = self.cluster_list
        path_list = []
        for scan in dataset:
            image_folder, cam_folder, depth_folder = self._folders(scan)
            for lighting in lighting_set:
                for p in range(int(words[0])):
                    views = [int(words[PAIR_WORDS * p + 1])]
                    views += [int(words[PAIR_WORDS * p + 2 * v + 3]) for v in range(self.num_view - 1)]
                    path_list.append({
                        "view_image_paths": [osp.join(image_folder, "rect_{:03d}_{}_r5000.png".format(i + 1, lighting))
                                             for i in views],
                        "view_cam_paths": [osp.join(cam_folder, "{:08d}_cam.txt".format(i)) for i in views],
                        "view_depth_paths": [osp.join(depth_folder, "depth_map_{:04d}.pfm".format(i)) for i in views],
                    })
        return path_list

    def __len__(self):
        return len(self.path_list)

    def _load_views(self, paths):
        images = [imread_bgr(p) for p in paths["view_image_paths"]]
        cams = []
        for p in paths["view_cam_paths"]:
            with open(p) as f:
                cams.append(io.load_cam_dtu(f, num_depth=self.num_virtual_plane, interval_scale=self.interval_scale))
        return images, cams

    def __getitem__(self, index):
        paths = self.path_list[index]
        images, cams = self._load_views(paths)
        item = self._test_item(paths, images, cams) if self.split == "test" else self._train_item(paths, images, cams)
        item.update(ref_img_path=paths["view_image_paths"][0], mean=self.mean, std=self.std)
        return item

    def _train_item(self, paths, images, cams):
        depth_images = [io.load_pfm(p)[0] for p in paths["view_depth_paths"]]
        # out-of-range depths -> 0, in a range relaxed by one interval at either end
        depth_start = cams[0][1, 3, 0] + cams[0][1, 3, 1]
        depth_end = cams[0][1, 3, 0] + (self.num_virtual_plane - 2) * cams[0][1, 3, 1]
        ref_depth = mask_depth_image(depth_images[0], depth_start, depth_end)
        img_list, _, _ = preprocess_views(images, device=self.device)
        depth_list = torch.tensor(np.stack(depth_images, axis=0)).unsqueeze(1).float()
        depth_list = depth_list * (depth_list > depth_start).float() * (depth_list < depth_end).float()
        return {
            "img_list": img_list,
            "cam_params_list": torch.tensor(np.stack(cams, axis=0)).float(),
            "gt_depth_img": torch.tensor(np.ascontiguousarray(ref_depth)).permute(2, 0, 1).float(),
            "depth_list": depth_list,
        }

    def _test_item(self, paths, images, cams):
        if self.depth_folder:
            depth_images = [io.load_pfm(p)[0] for p in paths["view_depth_paths"]]
        else:
            depth_images = [np.zeros((self.height, self.width), np.float64) for _ in paths["view_depth_paths"]]
        h, w = images[0].shape[:2]
        h_scale, w_scale = float(self.height) / h, float(self.width) / w
        if h_scale > 1 or w_scale > 1:
            raise ValueError("the target size {} x {} must not exceed the images' {} x {}".format(
                self.height, self.width, h, w))
        resize_scale = max(h_scale, w_scale)
        img_list, ref_img, (start_h, start_w) = preprocess_views(
            images, resize_scale, self.height, self.width, self.base_image_size, device=self.device)
        cams = [crop_camera(scale_camera(cam, resize_scale), start_h, start_w) for cam in cams]
        # the reference view's depth map: nearest-resized by the same scale, cropped by the images' window
        ref_depth = depth_images[0]
        if resize_scale != 1:
            ref_depth = _resize_nearest(ref_depth, scaled_size(ref_depth.shape[0], resize_scale),
                                        scaled_size(ref_depth.shape[1], resize_scale))
        ref_depth = ref_depth[start_h:start_h + img_list.shape[2], start_w:start_w + img_list.shape[3]].copy()
        return {
            "img_list": img_list,
            "cam_params_list": torch.tensor(np.stack(cams, axis=0)).float(),
            "gt_depth_img": ref_depth,
            "depth_list": torch.tensor(np.stack(depth_images, axis=0)).unsqueeze(1).float(),
            "ref_img": ref_img[0] if self.device is not None else ref_img[0].numpy(),
        }
