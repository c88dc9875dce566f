"""Golden arrays for the image / camera preprocessing, produced by the reference's own utils/preprocess.py.

    python tests/golden/make_preprocess_golden.py      # build container only (imports /root/reference)

At scale 1 ``cv2.resize`` is the identity, so the reference's chain ``scale_dtu_input(scale=1)`` -> ``crop_dtu_input`` ->
``norm_image`` is plain NumPy and pins pointmvsnet_amd/utils/preprocess.py bit for bit.  ``cv2`` is not installed: a stub
module supplies ``resize``, which returns a copy for fx == fy == 1 and raises otherwise (the reference's resize at other
scales is OpenCV's fixed-point kernel and is not restated anywhere in this project).

Inputs: 2 seeded views of 72 x 100 and their cameras.  Cases (height, width, base_image_size), covering both branches of
the crop rule on both axes:
  a  (64, 96, 32)    size > target on both axes                    -> 64 x 96, offsets (4, 2)
  b  (80, 128, 24)   size <= target; 72 is a multiple of 24, 100 is not -> 72 x 96, offsets (0, 2)
  c  (72, 100, 16)   size == target (the "else" branch), neither a multiple of 16 -> 64 x 96, offsets (4, 2)
Stored per case: the cropped uint8 images, the standardised float32 images (V, h, w, 3) and the cameras; plus
``scale_camera(cam, 0.8)`` of every input camera.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

cv2 = types.ModuleType("cv2")
cv2.INTER_NEAREST, cv2.INTER_LINEAR = 0, 1


def _resize(img, dsize, fx=0, fy=0, interpolation=1):
    if dsize is not None or fx != 1 or fy != 1:
        raise NotImplementedError("cv2 stub: only fx == fy == 1")
    return np.array(img, copy=True)


cv2.resize = _resize
sys.modules["cv2"] = cv2

spec = importlib.util.spec_from_file_location("ref_preprocess", "/root/reference/pointmvsnet/utils/preprocess.py")
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

CASES = {"a": (64, 96, 32), "b": (80, 128, 24), "c": (72, 100, 16)}


def make_inputs(seed=0):
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, (2, 72, 100, 3), dtype=np.uint8)
    images[1, :, :, 2] = (images[1, :, :, 2] // 8) + 100             # a low-contrast channel: small variance
    cams = np.zeros((2, 2, 4, 4))
    for v in range(2):
        cams[v, 0] = np.eye(4)
        cams[v, 0, :3, 3] = rng.normal(0.0, 50.0, 3)
        cams[v, 1, 0, 0], cams[v, 1, 1, 1] = 2892.33 + v, 2883.18 - v
        cams[v, 1, 0, 2], cams[v, 1, 1, 2] = 823.205 + 0.37 * v, 619.071 - 0.11 * v
        cams[v, 1, 2, 2] = 1.0
        cams[v, 1, 3] = (425.0, 2.5 * 1.6, 128.0, 425.0 + 4.0 * 127)
    return images, cams


def main():
    images, cams = make_inputs()
    out = {"images": images, "cams": cams, "scaled_cams_0p8": np.stack([ref.scale_camera(c, 0.8) for c in cams])}
    for name, (height, width, base) in CASES.items():
        ims, cs = ref.scale_dtu_input([im.copy() for im in images], [c.copy() for c in cams], scale=1)
        ims, cs = ref.crop_dtu_input(ims, cs, height=height, width=width, base_image_size=base)
        out["case_%s_args" % name] = np.array([height, width, base])
        out["case_%s_crop" % name] = np.stack(ims)
        out["case_%s_norm" % name] = np.stack([ref.norm_image(im) for im in ims])
        out["case_%s_cams" % name] = np.stack(cs)
        print(name, np.stack(ims).shape, out["case_%s_norm" % name].dtype)
    path = os.path.join(HERE, "preprocess.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
