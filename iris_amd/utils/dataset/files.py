"""The files of a training scene -> the host arrays a PixelSet and a ShadingCache are built from.

Reference: ``InvRealDatasetLDR`` (utils/dataset/real_ldr.py:261-386) and ``InvSyntheticDatasetLDR`` (synthetic_ldr.py:260-380) with ``pixel=True`` and an
``img_dir``: the LDR images ``<img_dir>/{:03d}_0001.png``, the albedo prior ``<img_dir>/albedo/{:03d}_0001.png``, the exposures
``<img_dir>/cam/exposure.npy``, the segment ids in channel 0 of ``segmentation/{:03d}.exr`` (``IndexMA/{:03d}_0001.exr`` for a synthetic scene with part
segmentation) and the baked shadings of ``cache_dir``.  8-bit images stay 8-bit (PixelSet decodes them as the reference's ``u / 255``).

File indices: the real layout names its images by the id of the view in the capture (the train split leaves out views 0, 10, .. 150) and its cache files by
the view's position in the split (real_ldr.py:342-363); the synthetic layout (rooted at ``<scene>/train``) uses the frame index for both.

Not built, and refused with a message: an image whose size differs from the scene's, ``res_scale != 1``, the scannetpp layout.
"""
import os

import numpy as np

from ... import _lib as L
from .. import cameras
from ..exr import read_exr, read_exr_header
from ..stage import mesh_path


def _open_png(path, img_hw):
    from PIL import Image         # (the reference reads its albedo PNGs with PIL too)
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    a = np.asarray(Image.open(path).convert("RGB"))
    if a.shape[:2] != tuple(img_hw):
        raise L.IrisError(f"{path}: the image is {a.shape[0]} x {a.shape[1]}, the scene's views {img_hw[0]} x {img_hw[1]}: resizing images is not built")
    if a.dtype != np.uint8:
        raise L.IrisError(f"{path}: expected an 8-bit image, got {a.dtype}")
    return np.array(a)            # (a copy: PIL's buffer is read-only)


def _image_size(root, first_png):
    """(H, W): the reference takes it from Image/000_0001.exr (real_ldr.py:298); a scene without HDR images gives its first LDR image's"""
    hdr = os.path.join(root, "Image", "000_0001.exr")
    if os.path.isfile(hdr):
        h = read_exr_header(hdr)
        return int(h["height"]), int(h["width"])
    from PIL import Image
    if not os.path.isfile(first_png):
        raise FileNotFoundError(first_png)
    with Image.open(first_png) as im:
        return int(im.size[1]), int(im.size[0])


def load_training_files(dataset, root, ldr_img_dir, *, has_part=0, res_scale=1.0, cache_dir=None, device="cuda"):
    """-> dict(img_hw, views, synthetic, rgb [V x (H,W,3) uint8], int_albedo [V x (H,W,3) uint8], segmentation [V x (H*W) float32], exposure (V) float32,
    cache: ShadingCache or None, mesh_path) for ``--dataset real DIR`` / ``--dataset synthetic DIR``."""
    if dataset == "scannetpp":
        raise L.IrisError("--dataset scannetpp: the scannetpp training files (psdf/images, the per-scene albedo and segmentation folders) are not built; "
                          "only the real and synthetic layouts are")
    if dataset not in ("real", "synthetic"):
        raise L.IrisError(f"--dataset {dataset}: expected real or synthetic")
    if float(res_scale) != 1.0:
        raise L.IrisError(f"--res_scale {res_scale}: resizing the training images is not built (only res_scale 1)")
    if not ldr_img_dir:
        raise L.IrisError("--ldr_img_dir is needed: the BRDF-CRF stage trains on the LDR images, their exposures and their albedo prior")
    synthetic = dataset == "synthetic"
    data_root = os.path.join(root, "train") if synthetic else root
    if synthetic:
        n_total = None
        img_hw = _image_size(data_root, os.path.join(data_root, ldr_img_dir, "000_0001.png"))
        img_hw, views = cameras.load_synthetic(root, img_hw=img_hw)
        file_ids = list(range(len(views)))
    else:
        with open(os.path.join(root, "cam.txt")) as fh:
            n_total = int(fh.readline())
        file_ids = cameras.real_split_ids(n_total, "train")
        if not file_ids:
            raise L.IrisError(f"{root}: no training views ({n_total} views, all in the validation split)")
        img_hw = _image_size(data_root, os.path.join(data_root, ldr_img_dir, "%03d_0001.png" % file_ids[0]))
        img_hw, views = cameras.load_real(root, img_hw=img_hw, split="train")
    if len(views) != len(file_ids):
        raise L.IrisError(f"{root}: {len(views)} cameras for {len(file_ids)} training views")
    exposures = np.load(os.path.join(data_root, ldr_img_dir, "cam", "exposure.npy")).astype(np.float32).reshape(-1)
    if n_total is not None and exposures.shape[0] != n_total or synthetic and exposures.shape[0] != len(views):
        raise L.IrisError(f"{ldr_img_dir}/cam/exposure.npy holds {exposures.shape[0]} values for {n_total if n_total is not None else len(views)} views")
    exposures = exposures[file_ids]
    hw = img_hw[0] * img_hw[1]
    rgb, albedo, seg = [], [], []
    for i in file_ids:
        rgb.append(_open_png(os.path.join(data_root, ldr_img_dir, "%03d_0001.png" % i), img_hw))
        albedo.append(_open_png(os.path.join(data_root, ldr_img_dir, "albedo", "%03d_0001.png" % i), img_hw))
        seg_path = os.path.join(data_root, "IndexMA", "%03d_0001.exr" % i) if synthetic and has_part else os.path.join(data_root, "segmentation", "%03d.exr" % i)
        s = read_exr(seg_path)
        if s.shape[:2] != tuple(img_hw):
            raise L.IrisError(f"{seg_path}: the map is {s.shape[0]} x {s.shape[1]}, the scene's views {img_hw[0]} x {img_hw[1]}: resizing is not built")
        # the reference's `cv2.imread(path, -1)[..., 0]` is the file's B channel (cv2 orders B, G, R; read_exr R, G, B); a file of other channels gives its first
        seg.append(np.ascontiguousarray(s[..., 2 if s.shape[2] == 3 else 0], dtype=np.float32).reshape(hw))
    cache = None
    if cache_dir is not None:
        from ..shading_cache import ShadingCache
        cache = ShadingCache.from_exr_dir(cache_dir, len(views), device=device)        # cache files are numbered by position in the split
        if len(cache) != hw * len(views):
            raise L.IrisError(f"{cache_dir}: the maps hold {len(cache) // len(views)} pixels per view, the images {hw}")
    return dict(img_hw=img_hw, views=views, synthetic=synthetic, rgb=rgb, int_albedo=albedo, segmentation=seg, exposure=exposures, cache=cache,
                mesh_path=mesh_path(dataset, root))
