"""The files of a training scene -> the host arrays a PixelSet and a ShadingCache are built from.

Reference: ``InvRealDatasetLDR`` (utils/dataset/real_ldr.py:261-386) and ``InvSyntheticDatasetLDR`` (synthetic_ldr.py:260-380) with ``pixel=True`` and an
``img_dir``: the LDR images ``<img_dir>/{:03d}_0001.png``, the albedo prior ``<img_dir>/albedo/{:03d}_0001.png``, the exposures
``<img_dir>/cam/exposure.npy``, the segment ids in channel 0 of ``segmentation/{:03d}.exr`` (``IndexMA/{:03d}_0001.exr`` for a synthetic scene with part
segmentation) and the baked shadings of ``cache_dir``.  8-bit images stay 8-bit (PixelSet decodes them as the reference's ``u / 255``).

File indices: the real layout names its images by the id of the view in the capture (the train split leaves out views 0, 10, .. 150) and its cache files by
the view's position in the split (real_ldr.py:342-363); the synthetic layout (rooted at ``<scene>/train``) uses the frame index for both.

The scannetpp layout (``InvScannetpp``, scannetpp/dataset.py:263-384: ``psdf/images``, ``psdf/albedo``, ``psdf/seg`` by the view's file name, exposures all 1)
is the one that takes a ``res_scale``: its 8-bit files are uploaded at the size they have and resized to the views' size on the device
(iris_amd/utils/resize.py: linear as cv2.resize for the images, nearest as PIL for the segment ids).

Not built, and refused with a message: for the real and synthetic layouts an image whose size differs from the scene's and ``res_scale != 1`` (their
reference classes take no scale); resizing float32 (EXR) maps; a shading cache baked at another scale than the one trained at.
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


EIGHT_BIT_MODES = ("1", "L", "P", "LA", "PA", "RGB", "RGBA", "RGBX", "CMYK", "YCbCr")      # PIL modes of one byte per channel


def _scannetpp_paths(root, scene, name):
    psdf = os.path.join(root, "data", scene, "psdf")
    return [os.path.join(psdf, d, name) for d in ("images", "albedo", "seg")]


def _check_eight_bit(path, im):
    if im.mode not in EIGHT_BIT_MODES:
        raise L.IrisError(f"{path}: expected an 8-bit image, got PIL mode {im.mode}")


def check_scannetpp_files(root, scene, res_scale=1.0):
    """what can be refused of a scannetpp training scene without a device and without decoding an image -> (img_hw, views) of the train split.  IrisError
    naming the layout and the missing path for psdf/train_test_lists.json, psdf/transforms_all.json, an empty split and the mesh; FileNotFoundError or
    IrisError for the FIRST view's three files (images, albedo, seg: their headers only)."""
    from PIL import Image
    scene = scene or ""
    psdf = os.path.join(root, "data", scene, "psdf")
    for name in ("train_test_lists.json", "transforms_all.json"):
        if not os.path.isfile(os.path.join(psdf, name)):
            raise L.IrisError(f"--dataset scannetpp: {os.path.join(psdf, name)} is missing (the scannetpp layout is <root>/data/<--scene>/psdf with "
                              "train_test_lists.json, transforms_all.json, images/, albedo/ and seg/)")
    img_hw, views = cameras.load_scannetpp(root, scene, res_scale, "train")
    if not views:
        raise L.IrisError(f"--dataset scannetpp: {psdf}: the train split has no views")
    if min(img_hw) < 1:
        raise L.IrisError(f"--dataset scannetpp: --res_scale {res_scale} leaves views of {img_hw[0]} x {img_hw[1]} pixels")
    mesh_path("scannetpp", root, scene)
    for path in _scannetpp_paths(root, scene, views[0]["name"]):
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
        with Image.open(path) as im:
            _check_eight_bit(path, im)
    return img_hw, views


def _load_scannetpp(root, scene, res_scale, cache_dir, device):
    """InvScannetpp(root, scene, split='train', pixel=True, cache_dir, res_scale) (utils/dataset/scannetpp/dataset.py:263-384): per view name of the train
    split the photograph psdf/images/<name> and the albedo prior psdf/albedo/<name> through open_png -- cv2.resize, linear, when the file's size is not
    img_hw --, the segment ids from channel B of psdf/seg/<name> (cv2.imread(...)[:, :, 0] is PIL's convert('RGB') channel 2) through sample_nearest when
    the size differs; exposures all 1 (np.ones).  Every file is decoded on the host, uploaded at full size and resized on the device
    (utils.resize.resize_u8): the lists hold HIP tensors, which PixelSet takes as they are."""
    import torch
    from PIL import Image
    from ..resize import resize_u8
    img_hw, views = check_scannetpp_files(root, scene, res_scale)
    device = torch.device(device)
    if device.type != "cuda":
        raise L.IrisError(f"{device}: the scannetpp training files are resized on a HIP device (there is no CPU fallback)")

    def decode(path):
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
        with Image.open(path) as im:
            _check_eight_bit(path, im)
            return torch.from_numpy(np.array(im.convert("RGB"))).to(device)

    rgb, albedo, seg = [], [], []
    for view in views:
        image, prior, ids = (decode(p) for p in _scannetpp_paths(root, scene, view["name"]))
        rgb.append(resize_u8(image, img_hw, "linear"))
        albedo.append(resize_u8(prior, img_hw, "linear"))
        seg.append(resize_u8(ids[..., 2].contiguous(), img_hw, "nearest").reshape(-1))
    hw = img_hw[0] * img_hw[1]
    cache = None
    if cache_dir is not None:
        from ..shading_cache import ShadingCache
        cache = ShadingCache.from_exr_dir(cache_dir, len(views), device=device)        # cache files are numbered by position in the split
        if len(cache) != hw * len(views):
            raise L.IrisError(f"{cache_dir}: the maps hold {len(cache) // len(views)} pixels per view, the images {hw} (a cache baked at another --res_scale?)")
    return dict(img_hw=img_hw, views=views, synthetic=False, rgb=rgb, int_albedo=albedo, segmentation=seg, exposure=np.ones(len(views), np.float32), cache=cache,
                mesh_path=mesh_path("scannetpp", root, scene))


def load_training_files(dataset, root, ldr_img_dir, *, has_part=0, res_scale=1.0, cache_dir=None, device="cuda", scene=None):
    """-> dict(img_hw, views, synthetic, rgb [V x (H,W,3) uint8], int_albedo [V x (H,W,3) uint8], segmentation [V x (H*W)], exposure (V) float32,
    cache: ShadingCache or None, mesh_path) for ``--dataset real DIR`` / ``--dataset synthetic DIR`` (host arrays, segment ids float32) and for
    ``--dataset scannetpp ROOT --scene ID`` (_load_scannetpp: HIP tensors, segment ids uint8, any res_scale; ldr_img_dir and has_part are not needed and
    are ignored, as in the reference)."""
    if dataset == "scannetpp":
        return _load_scannetpp(root, scene, res_scale, cache_dir, device)
    if dataset not in ("real", "synthetic"):
        raise L.IrisError(f"--dataset {dataset}: expected real, synthetic or scannetpp")
    if float(res_scale) != 1.0:
        raise L.IrisError(f"--res_scale {res_scale}: resizing the training images is built for the scannetpp layout only (real and synthetic: res_scale 1)")
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
