"""Camera lists (intrinsics + camera-to-world) of a split's views for the command-line stages (utils/stage.py: load_views).

Only the pose / intrinsics part of the reference's dataset classes is needed by bake_shading (images are never read there):
  synthetic : {scene}/{split}/transforms.json, focal = 0.5 w / tan(0.5 camera_angle_x)          (utils/dataset/synthetic_ldr.py:129-150)
  real      : {scene}/cam.txt (origin, lookat, up per view) + K_list.txt, train or val split   (utils/dataset/real_ldr.py:25-34,85-166)
  scannetpp : {dataset_root}/data/{scene}/psdf/train_test_lists.json + transforms_all.json (nerfstudio layout: one shared
              fl_x fl_y cx cy h w, per frame an OpenGL camera-to-world), the split's list            (utils/dataset/scannetpp/dataset.py:78-141)
  generic   : a JSON file {"img_hw":[H,W], "views":[{"K":3x3, "c2w":3x4}, ...]} (OpenCV convention); a view may carry "image" and "exposure"
and the render trajectory of the first three (load_trajectory: render_traj.npy seen through the split's camera; the datasets' load_traj=True).
"""
import json
import os

import numpy as np


def _img_hw_from_exr(path, res_scale):
    from .exr import read_exr_header
    h = read_exr_header(path)
    return int(h["height"] * res_scale), int(h["width"] * res_scale)


def load_synthetic(scene_dir, res_scale=1.0, img_hw=None, split="train"):
    root = os.path.join(scene_dir, split)
    with open(os.path.join(root, "transforms.json")) as fh:
        meta = json.load(fh)
    if img_hw is None:
        img_hw = _img_hw_from_exr(os.path.join(root, "Image", "000_0001.exr"), res_scale)
    h, w = img_hw
    focal = float(0.5 * w / np.tan(0.5 * meta["camera_angle_x"]))
    views = [{"kind": "synthetic", "focal": focal, "c2w": np.asarray(f["transform_matrix"], np.float32)[:3, :4]} for f in meta["frames"]]
    return img_hw, views


def _read_cam_params(path):
    with open(path) as fh:
        rows = fh.read().splitlines()
    n = int(rows[0])
    a = np.array([r.split() for r in rows[1:1 + 3 * n]], dtype=np.float32)
    return np.split(a, n, axis=0)


def real_split_ids(n_views, split="train"):
    """capture ids of a split of the real layout (get_split_ids, real_ldr.py:85-91): views 0, 10, .. 150 validate, every other view trains.  The ONE
    statement of the rule: the camera list, the training files and the photographs' paths (files named by capture id) all take it from here."""
    val_ids = {i * 10 for i in range(16)}
    return [i for i in range(int(n_views)) if (i in val_ids) != (split == "train")]


def load_real(scene_dir, res_scale=1.0, img_hw=None, split="train"):
    if img_hw is None:
        img_hw = _img_hw_from_exr(os.path.join(scene_dir, "Image", "000_0001.exr"), res_scale)
    views = []
    cams = _read_cam_params(os.path.join(scene_dir, "cam.txt"))
    Ks = _read_cam_params(os.path.join(scene_dir, "K_list.txt"))
    keep = set(real_split_ids(len(cams), split))
    for i, (cam, K) in enumerate(zip(cams, Ks)):
        if i not in keep:
            continue
        origin, lookat, up = cam[0], cam[1], cam[2]
        at = (lookat - origin) / np.linalg.norm(lookat - origin)
        R = np.stack((np.cross(-up, at), -up, at), -1).astype(np.float32)   # OpenGL (origin, lookat, up) -> OpenCV c2w
        K = K.copy(); K[:2, :] *= res_scale
        views.append({"kind": "real", "K": K.astype(np.float32), "c2w": np.hstack((R, origin.reshape(3, 1))).astype(np.float32)})
    return img_hw, views


def load_scannetpp(dataset_root, scene_id, res_scale=1.0, split="train"):
    """The pose list of the reference's ``Scannetpp(dataset_root, scene_id, split, pixel=False, res_scale)`` (utils/dataset/scannetpp/dataset.py:78-141;
    built at bake_shading.py:68, refine_shading.py:73, slf_bake.py:62): image size ``(int(h*s), int(w*s))``; ONE intrinsic matrix for every view, its first
    two rows scaled by ``s`` (formed in double, rounded to f32 once, as ``torch.tensor(Ks).float()``); per frame of ``transforms_all.json`` whose file name
    is in the split's list, the 4x4 ``transform_matrix`` with its y and z camera axes negated (OpenGL -> OpenCV) and the top three rows kept; views ordered
    by the position of their name in the split's list (frames not in it are skipped; a listed name without a frame has no view).  The images under
    ``psdf/images`` are never opened: the bake does not use them."""
    root = os.path.join(dataset_root, "data", scene_id, "psdf")
    with open(os.path.join(root, "train_test_lists.json")) as fh:
        lists = json.load(fh)
    names = lists["train"] if split == "train" else lists["test"] if split == "test" else lists["train"] + lists["test"]
    with open(os.path.join(root, "transforms_all.json")) as fh:
        meta = json.load(fh)
    img_hw = (int(meta["h"] * res_scale), int(meta["w"] * res_scale))
    K = np.array([[meta["fl_x"], 0, meta["cx"]], [0, meta["fl_y"], meta["cy"]], [0, 0, 1]], dtype=np.float64)
    K[:2] *= res_scale
    K = K.astype(np.float32)
    first = {}
    for i, n in enumerate(names):                                      # list.index(): the FIRST position of a name
        first.setdefault(n, i)
    found = []
    for frame in meta["frames"]:
        name = frame["file_path"].split("/")[-1]
        if name not in first:
            continue
        c2w = np.array(frame["transform_matrix"], dtype=np.float64)
        c2w[:3, 1:3] *= -1
        found.append((first[name], c2w[:3].astype(np.float32)))
    order = np.argsort(np.array([i for i, _ in found], dtype=np.int64)) if found else []   # the reference's np.argsort(ids)
    views = [{"kind": "real", "K": K.copy(), "c2w": found[j][1], "name": names[found[j][0]]} for j in order]
    return img_hw, views


def load_generic(json_path, res_scale=1.0, extras=False):
    """extras: every view also gets 'image' (the photograph's path or None; a relative one is taken from the JSON file's folder) and 'exposure' (default 1.0)"""
    with open(json_path) as fh:
        meta = json.load(fh)
    h, w = meta["img_hw"]
    views = []
    for v in meta["views"]:
        K = np.asarray(v["K"], np.float32).reshape(3, 3).copy(); K[:2, :] *= res_scale
        views.append({"kind": "real", "K": K, "c2w": np.asarray(v["c2w"], np.float32).reshape(-1)[:12].reshape(3, 4)})
        if extras:
            image = v.get("image")
            if image and not os.path.isabs(image):
                image = os.path.join(os.path.dirname(os.path.abspath(json_path)), image)
            views[-1].update(image=image, exposure=float(v.get("exposure", 1.0)))
    return (int(h * res_scale), int(w * res_scale)), views


def trajectory_path(dataset, root, scene=None):
    """where a scene's render trajectory lies: <root>/render_traj.npy for synthetic (the scene folder, not the split's) and real,
    <root>/data/<scene>/psdf/render_traj.npy for scannetpp (synthetic_ldr.py:187, real_ldr.py:205, scannetpp/dataset.py:176)"""
    if dataset == "scannetpp":
        return os.path.join(root, "data", scene, "psdf", "render_traj.npy")
    return os.path.join(root, "render_traj.npy")


def load_trajectory(dataset, root, scene, res_scale, img_hw=None, split="val"):
    """The views of the datasets' load_traj=True (render_video.py, render_relight.py --mode traj): -> (img_hw, views), one view per frame of render_traj.npy.
    The file holds (N,3,4) or (N,4,4) camera-to-world matrices (the top three rows are used, cast to float32 as torch.FloatTensor does); every frame is seen
    through the loaded split's camera: the split's focal for synthetic, the FIRST view's K of the split (res_scale applied) for real and scannetpp; the image
    size is the split's.  root, scene: as stage.mesh_path takes them.  A missing file is an IrisError naming the path, raised before anything else is read."""
    from .. import _lib as L
    if dataset not in ("synthetic", "real", "scannetpp"):
        raise L.IrisError("load_trajectory: --dataset {!r}: synthetic | real | scannetpp".format(dataset))
    path = trajectory_path(dataset, root, scene)
    if not os.path.isfile(path):
        raise L.IrisError("render trajectory not found: " + path)
    traj = np.load(path)
    if traj.ndim != 3 or tuple(traj.shape[1:]) not in ((3, 4), (4, 4)):
        raise L.IrisError(f"{path}: expected (N,3,4) or (N,4,4) camera-to-world matrices, got {traj.shape}")
    traj = np.ascontiguousarray(traj[:, :3, :], dtype=np.float32)
    if dataset == "synthetic":
        img_hw, views = load_synthetic(root, res_scale, img_hw, split=split)
    elif dataset == "real":
        img_hw, views = load_real(root, res_scale, img_hw, split=split)
    else:
        img_hw, views = load_scannetpp(root, scene, res_scale, split=split)
    if not views:
        raise L.IrisError(f"load_trajectory: split {split!r} has no view to take the camera from")
    first = views[0]
    camera = {"kind": "synthetic", "focal": first["focal"]} if dataset == "synthetic" else {"kind": "real", "K": first["K"]}
    return img_hw, [dict(camera, c2w=c2w) for c2w in traj]


def view_rays(view, img_hw, device, ray_diff=False):
    """Pixel-centre rays of one view on the GPU: (H*W,3) origins and unit directions; with ray_diff the four tensors (origin, direction, dxdu, dydv) the
    reference's datasets give with ray_diff=True."""
    from .dataset import real_ldr, synthetic_ldr
    if view["kind"] == "synthetic":
        return synthetic_ldr.get_rays(synthetic_ldr.get_ray_directions(img_hw[0], img_hw[1], view["focal"]), view["c2w"], focal=view["focal"] if ray_diff else None,
                                      device=device)
    return real_ldr.to_world(real_ldr.get_direction(view["K"], img_hw), view["c2w"], ray_diff, device=device)
