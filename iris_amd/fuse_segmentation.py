"""``python -m iris_amd.fuse_segmentation``: the reference's utils/fuse_segmentation.py command -- the per-view part segmentations of a `real` or
`synthetic` scene (segmentation/{:03d}.exr, what the trainers read under --has_part) made consistent across views.

Every view's pixels vote for their segment id at the triangle they see; each triangle takes the id with the most votes (the lower id among equal counts,
0 without a vote); every view is painted again from the triangles' labels (0 where its ray hits nothing).  One fused launch per view and pass
(utils/segmentation.py, csrc/iris_labels.h).  By default, as the reference: the new files go to `segmentation-new`, then `segmentation` is renamed to
`segmentation-old` and `segmentation-new` to `segmentation`; --output DIR writes there instead and renames nothing.

Where the reference leaves a choice, or cannot run:
  --split all (default)    real: every capture of cam.txt, view i <-> segmentation/{i:03d}.exr (the name the trainers' loader reads); synthetic: the frames
                           of <scene>/train, files under train/segmentation.  --split train: the train split only.
  row width                n_labels = seg_num + 1, so that the largest id can win; --compat reference: n_labels = seg_num, the reference's arithmetic
                           with the votes for the largest id dropped (the reference spills them into the next triangle's unread column 0 and fails on the
                           last triangle)
  --max_hist_gb            the dense (triangles, n_labels) uint32 histogram is refused above this size, before the device is opened
The image size is the first segmentation file's; a file of another size is refused.  There is no --res_scale."""
import os

import numpy as np
import torch

from . import _lib as L
from .utils.stage import exit_status

NAME = "fuse_segmentation"


def parser():
    import argparse
    from .utils import stage
    ap = argparse.ArgumentParser(prog="python -m iris_amd.fuse_segmentation", description="fuse the per-view part segmentations of a scene by a vote per triangle")
    ap.add_argument("--scene", type=str, required=True, help="scene path")
    ap.add_argument("--dataset", type=str, required=True, help="scene type: real | synthetic")
    ap.add_argument("--split", type=str, default="all", choices=["all", "train"], help="the views that vote and are written (default: all)")
    ap.add_argument("--compat", type=str, default="none", choices=["none", "reference"], help="reference: rows of seg_num columns, the largest id never wins")
    ap.add_argument("--max_hist_gb", type=float, default=16.0, help="largest histogram (triangles x n_labels x 4 bytes) the stage allocates")
    ap.add_argument("--output", type=str, default=None, help="write the fused maps here and rename nothing (default: swap the scene's segmentation folder)")
    stage.add_common_options(ap, "compression")
    ap.add_argument("--device", type=int, default=0)
    return ap


def load_split(dataset, root, split, img_hw):
    """-> (capture ids, views) of --split.  real: `all` is every capture of cam.txt -- the train and val halves of cameras.load_real merged by the
    capture ids of cameras.real_split_ids --, `train` the train half; a view's id names its file.  synthetic: the frames of <root>/train either way."""
    from .utils import cameras, stage
    if dataset == "synthetic":
        _, views = stage.load_views(dataset, root, None, 1.0, split="train", img_hw=img_hw)
        return list(range(len(views))), views
    with open(os.path.join(root, "cam.txt")) as fh:
        n_total = int(fh.readline())
    by_id = {}
    for half in ("train",) if split == "train" else ("train", "val"):
        ids = cameras.real_split_ids(n_total, half)
        _, views = stage.load_views(dataset, root, None, 1.0, split=half, img_hw=img_hw)
        if len(ids) != len(views):
            raise L.IrisError(f"{root}: {len(views)} cameras for {len(ids)} {half} views")
        by_id.update(zip(ids, views))
    ids = sorted(by_id)
    return ids, [by_id[i] for i in ids]


def segment_ids(path, img_hw):
    """the ids of one segmentation file, (H, W) float32: the reference's cv2.imread(path, -1)[..., 0], which is the file's B channel (read_exr orders
    R, G, B); a file of other channels gives its first.  Decoded once."""
    from .utils.exr import read_exr
    s = read_exr(path)
    if s.shape[:2] != tuple(img_hw):
        raise L.IrisError(f"{path}: the map is {s.shape[0]} x {s.shape[1]}, the first one {img_hw[0]} x {img_hw[1]}: resizing segmentation maps is not built")
    return np.ascontiguousarray(s[..., 2 if s.shape[2] == 3 else 0], dtype=np.float32)


def open_fusion(args):
    """the host half: everything that can be refused is refused here, before the device is touched
    -> (faces count, mesh (vertices, faces), img_hw, ids, views, host maps, n_labels, seg_num, input folder, output folder, swap)"""
    from .utils import stage
    from .utils.exr import read_exr_header
    from .utils.path_tracing import load_mesh
    if args.dataset not in ("real", "synthetic"):
        raise L.IrisError(f"--dataset {args.dataset}: the segmentation fusion is built for the real and synthetic layouts")
    root = args.scene
    mesh = stage.mesh_path(args.dataset, root)
    data_root = os.path.join(root, "train") if args.dataset == "synthetic" else root
    seg_dir = os.path.join(data_root, "segmentation")
    swap = args.output is None
    out_dir = os.path.join(data_root, "segmentation-new") if swap else args.output
    if swap:
        for taken in (os.path.join(data_root, "segmentation-old"), out_dir):
            if os.path.lexists(taken):
                raise L.IrisError(f"{taken} exists already: move it away (the fused maps are written to segmentation-new, and segmentation is renamed to "
                                  "segmentation-old), or write elsewhere with --output")
    if args.dataset == "real":
        with open(os.path.join(root, "cam.txt")) as fh:
            n_total = int(fh.readline())
        from .utils.cameras import real_split_ids
        first_ids = list(range(n_total)) if args.split == "all" else real_split_ids(n_total, "train")
        if not first_ids:
            raise L.IrisError(f"{root}: --split {args.split} has no views")
        first = first_ids[0]
    else:
        first = 0
    first_path = os.path.join(seg_dir, "%03d.exr" % first)
    if not os.path.isfile(first_path):
        raise FileNotFoundError(first_path)
    h = read_exr_header(first_path)
    img_hw = (int(h["height"]), int(h["width"]))
    ids, views = load_split(args.dataset, root, args.split, img_hw)
    if not views:
        raise L.IrisError(f"{root}: --split {args.split} has no views")
    paths = [os.path.join(seg_dir, "%03d.exr" % i) for i in ids]
    for path in paths:                                                 # (headers only: a missing or mis-sized file ends the run before anything is decoded)
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
        h = read_exr_header(path)
        if (int(h["height"]), int(h["width"])) != img_hw:
            raise L.IrisError(f"{path}: the map is {h['height']} x {h['width']}, the first one {img_hw[0]} x {img_hw[1]}: resizing segmentation maps is not built")
    vertices, faces = load_mesh(mesh)
    maps = [segment_ids(path, img_hw) for path in paths]
    seg_num = 0
    for path, m in zip(paths, maps):                                   # seg_num = max(int(segmentation.max()), seg_num)   (fuse_segmentation.py:63-66)
        top = float(m.max()) if m.size else 0.0
        if not np.isfinite(top):
            raise L.IrisError(f"{path}: the largest id is {top}")
        seg_num = max(int(top), seg_num)
    n_labels = seg_num if args.compat == "reference" else seg_num + 1
    if n_labels < 2:
        raise L.IrisError(f"{seg_dir}: the largest id is {seg_num}: with rows of {n_labels} column(s) no id can be voted for")
    hist_bytes = len(faces) * n_labels * 4
    if hist_bytes > args.max_hist_gb * 2.0 ** 30:
        raise L.IrisError(f"the histogram of {len(faces)} triangles x {n_labels} ids x 4 bytes is {hist_bytes / 2.0 ** 30:.3f} GiB, more than --max_hist_gb "
                          f"{args.max_hist_gb:g}: raise it if the device has the memory (a histogram that is not dense is not built)")
    return (vertices, faces), img_hw, ids, views, maps, n_labels, seg_num, seg_dir, out_dir, swap


def main(argv=None):
    from .utils import stage
    from .utils.exr import chunk_pool, write_exr
    from .utils.path_tracing import Scene
    from .utils.segmentation import fuse, label_view
    args = parser().parse_args(argv)
    (vertices, faces), img_hw, ids, views, maps, n_labels, seg_num, seg_dir, out_dir, swap = open_fusion(args)
    device = stage.open_device(args.device, NAME)
    scene = Scene(vertices, faces, device=device)
    label_maps = [torch.from_numpy(m).to(device) for m in maps]        # float32 on the device, for the vote and for the comparison below
    tri_label, fused = fuse(scene, views, img_hw, label_maps, n_labels)
    # the summary's share: among the pixels whose ray hits the mesh, those whose id is not what it was (a hit mask costs one more launch per view; label 0
    # on a hit and a miss are the same value in the fused maps)
    ones = torch.ones(scene.n_triangles, dtype=torch.int32, device=device)
    hits, changed = torch.zeros((), dtype=torch.int64, device=device), torch.zeros((), dtype=torch.int64, device=device)
    for view, before, after in zip(views, label_maps, fused):
        hit = label_view(scene, ones, camera=view, img_hw=img_hw, dtype=torch.uint8).bool()
        hits += hit.sum()
        changed += (hit & (before.reshape(-1).trunc() != after)).sum()
    os.makedirs(out_dir, exist_ok=True)
    pool = chunk_pool()
    for i, after in zip(ids, fused):
        write_exr(os.path.join(out_dir, "%03d.exr" % i), after.reshape(*img_hw, 1).expand(*img_hw, 3).cpu().numpy(), args.compression, pool=pool)
    if swap:
        os.rename(seg_dir, os.path.join(os.path.dirname(seg_dir), "segmentation-old"))
        os.rename(out_dir, seg_dir)
    if args.dataset == "real" and args.split == "train":
        print(f"{NAME}: --split train: the validation captures have no file in the new folder", flush=True)
    hits, changed, labelled = int(hits), int(changed), int((tri_label > 0).sum())
    print(f"{NAME}: {len(views)} views of {img_hw[0]} x {img_hw[1]}, {scene.n_triangles} triangles, n_labels {n_labels} (largest id {seg_num}), "
          f"{labelled} triangles labelled, {changed} of {hits} hit pixels ({100.0 * changed / max(hits, 1):.2f} %) changed their id -> "
          f"{seg_dir if swap else out_dir}", flush=True)
    return 0


def cli(argv=None):
    return exit_status(NAME, main, argv)


if __name__ == "__main__":
    raise SystemExit(cli())
