"""The stages BEFORE the bake, on the device: they write the two files the bake loads.

  bake_slf         slf_bake.py:69-145          scene bounds -> occupancy histogram -> VoxelSLF mean-pooled radiance -> vslf.npz
  refine_slf       slf_refine.py:85-108        re-pool an existing grid with new radiance
  extract_emitters extract_emitter_ldr.py:72-115  per-triangle mean radiance -> threshold -> emitter.pth

`views` is any iterable of batch dicts, in either of two forms:
    {'rays': (N,6) [origin, direction], 'rgbs': (N,3), 'exposure': ...}                          the rows the reference's datasets give
    {'camera': a view dict of utils/cameras.py, 'img_hw': (H, W), 'image': (H,W,3), 'exposure': ...}   the rays are generated in the kernel
'rgbs' / 'image' (needed where radiance is pooled) is a uint8 or float32 tensor on the host or on the device; an 8-bit photograph stays 8-bit and is
decoded as u / 255 in the kernel.  Without `crf=` the values are LINEAR radiance and pooled as given.  With `crf=model` (an iris_amd.model.crf.EmorCRF on
the device) they are the LDR photographs and every batch also carries 'exposure': the functions pool ``model.inverse(rgbs, exposure)`` as the reference
does (slf_bake.py:128-129, slf_refine.py:96-97, extract_emitter_ldr.py).

Every pass over a view is ONE launch (utils/gbuffer.py pool_view, csrc/iris_prebake.h): ray, closest hit and the pass's sink, with no intermediate tensor
and no host synchronisation.  The passes retrace, as the reference does (tools/bench_prebake.py reports the trace's share of a pass).  Pooling is atomic
accumulation in HBM, so float sums agree with the reference's sequential CPU scatter up to summation order, integer results and the bounds exactly.
Everything stays on the device; only the final state dict goes to the host, in the reference's file format (so SLFEmitter(emitter_path, slf_path) loads
either side's files).

``python -m iris_amd.slf_bake`` is the reference's slf_bake.py command: it writes <output>/vslf.npz from a scene's photographs.
"""
import torch
import torch.nn.functional as NF

from . import _lib as L
from .model.slf import VoxelSLF
from .utils.gbuffer import pool_view
from .utils.stage import exit_status


def _view_args(batch, device, radiance=False, crf=None):
    """pool_view's ray (and radiance) arguments of one batch dict, either form"""
    if "camera" in batch:
        args = {"camera": batch["camera"], "img_hw": batch["img_hw"]}
        image = batch.get("image")
    else:
        args = {"rays": batch["rays"].to(device=device, dtype=torch.float32)}
        image = batch.get("rgbs")
    if radiance:
        image = torch.as_tensor(image)
        args["image"] = image.to(device) if image.dtype == torch.uint8 else image.to(device=device, dtype=torch.float32)
        if crf is not None:
            args["exposure"] = batch["exposure"]
    return args


def _crf_tables(crf):
    """(knots, inverse table) of the response model: built once per pass (the reference rebuilds the same table for every view)"""
    return None if crf is None else (crf.grid, crf.get_inv_crf())


def drop_hits(views):
    """Kept for callers of the earlier interface, where primary hits could stay attached to the batches: nothing is attached any more."""
    for batch in views:
        if isinstance(batch, dict):
            batch.pop("_iris_hits", None)


def scene_bounds(scene, views, dataset, device, cache=False):
    """slf_bake.py:69-93 including its scannetpp centre (``voxel_c = voxel_min + voxel_max``, not halved: kept, the files depend on it).
    cache: accepted and unused (every pass traces)."""
    # running min / max stay on the device (one host sync at the end); they start at the reference's values (1000, 0)
    bounds = torch.tensor([1000.0, 0.0], device=device)
    for batch in views:
        pool_view(scene, bounds=bounds, **_view_args(batch, device))
    voxel_min, voxel_max = bounds.cpu()
    if dataset in ("synthetic", "real"):
        voxel_min = 1.1 * voxel_min
        voxel_max = 1.1 * voxel_max
    else:
        voxel_c = voxel_min + voxel_max
        voxel_min, voxel_max = voxel_c + (voxel_min - voxel_c) * 1.1, voxel_c + (voxel_max - voxel_c) * 1.1
    return torch.as_tensor(voxel_min, dtype=torch.float32), torch.as_tensor(voxel_max, dtype=torch.float32)


def visible_voxels(scene, views, voxel_min, voxel_max, res_spatial, device, cache=False):
    """slf_bake.py:95-114: SpatialHist (res,res,res) f32 [z,y,x]; mask = SpatialHist > 0."""
    hist = torch.zeros(res_spatial, res_spatial, res_spatial, device=device, dtype=torch.float32)
    for batch in views:
        pool_view(scene, hist=hist, voxel_range=(float(voxel_min), float(voxel_max)), **_view_args(batch, device))
    return hist


def pool_radiance(scene, views, vslf, device, cache=False, crf=None):
    """slf_bake.py:120-138 / slf_refine.py:90-106: scatter every valid primary hit's radiance into its voxel, then average."""
    vslf = vslf.to(device)
    tables = _crf_tables(crf)
    for batch in views:
        pool_view(scene, vslf=vslf, crf_tables=tables, **_view_args(batch, device, True, crf))
    vslf.radiance = vslf.radiance / vslf.count[..., None].float().clamp_min(1)
    vslf.refresh()                                    # the buffer was rebound: the device tables are rebuilt at the next lookup
    return vslf


def bake_slf(scene, views, res_spatial=256, dataset="scannetpp", device="cuda", crf=None):
    """-> the dict slf_bake.py:140-145 saves as vslf.npz: {'mask', 'voxel_min', 'voxel_max', 'weight'}  (tensors on the host)."""
    views = list(views)
    device = torch.device(device)
    voxel_min, voxel_max = scene_bounds(scene, views, dataset, device)
    hist = visible_voxels(scene, views, voxel_min, voxel_max, res_spatial, device)
    mask = hist > 0
    vslf = VoxelSLF(mask, voxel_min.item(), voxel_max.item())            # index grid and buffers built on the device the mask was counted on
    vslf = pool_radiance(scene, views, vslf, device, crf=crf)
    return {"mask": mask.cpu(), "voxel_min": voxel_min.item(), "voxel_max": voxel_max.item(),
            "weight": {k: v.cpu() for k, v in vslf.state_dict().items()}}


def refine_slf(state_dict, scene, views, device="cuda", crf=None):
    """slf_refine.py:85-108: same grid, radiance pooled anew; returns the updated dict."""
    vslf = VoxelSLF(state_dict["mask"], state_dict["voxel_min"], state_dict["voxel_max"])
    vslf = pool_radiance(scene, list(views), vslf, torch.device(device), crf=crf)
    out = dict(state_dict)
    out["weight"] = {k: v.cpu() for k, v in vslf.state_dict().items()}
    return out


def extract_emitters(scene, vertices, faces, views, threshold, device="cuda", crf=None):
    """extract_emitter_ldr.py:77-115 (mode 'export'): per-triangle mean of the radiance of the primary hits that landed on it, max over
    the channels, > threshold -> emitter; returns the dict saved as emitter.pth."""
    device = torch.device(device)
    vertices = torch.as_tensor(vertices, dtype=torch.float32); faces = torch.as_tensor(faces).long()
    n_face = len(faces)
    triangle_radiance = torch.zeros(n_face, 3, device=device)
    triangle_count = torch.zeros(n_face, device=device)
    tables = _crf_tables(crf)
    for batch in views:
        pool_view(scene, tri_sum=triangle_radiance, tri_count=triangle_count, crf_tables=tables, **_view_args(batch, device, True, crf))
    mean = triangle_radiance / triangle_count.unsqueeze(-1).clamp_min(1)
    is_emitter = (torch.max(mean, dim=-1)[0] > threshold).cpu()
    ev = vertices[faces[is_emitter]]
    area = torch.cross(ev[:, 1] - ev[:, 0], ev[:, 2] - ev[:, 0], dim=-1)
    return {"is_emitter": is_emitter, "emitter_vertices": ev, "emitter_area": area.norm(dim=-1) / 2.0, "emitter_normal": NF.normalize(area, dim=-1),
            "emitter_radiance": torch.zeros(n_face, 3)}


# ---- the command line (slf_bake.py:25-145)
def add_prebake_options(ap):
    """what the reference's three pre-bake scripts share, and this project's additions to them"""
    from .utils import stage
    ap.add_argument("--dataset_root", type=str, help="dataset root")
    ap.add_argument("--scene", type=str, required=True, help="dataset folder (scannetpp: the scene id under --dataset_root)")
    ap.add_argument("--output", type=str, required=True, help="output path")
    ap.add_argument("--dataset", type=str, required=True, help="dataset type: synthetic | real | scannetpp")
    ap.add_argument("--ldr_img_dir", type=str, default=None)
    ap.add_argument("--res_scale", type=float, default=1.0)
    stage.add_common_options(ap, "cameras", "emor_path", "max_views")
    ap.add_argument("--device", type=int, default=0)


def open_prebake(args, name, need_exposure):
    """the host half of a pre-bake stage: (mesh file, img_hw, views, photographs).  need_exposure: the stage divides by the views' exposures, which the real and
    synthetic layouts only have under --ldr_img_dir (the reference divides by None there)."""
    from .utils import stage
    if need_exposure and not args.cameras and args.dataset in ("real", "synthetic") and not args.ldr_img_dir:
        raise L.IrisError(f"--ldr_img_dir is needed: {name} divides the photographs by their exposures (<ldr_img_dir>/cam/exposure.npy)")
    root = args.dataset_root if args.dataset == "scannetpp" else args.scene
    mesh = stage.mesh_path(args.dataset, root, args.scene)
    img_hw, views, photographs = stage.load_photographs(args.dataset, root, args.scene, args.res_scale, ldr_img_dir=args.ldr_img_dir, cameras_json=args.cameras,
                                                        max_views=args.max_views)
    if not views:
        raise L.IrisError(f"{name}: the train split has no views")
    resize = stage.layout_resizes(args.dataset, args.cameras)          # the scannetpp layout's 8-bit photographs are resized on the device (--res_scale)
    for path, _ in photographs:                                        # everything that can be refused is refused before the device is touched
        stage.check_photograph_size(path, img_hw, resize)
    return mesh, img_hw, views, photographs


def parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m iris_amd.slf_bake", description="bake the voxel surface light field vslf.npz from a scene's photographs")
    add_prebake_options(ap)
    ap.add_argument("--voxel_num", type=int, default=256, help="resolution for voxel radiance cache")
    return ap


def main(argv=None):
    import os
    from .model.crf import EmorCRF
    from .utils import stage
    from .utils.path_tracing import load_scene
    args = parser().parse_args(argv)
    mesh, img_hw, views, photographs = open_prebake(args, "slf_bake", need_exposure=True)
    model_crf = EmorCRF(emor_path=args.emor_path)                       # model_crf = EmorCRF()   (slf_bake.py:67): default dimension, zero weights
    device = stage.open_device(args.device, "slf_bake")
    scene = load_scene(mesh, device=device)
    model_crf.to(device)
    batches = stage.photograph_batches(views, img_hw, photographs, device, resize=stage.layout_resizes(args.dataset, args.cameras))
    out = bake_slf(scene, batches, res_spatial=args.voxel_num, dataset=args.dataset, device=device, crf=model_crf)
    os.makedirs(args.output, exist_ok=True)
    torch.save(out, os.path.join(args.output, "vslf.npz"))
    print(f"slf_bake: {len(views)} views of {img_hw[0]} x {img_hw[1]}, {int(out['mask'].sum())} of {args.voxel_num}^3 voxels seen, "
          f"bounds [{out['voxel_min']:.6g}, {out['voxel_max']:.6g}] -> {os.path.join(args.output, 'vslf.npz')}", flush=True)
    return 0


def cli(argv=None):
    return exit_status("slf_bake", main, argv)


if __name__ == "__main__":
    raise SystemExit(cli())
