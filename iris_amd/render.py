"""The render stage (reference: render.py:57-298) on MI355X: for every view of a split the path-traced image (`path_tracing`, the full integrator) and, in the
same SPP // spp rounds, the scene intrinsics averaged over jittered primary rays (kd, a_prime, roughness, metallic, emission, surface light field); then the
denoiser, the camera response model, the maps on disk and PSNR -- with --metrics psnr,ssim also SSIM -- against the photograph.

Every ingredient is a HIP stage of this package: `utils.path_tracing.path_tracing`, `utils.render.render_intrinsics` (iris_render_primary + the material network +
iris_render_intrinsics), `utils.denoise.Denoiser` (the a-trous filter that stands where OptixDenoiser stands), `model.crf.EmorCRF`, `utils.exr.write_exr`, `utils.metrics.image_metrics` (SSIM on the
device: skimage's defaults restated).  With --material_metrics GT_DIR every view's material maps are also scored against a synthetic scene's
ground truth as it is rendered (utils.material_metrics: the reference's utils/metric_brdf.py table).

Not here: --light_type area (AreaEmitter), the magma colour maps (*_color.png), merge.png, crfs.png,
render_video.py / render_relight.py, and the trainers' validation(), which masks differently.
"""
import math
import os
import time

import numpy as np
import torch

from . import _lib as L
from .utils.path_tracing import path_tracing, ray_intersect
from .utils.render import MAPS, new_maps, render_intrinsics

INDIR_DEPTH = 5            # render.py:176
OUT_DIRS = ("rgb", "diffuse", "a_prime", "roughness", "metallic", "emission", "slf", "merge")      # render.py:145


def psnr(gt, img, data_range=1.0):
    """skimage.metrics.peak_signal_noise_ratio in closed form: 10 log10(data_range^2 / mean((gt - img)^2)), in float64 (render.py:236)"""
    gt, img = np.asarray(gt, np.float64), np.asarray(img, np.float64)
    mse = float(np.mean((gt - img) ** 2))
    return float("inf") if mse == 0.0 else 10.0 * math.log10(data_range * data_range / mse)


@torch.no_grad()
def render_view(scene, emitter_net, material_net, model_crf, rays, img_hw, SPP, spp, indir_depth=INDIR_DEPTH, exposure=1.0, gt=None, denoise=True, denoiser=None,
                chunk=None, metrics=("psnr",)):
    """One iteration of the reference's per-view loop (render.py:157-279).

    rays: (H*W, 12) float32 on the GPU -- origin, direction, dxdu, dydv as the datasets give them with ray_diff=True -- or the tuple of the four (H*W,3) tensors.
    SPP // spp rounds of `path_tracing(..., spp, indir_depth)` and `render_intrinsics(..., spp)`, every sum divided by the round count (:222,:241-271);
    L_full denoised (denoise=True, as the reference does; the guides are the pixel-centre primary hits) and mapped to LDR by model_crf(L, exposure) (None: no LDR);
    gt: optional (H,W,3) / (H*W,3) LDR photograph in [0,1] -> 'psnr' (data_range 1) and, with "ssim" in `metrics`, 'ssim' (render.py:238: skimage's defaults at
    data_range 1, evaluated on the device by utils.metrics.image_metrics).
    Returns {'rgb_full' (H,W,3) HDR, 'rgb_ldr' (H,W,3) or None, 'kd', 'a_prime', 'emission', 'slf' (H,W,3), 'roughness', 'metallic' (H,W), 'psnr' or None,
    'ssim' or None, 'rounds'}, device tensors; psnr and ssim Python floats."""
    unknown = set(metrics) - {"psnr", "ssim"}
    if unknown:
        raise L.IrisError(f"render_view: unknown metrics {sorted(unknown)} (psnr, ssim)")
    H, W = int(img_hw[0]), int(img_hw[1])
    if isinstance(rays, (tuple, list)):
        rays_x, rays_d, dxdu, dydv = rays
    else:
        rays = L.require_gpu(rays, torch.float32, "rays").reshape(-1, 12)
        rays_x, rays_d, dxdu, dydv = (rays[:, 3 * k:3 * k + 3].contiguous() for k in range(4))
    rays_x = L.require_gpu(rays_x, torch.float32, "rays_x").reshape(-1, 3)
    B, dev = rays_x.shape[0], rays_x.device
    if B != H * W:
        raise L.IrisError(f"render_view: {B} rays for an image of {H} x {W}")
    rounds = int(SPP) // int(spp)
    if rounds < 1:
        raise L.IrisError(f"render_view: SPP ({SPP}) // spp ({spp}) is zero: nothing would be rendered")
    L_full = torch.zeros(B, 3, device=dev)
    maps = new_maps(B, dev)
    for _ in range(rounds):
        L_round = path_tracing(scene, emitter_net, material_net, rays_x, rays_d, dxdu, dydv, spp, indir_depth).detach()
        if L_round.shape[0] != B:          # (no path continues after the primary hit: the integrator returns the un-reduced samples, as the reference's does)
            L_round = L_round.reshape(B, int(spp), 3).mean(1)
        L_full += L_round
        render_intrinsics(scene, emitter_net, material_net, rays_x, rays_d, dxdu, dydv, spp, out=maps, chunk=chunk)
    L_full = L_full / rounds
    out = {k: (maps[k] / rounds).reshape((H, W, 3) if c == 3 else (H, W)) for k, c in MAPS}
    if denoise:
        if denoiser is None:
            from .utils.denoise import Denoiser
            denoiser = Denoiser((W, H), dev)
        pos, nrm, _, _, valid = ray_intersect(scene, rays_x, torch.nn.functional.normalize(L.require_gpu(rays_d, torch.float32, "rays_d").reshape(-1, 3), dim=-1))
        denoiser.set_guides(nrm, pos, valid)
        L_full = denoiser(L_full.reshape(H, W, 3)).reshape(B, 3)
    out["rgb_full"] = L_full.reshape(H, W, 3)
    out["rgb_ldr"] = None if model_crf is None else model_crf(L_full.contiguous(), exposure).detach().reshape(H, W, 3)
    out["psnr"] = out["ssim"] = None
    if gt is not None and out["rgb_ldr"] is not None:
        g = gt.detach().cpu().numpy() if torch.is_tensor(gt) else np.asarray(gt)
        out["psnr"] = psnr(g.reshape(H, W, 3), out["rgb_ldr"].cpu().numpy(), 1.0)
        if "ssim" in metrics:
            from .utils.metrics import ssim
            g_dev = torch.as_tensor(np.ascontiguousarray(g, dtype=np.float32).reshape(H, W, 3)).to(dev)
            out["ssim"] = ssim(g_dev, out["rgb_ldr"].contiguous(), 1.0)
    out["rounds"] = rounds
    return out


def save_png(image, path):
    """render.py:37-46 save_image without the colour map: clip to [0,1], * 255, uint8.  Written only when PIL imports; returns whether it was."""
    try:
        from PIL import Image
    except ImportError:
        return False
    a = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    a = (np.clip(a, 0.0, 1.0) * 255).astype(np.uint8)
    Image.fromarray(a).save(path)
    return True


def write_view(output_path, split, i, out, compression="zip"):
    """The files of view i under the reference's tree (render.py:224-275): <output>/<split>/{rgb,diffuse,a_prime,roughness,metallic,emission}/{i:05d}_*.exr (+ .png).
    EXR through the project's three-channel writer, R,G,B meaning as imageio writes them; roughness / metallic replicated to three equal channels.  slf/ also gets
    {i:05d}_slf.exr: the reference accumulates that map and never writes it.  Returns the list of files written."""
    from .utils.exr import write_exr
    root = os.path.join(output_path, split)
    dirs = {n: os.path.join(root, n) for n in OUT_DIRS}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    files = []

    def exr(folder, name, img):
        a = img.detach().cpu().numpy()
        if a.ndim == 2:
            a = np.repeat(a[..., None], 3, -1)
        p = os.path.join(dirs[folder], "{:0>5d}_{}.exr".format(i, name))
        write_exr(p, a, compression)
        files.append(p)

    def png(folder, name, img):
        a = img
        if a.ndim == 2:
            a = a[..., None].expand(-1, -1, 3)
        p = os.path.join(dirs[folder], "{:0>5d}_{}.png".format(i, name))
        if save_png(a, p):
            files.append(p)
    exr("rgb", "rgb_full", out["rgb_full"])
    if out.get("rgb_ldr") is not None:
        png("rgb", "rgb_full", out["rgb_ldr"])
    for folder, name, key in (("diffuse", "kd", "kd"), ("a_prime", "a_prime", "a_prime"), ("roughness", "roughness", "roughness"), ("metallic", "metallic", "metallic"),
                              ("emission", "emission", "emission")):
        exr(folder, name, out[key])
        png(folder, name, out[key])
    exr("slf", "slf", out["slf"])
    return files


def write_metrics(path, psnr_list, ssim_list=None):
    """rgb/metrics.txt (render.py:283-290); views without a photograph are left out of the lists and of the means.  ssim_list (the same views, in the same order)
    None: the PSNR column only; else the reference's three columns Name, PSNR, SSIM."""
    mean = lambda l: float(np.mean([v for _, v in l])) if l else float("nan")
    if ssim_list is not None:
        if [i for i, _ in ssim_list] != [i for i, _ in psnr_list]:
            raise L.IrisError("write_metrics: the PSNR and SSIM lists name different views")
        with open(path, "w") as fh:
            fh.write("Name, PSNR, SSIM\n")
            for (i, p), (_, s) in zip(psnr_list, ssim_list):
                fh.write("{:0>5d}, {:.5f}, {:.5f}\n".format(i, p, s))
            fh.write("{:<5}, {:.5f}, {:.5f}\n".format("mean", mean(psnr_list), mean(ssim_list)))
        return
    with open(path, "w") as fh:
        fh.write("Name, PSNR\n")
        for i, p in psnr_list:
            fh.write("{:0>5d}, {:.5f}\n".format(i, p))
        fh.write("{:<5}, {:.5f}\n".format("mean", float(np.mean([p for _, p in psnr_list])) if psnr_list else float("nan")))


def build_parser():
    """The reference's render.py arguments (render.py:57-71 + configs/config.py) that matter here; the trainers' options it also registers are accepted and ignored."""
    import argparse
    from .utils import stage
    parser = argparse.ArgumentParser(description="python -m iris_amd.render: the reference's render.py on MI355X")
    parser.add_argument("--experiment_name", type=str, required=True)
    parser.add_argument("--checkpoint_path", type=str, default="./checkpoints")
    parser.add_argument("--output_path", type=str, default="outputs/kitchen_output")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--split", type=str, default="val")
    parser.add_argument("--ckpt", type=str, default="last.ckpt")
    parser.add_argument("--light_type", type=str, default="slf", choices=["slf", "area"])
    parser.add_argument("--dataset", type=str, nargs=2, default=["synthetic", "../data/indoor_synthetic/kitchen"], help="dataset type (synthetic | real | scannetpp | generic) and its path")
    parser.add_argument("--scene", type=str, default="")
    parser.add_argument("--emitter_path", type=str, required=True, help="folder holding vslf.npz, emitter.pth and vslf_0.npz (render.py:109-124)")
    parser.add_argument("--SPP", type=int, default=512)
    parser.add_argument("--spp", type=int, default=8)
    parser.add_argument("--indir_depth", type=int, default=INDIR_DEPTH)
    parser.add_argument("--crf_basis", type=int, default=3)
    parser.add_argument("--res_scale", type=float, default=1.0)
    parser.add_argument("--ldr_img_dir", type=str, default=None)
    parser.add_argument("--log_path", type=str, default="./logs")
    stage.add_ignored_trainer_options(parser)
    # additions (defaults reproduce the reference)
    stage.add_common_options(parser, "material", "cameras", "emor_path", "denoise", "compression", cameras=stage.COMMON_OPTIONS["cameras"]["help"] + "; a view may carry "
                             "\"image\" (an EXR or, with PIL, PNG photograph in [0,1]) and \"exposure\"")
    parser.add_argument("--metrics", type=str, default="psnr", choices=["psnr", "psnr,ssim"], metavar="psnr | psnr,ssim", help="columns of rgb/metrics.txt: psnr (default), or psnr,ssim -- the "
                        "reference's Name, PSNR, SSIM file, SSIM evaluated on the device")
    stage.add_common_options(parser, "seed", "max_views")
    return parser


def build_cli_parser():
    """build_parser(), --textures DIR and --material_metrics GT_DIR: what main() parses.  They stand apart because build_parser()'s option table is pinned
    entry for entry (tests/test_stage_setup_cpu.py) as the table of the options this stage had before it could render from the exported textures."""
    from .utils import stage
    parser = build_parser()
    stage.add_common_options(parser, "textures")
    parser.add_argument("--material_metrics", type=str, default=None, metavar="GT_DIR", help="the split folder of a synthetic scene (Emit/, albedo/, DiffCol/, Roughness/): "
                        "every view's emission, a_prime, kd and roughness maps are scored against its ground truth on the device (utils/material_metrics.py), the "
                        "reference's utils/metric_brdf.py table is printed and written to <output_path>/<split>/material_metrics.json -- the numbers "
                        "python -m iris_amd.utils.metric_brdf computes from the files this run writes")
    return parser


def material_metrics_view(gt_dir, i, out, img_hw):
    """utils.material_metrics.material_metrics of render_view's maps `out` (the float32 maps, quantised in the kernel as save_png quantises them: no PNG is
    decoded) against view i of the ground-truth folder.  Nothing synchronises with the host."""
    from .utils import material_metrics as M
    gt = M.load_gt_view(gt_dir, i)
    if gt["emit"].shape[:2] != tuple(img_hw):
        raise L.IrisError(f"{gt_dir}: the ground-truth maps of view {i} are {gt['emit'].shape[0]} x {gt['emit'].shape[1]}, the view {img_hw[0]} x {img_hw[1]}")
    est = {"emit": out["emission"], "albedo": out["a_prime"], "kd": out["kd"], "rough": out["roughness"]}
    return M.material_metrics(M.upload([gt], out["emission"].device), {k: v.to(torch.float32) for k, v in est.items()})


def main(argv=None):
    from .model.emitter import SLFEmitter
    from .utils import cameras, stage
    from .utils.path_tracing import load_scene
    args = build_cli_parser().parse_args(argv)
    stage.refuse_textures_with_material(args)
    if args.light_type != "slf":
        raise L.IrisError("--light_type area (AreaEmitter, relighting) is not part of this stage: only slf")
    if args.material_metrics and not os.path.isdir(args.material_metrics):
        raise L.IrisError(f"--material_metrics {args.material_metrics}: no such folder")
    device = stage.open_device(args.device, "render")
    print("==========================\nExp: {}\nOutput: {}\nSplit: {}\n==========================".format(args.experiment_name, args.output_path, args.split))
    name, path = args.dataset
    mesh = stage.mesh_path(name, path, args.scene)
    scene = load_scene(mesh, device=device)
    img_hw, views = stage.load_views(name, path, args.scene, args.res_scale, split=args.split, cameras_json=args.cameras, extras=True)
    if args.max_views is not None:
        views = views[:args.max_views]

    ckpt = os.path.join(args.checkpoint_path, args.experiment_name, args.ckpt)
    if args.textures:
        material_net = stage.load_texture_material(args.textures, mesh, device)
    else:
        material_net = stage.load_material(args.material, os.path.join(args.emitter_path, "vslf.npz"), ckpt)    # NGPBRDF(mask['voxel_min'], mask['voxel_max']) + 'material.' (:110-119)
    if isinstance(material_net, torch.nn.Module):
        material_net.to(device)
    emitter_net = SLFEmitter(os.path.join(args.emitter_path, "emitter.pth"), os.path.join(args.emitter_path, "vslf_0.npz")).to(device)      # :123-124
    model_crf = stage.load_crf(stage.read_checkpoint(ckpt)["model_crf"], args.crf_basis, args.emor_path, device)                            # :130-135
    stage.freeze(material_net, emitter_net, model_crf)
    denoiser = stage.make_denoiser(args.denoise, img_hw, device)
    metrics = tuple(args.metrics.split(","))
    psnr_list, ssim_list = [], []
    table = None
    if args.material_metrics:
        from .utils import material_metrics as M
        table = M.Table(img_hw)
    t0 = time.time()
    for i, view in enumerate(views):
        stage.view_seed_torch(args.seed, i)
        rays = cameras.view_rays(view, img_hw, device, ray_diff=True)
        gt = stage.read_image(view["image"], img_hw) if view.get("image") else None
        out = render_view(scene, emitter_net, material_net, model_crf, rays, img_hw, args.SPP, args.spp, args.indir_depth, exposure=float(view.get("exposure", 1.0)),
                          gt=gt, denoise=denoiser is not None, denoiser=denoiser, metrics=metrics)
        write_view(args.output_path, args.split, i, out, args.compression)
        if table is not None:
            table.add(material_metrics_view(args.material_metrics, i, out, img_hw))
        if out["psnr"] is not None:
            psnr_list.append((i, out["psnr"]))
        if out["ssim"] is not None:
            ssim_list.append((i, out["ssim"]))
    if psnr_list:
        print("Mean PSNR: {:.5f}".format(float(np.mean([p for _, p in psnr_list]))))
    if ssim_list:
        print("Mean SSIM: {:.5f}".format(float(np.mean([s for _, s in ssim_list]))))
    if table is not None and views:
        from .utils.metric_brdf import write_json
        summary, doc = table.finish()
        print(M.format_summary(summary))
        write_json(os.path.join(args.output_path, args.split, "material_metrics.json"), dict(doc, gt=args.material_metrics))
    os.makedirs(os.path.join(args.output_path, args.split, "rgb"), exist_ok=True)
    write_metrics(os.path.join(args.output_path, args.split, "rgb", "metrics.txt"), psnr_list, ssim_list if "ssim" in metrics else None)
    torch.cuda.synchronize()
    print("[render] {} views: {:.2f} s".format(len(views), time.time() - t0))


if __name__ == "__main__":
    main()
