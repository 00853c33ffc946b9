"""The relighting stage (reference: render_relight.py) on MI355X: the room's recovered materials under NEW lights.

    python -m iris_amd.render_relight --experiment_name EXP --ckpt last_1.ckpt --dataset synthetic DATA/kitchen --emitter_path checkpoints/EXP/bake
        --light_cfg configs/fipt/kitchen/relight_0.yaml --output_path OUT --SPP 256 --spp 16

The reference loads the light configuration into a Mitsuba scene and lets Mitsuba's `path` integrator call the material network per bounce.  Here the
configuration is parsed by utils.lights, the room mesh is composed with the inserted shapes and lights, and `utils.relight.path_tracing_relit` traces it with the
HIP stages of this package.  Per view: SPP // spp rounds at (h a, w a) pixels (a = --anti_aliasing), NaN -> 0, the mean, the a-trous denoiser guided by the
composed scene's primary hits, the camera response model at exposure 1, the a x a box average (cv2.INTER_AREA for an integer factor), and
{i:05d}_rgb.png (when PIL imports) + {i:05d}_rgb.exr (an addition) under --output_path.

--mode traj takes its views from the scene's render trajectory (utils.cameras.load_trajectory; --cameras, when given, replaces it) and also writes
relight.ffconcat: the frames forward and then reversed at 30 fps, the list `ffmpeg -f concat` turns into the reference's relight.mp4.  The trajectory's frames
are used as camera-to-world matrices directly: the reference's c2w[:, :2] *= -1 only adapts them to Mitsuba's look_at and describes the same camera.
With --video mjpeg (default none; --video_quality, default 90) it also writes relight.avi, a Motion-JPEG file of the same frames in the same order, the JPEG
frames encoded on the device (utils/jpeg.py, utils/avi.py; render_video.py does the same for its eight files).

Not here: relight.mp4 itself (no H.264 encoder), inserted obj / ply meshes, textures, environment maps, point lights.
"""
import os
import time

import numpy as np
import torch

from . import _lib as L
from .utils import lights as LT
from .utils.path_tracing import load_mesh, ray_intersect
from .utils.relight import RelitScene, path_tracing_relit

INDIR_DEPTH = 5


def scaled_view(view, a):
    """the view with its intrinsics scaled by the integer anti-aliasing factor `a` (render_relight.py:219-233)"""
    v = dict(view)
    if v["kind"] == "synthetic":
        v["focal"] = float(v["focal"]) * a
    else:
        K = np.asarray(v["K"], np.float32).copy()
        K[:2, :] *= a
        v["K"] = K
    return v


@torch.no_grad()
def relight_view(relit, material_net, model_crf, rays, img_hw, SPP, spp, indir_depth=INDIR_DEPTH, anti_aliasing=1, exposure=1.0, denoise=True, denoiser=None):
    """One iteration of the reference's per-view loop (render_relight.py:265-298).

    relit: the RelitScene of this view; rays: the four (H a * W a, 3) tensors (origin, direction, dxdu, dydv) of the view at the anti-aliased size, or one
    (.., 12) tensor; img_hw: the OUTPUT size (h, w).  SPP // spp rounds of path_tracing_relit(..., spp, max_depth = indir_depth + 2), NaN -> 0 per round, the mean,
    the denoiser (guides: the composed scene's pixel-centre primary hits), model_crf(L, exposure) (None: no LDR image), the a x a box average.
    Returns {'rgb_full' (h a, w a, 3) HDR (denoised), 'rgb_ldr' (h, w, 3) or None, 'rounds'}, device tensors."""
    a = int(anti_aliasing)
    if a < 1:
        raise L.IrisError(f"relight_view: anti_aliasing = {anti_aliasing} must be a positive integer")
    h, w = int(img_hw[0]), int(img_hw[1])
    H, W = h * a, w * a
    if isinstance(rays, (tuple, list)):
        rays_x, rays_d, dxdu, dydv = rays
    else:
        rays = L.require_gpu(rays, torch.float32, "rays").reshape(-1, 12)
        rays_x, rays_d, dxdu, dydv = (rays[:, 3 * k:3 * k + 3].contiguous() for k in range(4))
    rays_x = L.require_gpu(rays_x, torch.float32, "rays_x").reshape(-1, 3)
    B, dev = rays_x.shape[0], rays_x.device
    if B != H * W:
        raise L.IrisError(f"relight_view: {B} rays for an image of {H} x {W} ({h} x {w} at anti_aliasing {a})")
    rounds = int(SPP) // int(spp)
    if rounds < 1:
        raise L.IrisError(f"relight_view: SPP ({SPP}) // spp ({spp}) is zero: nothing would be rendered")
    img = torch.zeros(B, 3, device=dev)
    for _ in range(rounds):
        img_ = path_tracing_relit(relit, material_net, rays_x, rays_d, dxdu, dydv, spp, int(indir_depth) + 2)
        img_[img_.isnan()] = 0                                           # render_relight.py:283
        img += img_
    img = img / rounds
    if denoise:
        if denoiser is None:
            from .utils.denoise import Denoiser
            denoiser = Denoiser((W, H), dev)
        pos, nrm, _, _, valid = ray_intersect(relit.scene, rays_x, torch.nn.functional.normalize(L.require_gpu(rays_d, torch.float32, "rays_d").reshape(-1, 3), dim=-1))
        denoiser.set_guides(nrm, pos, valid)
        img = denoiser(img.reshape(H, W, 3)).reshape(B, 3)
    out = {"rgb_full": img.reshape(H, W, 3), "rgb_ldr": None, "rounds": rounds}
    if model_crf is not None:
        ldr = model_crf(img.contiguous(), exposure).detach().reshape(H, W, 3)
        if a > 1:
            ldr = torch.nn.functional.avg_pool2d(ldr.permute(2, 0, 1)[None], a)[0].permute(1, 2, 0).contiguous()
        out["rgb_ldr"] = ldr
    return out


def save_image(image, path):
    """render_relight.py:43-55 save_image without the colour map: clip to [0,1], * 255, uint8, odd trailing row / column dropped.  Written only when PIL imports."""
    try:
        from PIL import Image
    except ImportError:
        return False
    a = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    a = (np.clip(a, 0.0, 1.0) * 255).astype(np.uint8)
    hh, ww = a.shape[:2]
    Image.fromarray(a[:hh - hh % 2, :ww - ww % 2]).save(path)
    return True


def build_parser():
    """The reference's render_relight.py arguments (render_relight.py:117-131 + configs/config.py); the trainers' options are accepted and ignored."""
    import argparse
    from .utils import stage
    parser = argparse.ArgumentParser(description="python -m iris_amd.render_relight: the reference's render_relight.py on MI355X")
    parser.add_argument("--experiment_name", type=str, required=True)
    parser.add_argument("--mode", type=str, default="train_val", choices=["train_val", "traj"])
    parser.add_argument("--log_path", type=str, default="./logs")
    parser.add_argument("--checkpoint_path", type=str, default="./checkpoints")
    parser.add_argument("--output_path", type=str, default="outputs/kitchen_output")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--split", type=str, default="val")
    parser.add_argument("--ckpt", type=str, default="last.ckpt")
    parser.add_argument("--anti_aliasing", type=int, default=1)
    parser.add_argument("--light_cfg", type=str, required=True)
    parser.add_argument("--dataset", type=str, nargs=2, default=["synthetic", "../data/indoor_synthetic/kitchen"], help="dataset type (synthetic | real | scannetpp) and its path")
    parser.add_argument("--scene", type=str, default="")
    parser.add_argument("--emitter_path", type=str, required=True, help="folder holding vslf.npz and emitter.pth (render_relight.py:184-198)")
    parser.add_argument("--SPP", type=int, default=512)
    parser.add_argument("--spp", type=int, default=8)
    parser.add_argument("--indir_depth", type=int, default=INDIR_DEPTH)
    parser.add_argument("--crf_basis", type=int, default=3)
    parser.add_argument("--res_scale", type=float, default=1.0)
    parser.add_argument("--ldr_img_dir", type=str, default=None)
    stage.add_ignored_trainer_options(parser)
    # additions (defaults reproduce the reference)
    stage.add_common_options(parser, "material", "cameras", "emor_path", "denoise", "compression", "seed", "max_views",
                             cameras=stage.COMMON_OPTIONS["cameras"]["help"] + " (needed for --mode traj)")
    parser.add_argument("--keep_lights", type=float, default=0.0, help="0: the room's own lamps are switched off (absorbers); s > 0: they stay, their radiance times s")
    parser.add_argument("--sphere_subdiv", type=int, default=2, help="icosphere subdivisions of inserted spheres (2: 320 triangles)")
    return parser


def build_video_parser():
    """build_parser(), the two options of the video stage, --video and --video_quality, and --textures DIR: what main() parses.  They stand apart because
    build_parser()'s option table is pinned entry for entry (tests/test_stage_setup_cpu.py) as the table of the options this stage had before it could write a
    video or render from the exported textures."""
    from .utils import stage
    parser = build_parser()
    stage.add_common_options(parser, "video", "video_quality", "textures", video=stage.COMMON_OPTIONS["video"]["help"] + " (--mode traj: relight.avi beside relight.ffconcat)")
    return parser


def main(argv=None):
    from .utils import cameras, stage
    from .utils.exr import write_exr
    args = build_video_parser().parse_args(argv)
    stage.refuse_textures_with_material(args)
    name, path = args.dataset
    traj = None
    if args.mode == "traj" and not args.cameras:
        traj = stage.load_trajectory(name, path, args.scene, args.res_scale, split=args.split)          # (before the device: a missing trajectory ends here)
    device = stage.open_device(args.device, "render_relight")
    print("==========================\nExp: {}\nMode: {}\nOutput: {}\nSplit: {}\n==========================".format(args.experiment_name, args.mode, args.output_path, args.split))
    mesh = stage.mesh_path(name, path, args.scene)
    verts, faces = load_mesh(mesh)
    emitter_state = torch.load(os.path.join(args.emitter_path, "emitter.pth"), map_location="cpu")
    lights = LT.load_light_config(args.light_cfg)
    img_hw, views = traj or stage.load_views(name, path, args.scene, args.res_scale, split=args.split, cameras_json=args.cameras, extras=True)
    if args.max_views is not None:
        views = views[:args.max_views]
    ckpt = os.path.join(args.checkpoint_path, args.experiment_name, args.ckpt)
    if args.textures:                           # the material's own Scene of the ROOM mesh: the traced scene below has the inserted lights in it
        material_net = stage.load_texture_material(args.textures, mesh, device)
    else:
        material_net = stage.load_material(args.material, os.path.join(args.emitter_path, "vslf.npz"), ckpt)
    if isinstance(material_net, torch.nn.Module):
        material_net.to(device)
    model_crf = stage.load_crf(stage.read_checkpoint(ckpt)["model_crf"], args.crf_basis, args.emor_path, device)
    stage.freeze(material_net, model_crf)
    a = int(args.anti_aliasing)
    hw_aa = (img_hw[0] * a, img_hw[1] * a)
    denoiser = stage.make_denoiser(args.denoise, hw_aa, device)
    os.makedirs(args.output_path, exist_ok=True)
    relit, t0, frames, video = None, time.time(), [], None
    for i, view in enumerate(views):
        stage.view_seed_torch(args.seed, i)
        if relit is None or lights.disco is not None:                   # the scene is recomposed per view only for the disco ball (timestep = i)
            relit = RelitScene(LT.compose(verts, faces, emitter_state, lights.at(i), args.keep_lights, args.sphere_subdiv), device)
        rays = cameras.view_rays(scaled_view(view, a), hw_aa, device, ray_diff=True)
        out = relight_view(relit, material_net, model_crf, rays, img_hw, args.SPP, args.spp, args.indir_depth, anti_aliasing=a, exposure=1.0,
                           denoise=denoiser is not None, denoiser=denoiser)
        frames.append(os.path.join(args.output_path, "{:0>5d}_rgb.png".format(i)))
        written = save_image(out["rgb_ldr"], frames[-1])
        if args.mode == "traj" and args.video == "mjpeg":
            from .utils import avi, jpeg
            ldr = out["rgb_ldr"].detach()
            if video is None:
                video = avi.AviWriter(os.path.join(args.output_path, "relight.avi"), ldr.shape[1] - ldr.shape[1] % 2, ldr.shape[0] - ldr.shape[0] % 2, 30)
            video.add_frame(jpeg.encode_frames_device([ldr], quality=args.video_quality)[0])
        write_exr(os.path.join(args.output_path, "{:0>5d}_rgb.exr".format(i)), out["rgb_full"].detach().cpu().numpy(), args.compression)
    if args.mode == "traj" and frames and written:
        stage.write_ffconcat(os.path.join(args.output_path, "relight.ffconcat"), frames)                # (render_relight.py:300-303: imgs += imgs[::-1], fps 30)
    if video is not None:
        video.close(reverse=True)
    torch.cuda.synchronize()
    print("[render_relight] {} views: {:.2f} s".format(len(views), time.time() - t0))


if __name__ == "__main__":
    main()
