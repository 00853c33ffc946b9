"""The video stage (reference: render_video.py) on MI355X: the frames of the scene's render trajectory, eight 8-bit PNG files per frame.

    python -m iris_amd.render_video --experiment_name EXP --ckpt last_1.ckpt --dataset synthetic DATA/kitchen --emitter_path checkpoints/EXP/bake
        --output_path OUT --split val --SPP 256 --spp 16 --crf_basis 3

Per frame i of render_traj.npy (utils.cameras.load_trajectory: the datasets' load_traj=True): `render.render_view` at exposure 1 -- the path-traced image, denoised
and mapped to LDR by the camera response model, and the intrinsics averaged over the same SPP // spp rounds --, then under --output_path
    rgb/{i:05d}_rgb_full.png   diffuse/{i:05d}_kd.png   a_prime/{i:05d}_a_prime.png   emission/{i:05d}_emission.png (emission / 10)
    roughness/{i:05d}_roughness.png, _roughness_color.png   metallic/{i:05d}_metallic.png, _metallic_color.png      (grey, and through the MAGMA colour map)
each clipped to [0,1], times 255, truncated to 8 bits, an odd trailing row / column dropped (the reference's save_image).

The PNG files are made on the device by default (--png_encoder device, utils/png.py: quantiser, colour map, crop and Sub filter in one launch per group of
equal-size maps, the EXR writer's deflate kernels in zlib-stream mode, one device-to-host copy); FrameWriter overlaps that copy, the CRC and the file writes of
frame i with the render of frame i + 1.  --png_encoder host quantises in numpy and compresses with zlib on writer threads.  Both decode to the same pixels.

The videos are made with --video mjpeg: eight Motion-JPEG files <output_path>/<name>.avi (rgb_full, kd, a_prime, roughness, roughness_color, metallic,
metallic_color, emission) where the reference's <name>.mp4 stand -- the frames forward and then reversed at 30 fps, as the reference's imgs += imgs[::-1] and
mimsave(fps=30).  Each frame is a baseline JPEG of exactly the pixels of the frame's PNG file, encoded on the device (utils/jpeg.py, --video_quality, default
90) and appended to its file as it arrives (utils/avi.py); ffmpeg, VLC and mpv play them.  The default, --video none, writes none of them.  Either way the
stage writes eight lists, <output_path>/<name>.ffconcat, of the PNG frames in the same order: `ffmpeg -f concat -i rgb_full.ffconcat -pix_fmt yuv420p
rgb_full.mp4` produces the reference's H.264 video on any machine that has ffmpeg (there is no H.264 encoder here).
Not here either: --light_type area (AreaEmitter), as in the render stage.
"""
import os
import time

import torch

from . import _lib as L
from .render import INDIR_DEPTH, render_view

# (folder, file name, key of render_view's dict, divisor, magma)
FRAME_FILES = (("rgb", "rgb_full", "rgb_ldr", 1.0, False), ("diffuse", "kd", "kd", 1.0, False), ("a_prime", "a_prime", "a_prime", 1.0, False),
               ("roughness", "roughness", "roughness", 1.0, False), ("roughness", "roughness_color", "roughness", 1.0, True),
               ("metallic", "metallic", "metallic", 1.0, False), ("metallic", "metallic_color", "metallic", 1.0, True),
               ("emission", "emission", "emission", 10.0, False))
FPS = 30


def frame_paths(output_path, i):
    """the eight files of frame i, in FRAME_FILES order"""
    return [os.path.join(output_path, folder, "{:0>5d}_{}.png".format(i, name)) for folder, name, _, _, _ in FRAME_FILES]


class FrameWriter:
    """A frame's eight maps -> eight PNG files, off the critical path.  encoder "device": submit() enqueues utils.png.enqueue_frames_device and one
    device-to-host copy into a pinned buffer on a side stream and returns; a writer thread waits for the copy's event, wraps the streams (CRC-32) and writes.
    encoder "host": submit() enqueues the copy of the float maps; the writer threads quantise (utils.png.quantize_host) and compress (zlib level 1).
    Two buffer sets: a third frame waits for the first one's files.  Files appear under their final name only when complete.
    video "mjpeg": submit() also enqueues utils.jpeg.enqueue_frames_device and the copy of the stream offsets on the side stream; ONE video thread (frames
    enter a file in order) waits for that copy, enqueues the copy of exactly the used bytes, waits for it and appends the eight JPEG files to
    <output_path>/<name>.avi (utils.avi.AviWriter); close() finishes the eight files."""

    def __init__(self, device, encoder="device", n_buffers=2, level=1, video="none", video_quality=90):
        from concurrent.futures import ThreadPoolExecutor
        if encoder not in ("host", "device"):
            raise L.IrisError(f"FrameWriter: encoder {encoder!r} is not 'host' or 'device'")
        if video not in ("none", "mjpeg"):
            raise L.IrisError(f"FrameWriter: video {video!r} is not 'none' or 'mjpeg'")
        self.video, self.video_quality, self.device = video, video_quality, device
        if video == "mjpeg":
            self.video_pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="video")
            self.video_busy, self.video_heads, self.video_data, self.avis = [None] * n_buffers, [None] * n_buffers, None, None
        self.encoder, self.level, self.n_buffers = encoder, level, n_buffers
        self.stream = torch.cuda.Stream(device=device)
        self.bufs = [None] * n_buffers
        self.busy = [[] for _ in range(n_buffers)]
        self.pool = ThreadPoolExecutor(max_workers=min(len(FRAME_FILES), 16), thread_name_prefix="frames")
        self.k = 0

    def _to_host(self, slot, tensors):
        """one pinned buffer per tensor of this slot (sized at first use, regrown when a frame needs more), the copies on the side stream -> (arrays, event)"""
        if self.bufs[slot] is None or len(self.bufs[slot]) != len(tensors) or any(b.numel() < t.numel() or b.dtype != t.dtype for b, t in zip(self.bufs[slot], tensors)):
            self.bufs[slot] = [torch.empty(t.numel(), dtype=t.dtype).pin_memory() for t in tensors]
        ready = torch.cuda.Event(); ready.record()
        done = torch.cuda.Event()
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            for b, t in zip(self.bufs[slot], tensors):
                b[:t.numel()].copy_(t.reshape(-1), non_blocking=True)
                t.record_stream(self.stream)
            done.record(self.stream)
        return [b[:t.numel()].numpy().reshape(tuple(t.shape)) for b, t in zip(self.bufs[slot], tensors)], done

    def submit(self, output_path, i, out):
        """out: render_view's dict (device tensors, produced on the current stream) -> the eight files of frame i; returns their paths"""
        from .utils import png
        paths = frame_paths(output_path, i)
        for p in paths:
            os.makedirs(os.path.dirname(p), exist_ok=True)
        if out.get("rgb_ldr") is None:
            raise L.IrisError("render_video: the frame has no LDR image (render_view was called without a response model)")
        slot = self.k % self.n_buffers; self.k += 1
        for f in self.busy[slot]:
            f.result()                                      # this buffer's previous files are on disk (re-raises a writer's exception)

        def replace(path, data):
            with open(path + ".part", "wb") as fh:
                fh.write(data)
            os.replace(path + ".part", path)
        if self.encoder == "device":
            buf, layout = png.enqueue_frames_device([out[key] for _, _, key, _, _ in FRAME_FILES], [d for _, _, _, d, _ in FRAME_FILES], [m for _, _, _, _, m in FRAME_FILES])
            (host,), done = self._to_host(slot, [buf])

            def write(path, j):
                done.synchronize()
                replace(path, png.png_container(*png.streams_from_host(host, layout, len(paths))[j]))      # (the CRC-32 of a large buffer runs without the GIL)
            self.busy[slot] = [self.pool.submit(write, p, j) for j, p in enumerate(paths)]
        else:
            keys = sorted({key for _, _, key, _, _ in FRAME_FILES})
            arrays, done = self._to_host(slot, [out[k].contiguous() for k in keys])
            maps = dict(zip(keys, arrays))

            def write(path, key, divisor, magma):
                done.synchronize()
                replace(path, png.encode_png_host(png.quantize_host(maps[key], divisor, magma), self.level))
            self.busy[slot] = [self.pool.submit(write, p, key, d, m) for p, (_, _, key, d, m) in zip(paths, FRAME_FILES)]
        if self.video == "mjpeg":
            self._submit_video(output_path, slot, out)
        return paths

    def _submit_video(self, output_path, slot, out):
        from .utils import avi, jpeg
        if self.video_busy[slot] is not None:
            self.video_busy[slot].result()                  # this slot's offsets buffer is free again (re-raises the video thread's exception)
        buf, layout = jpeg.enqueue_frames_device([out[key] for _, _, key, _, _ in FRAME_FILES], [d for _, _, _, d, _ in FRAME_FILES], [m for _, _, _, _, m in FRAME_FILES],
                                                 self.video_quality)
        if self.avis is None:
            sizes = {i: (g["width"], g["height"]) for g in layout["groups"] for i in g["indices"]}
            self.avis = [avi.AviWriter(os.path.join(output_path, name + ".avi"), *sizes[k], FPS) for k, (_, name, _, _, _) in enumerate(FRAME_FILES)]
        if self.video_heads[slot] is None or self.video_heads[slot].numel() < layout["head"]:
            self.video_heads[slot] = torch.empty(layout["head"], dtype=torch.uint8).pin_memory()
        head = self.video_heads[slot][:layout["head"]]
        ready = torch.cuda.Event(); ready.record()
        head_done = torch.cuda.Event()
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            head.copy_(buf[:layout["head"]], non_blocking=True)
            buf.record_stream(self.stream)
            head_done.record(self.stream)

        def append():
            head_done.synchronize()
            sizes = jpeg.group_sizes(head.numpy(), layout)
            if self.video_data is None or self.video_data.numel() < sum(sizes):
                self.video_data = torch.empty(sum(sizes), dtype=torch.uint8).pin_memory()
            data, o = [], 0
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):      # (after the offsets' copy on that stream, so after the encoder)
                for g, size in zip(layout["groups"], sizes):
                    data.append(self.video_data[o:o + size])
                    data[-1].copy_(buf[g["pos"]:g["pos"] + size], non_blocking=True)
                    o += size
                done = torch.cuda.Event(); done.record(self.stream)
            done.synchronize()
            for w, f in zip(self.avis, jpeg.files_from_host(head.numpy(), [d.numpy() for d in data], layout, len(FRAME_FILES))):
                w.add_frame(f)
        self.video_busy[slot] = self.video_pool.submit(append)

    def close(self):
        for fs in self.busy:
            for f in fs:
                f.result()
        self.busy = [[] for _ in range(self.n_buffers)]
        self.pool.shutdown()
        if self.video == "mjpeg":
            busy, self.video_busy = self.video_busy, [None] * self.n_buffers
            for f in busy:
                if f is not None:
                    f.result()
            self.video_pool.shutdown()
            avis, self.avis = self.avis or [], None
            for w in avis:
                w.close(reverse=True)


def write_lists(output_path, n_frames):
    """<output_path>/<name>.ffconcat for the eight file kinds (what stands where rgb_full.mp4 ... emission.mp4 stand); returns their paths"""
    from .utils import stage
    lists = []
    for k, (_, name, _, _, _) in enumerate(FRAME_FILES):
        lists.append(os.path.join(output_path, name + ".ffconcat"))
        stage.write_ffconcat(lists[-1], [frame_paths(output_path, i)[k] for i in range(n_frames)], FPS)
    return lists


def build_parser():
    """The reference's render_video.py arguments (render_video.py:58-72 + configs/config.py) that matter here; the trainers' options are accepted and ignored."""
    import argparse
    from .utils import stage
    parser = argparse.ArgumentParser(description="python -m iris_amd.render_video: the reference's render_video.py on MI355X")
    parser.add_argument("--experiment_name", type=str, required=True)
    parser.add_argument("--log_path", type=str, default="./logs")
    parser.add_argument("--checkpoint_path", type=str, default="./checkpoints")
    parser.add_argument("--output_path", type=str, default="outputs/kitchen_output")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--split", type=str, default="val")
    parser.add_argument("--ckpt", type=str, default="last.ckpt")
    parser.add_argument("--light_type", type=str, default="slf", choices=["slf", "area"])
    parser.add_argument("--dataset", type=str, nargs=2, default=["synthetic", "../data/indoor_synthetic/kitchen"], help="dataset type (synthetic | real | scannetpp) and its path")
    parser.add_argument("--scene", type=str, default="")
    parser.add_argument("--emitter_path", type=str, required=True, help="folder holding vslf.npz, emitter.pth and vslf_0.npz (render_video.py:126-141)")
    parser.add_argument("--SPP", type=int, default=512)
    parser.add_argument("--spp", type=int, default=8)
    parser.add_argument("--indir_depth", type=int, default=INDIR_DEPTH)
    parser.add_argument("--crf_basis", type=int, default=3)
    parser.add_argument("--res_scale", type=float, default=1.0)
    parser.add_argument("--ldr_img_dir", type=str, default=None)
    stage.add_ignored_trainer_options(parser)
    # additions (defaults reproduce the reference)
    stage.add_common_options(parser, "material", "emor_path", "denoise", "seed", "max_views", max_views="render only the first N frames of the trajectory")
    parser.add_argument("--png_encoder", type=str, default="device", choices=["device", "host"], help="where the eight PNG files of a frame are encoded: on the GPU "
                        "(default; larger files, matches at distance 1 only) or with zlib on host threads; both decode to the same pixels")
    stage.add_common_options(parser, "video", "video_quality", "textures")
    return parser


def main(argv=None):
    from .model.emitter import SLFEmitter
    from .utils import cameras, stage
    from .utils.path_tracing import load_scene
    args = build_parser().parse_args(argv)
    stage.refuse_textures_with_material(args)
    if args.light_type != "slf":
        raise L.IrisError("--light_type area (AreaEmitter, relighting) is not part of this stage: only slf")
    name, path = args.dataset
    img_hw, views = stage.load_trajectory(name, path, args.scene, args.res_scale, split=args.split)      # (before the device: a missing trajectory ends here)
    if args.max_views is not None:
        views = views[:args.max_views]
    device = stage.open_device(args.device, "render_video")
    print("==========================\nExp: {}\nOutput: {}\nFrames: {}\n==========================".format(args.experiment_name, args.output_path, len(views)))
    mesh = stage.mesh_path(name, path, args.scene)
    scene = load_scene(mesh, device=device)
    ckpt = os.path.join(args.checkpoint_path, args.experiment_name, args.ckpt)
    if args.textures:
        material_net = stage.load_texture_material(args.textures, mesh, device)
    else:
        material_net = stage.load_material(args.material, os.path.join(args.emitter_path, "vslf.npz"), ckpt)
    if isinstance(material_net, torch.nn.Module):
        material_net.to(device)
    emitter_net = SLFEmitter(os.path.join(args.emitter_path, "emitter.pth"), os.path.join(args.emitter_path, "vslf_0.npz")).to(device)
    model_crf = stage.load_crf(stage.read_checkpoint(ckpt)["model_crf"], args.crf_basis, args.emor_path, device)
    stage.freeze(material_net, emitter_net, model_crf)
    denoiser = stage.make_denoiser(args.denoise, img_hw, device)
    writer = FrameWriter(device, args.png_encoder, video=args.video, video_quality=args.video_quality)
    t0 = time.time()
    try:
        for i, view in enumerate(views):
            stage.view_seed_torch(args.seed, i)
            rays = cameras.view_rays(view, img_hw, device, ray_diff=True)
            out = render_view(scene, emitter_net, material_net, model_crf, rays, img_hw, args.SPP, args.spp, args.indir_depth, exposure=1.0, gt=None,
                              denoise=denoiser is not None, denoiser=denoiser)
            writer.submit(args.output_path, i, out)
    finally:
        writer.close()
    write_lists(args.output_path, len(views))
    torch.cuda.synchronize()
    print("[render_video] {} frames: {:.2f} s".format(len(views), time.time() - t0))


if __name__ == "__main__":
    main()
