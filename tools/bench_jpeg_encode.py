#!/usr/bin/env python3
"""What the eight JPEG files of one 1080p video frame cost, on the maps of one `render_view` of the bench scene (the room of bench.py: seed 1,
1 M triangles, SLF H = 256; material = NGPBRDF with random parameters; the response model is a gamma curve with a small EMoR-like basis), as
tools/bench_png_encode.py does for the PNG files.  Everything in ONE process, arms interleaved, after a warm-up of each:
  jpeg_device utils.jpeg.enqueue_frames_device, the copy of the offsets, the copy of the used bytes (pinned buffers), the headers: HIP events around the
              encoder and around each copy, a host clock around the headers and around the whole arm (it ends in a synchronise)
  png_device  the device PNG path of the same frame (utils.png), measured here, in the same process
  pil_1       utils.png.quantize_host + PIL's JPEG encoder at the same tables (qtables=quant_tables(q), 4:2:0, optimize=False), one thread: a host encoder's cost
  pil_16      the same eight files in a pool of 16 threads
The host arms start from the float maps in pinned host memory; that copy is timed on its own (maps_copy_ms) and belongs to each of them.
The encoder's own stages -- transform, entropy, compaction (assemble, offsets, emit) -- are kernels of one library call: their times come from a
`rocprofv3 --kernel-trace --stats` run of `--only_device N` (a run of its own), whose kernel_stats CSV a second run folds in with --kernel_stats.
Writes profiles/jpeg_encode_1080p.json and prints it as one JSON line.  Needs the GPU; nothing is estimated: a figure that was not taken is null."""
import argparse
import csv
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

STAGES = {"transform": ("jpeg_transform_kernel",), "entropy": ("jpeg_entropy_kernel",), "compaction": ("jpeg_assemble_kernel", "zip_offsets_kernel", "jpeg_emit_kernel")}


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def kernel_stages(path, calls_per_frame):
    """rocprofv3's kernel_stats CSV -> ms per frame of each stage: total time of the stage's kernels over the frames traced (a frame is calls_per_frame
    iris_jpeg_encode calls, one jpeg_entropy_kernel each); zip_offsets_kernel only counts in a --only_device run, where nothing else launches it"""
    rows = {r["Name"]: r for r in csv.DictReader(open(path))}
    frames = sum(int(r["Calls"]) for n, r in rows.items() if "jpeg_entropy_kernel" in n) / calls_per_frame
    return {s: round(sum(int(r["TotalDurationNs"]) for n, r in rows.items() if any(k in n for k in ks)) / frames * 1e-6, 4) for s, ks in STAGES.items()}, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16); ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--height", type=int, default=1080); ap.add_argument("--width", type=int, default=1920); ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--repeats", type=int, default=7, help="timed passes of the device arms"); ap.add_argument("--pil_repeats", type=int, default=3)
    ap.add_argument("--only_device", type=int, default=0, help="N > 0: after the warm-up run the jpeg_device arm N times and stop (the run to put under rocprofv3)")
    ap.add_argument("--kernel_stats", type=str, default=None, help="kernel_stats CSV of a rocprofv3 --kernel-trace --stats run of --only_device")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "jpeg_encode_1080p.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_encode needs the GPU")
    from PIL import Image
    import bench
    from iris_amd import _lib as L
    from iris_amd import render_video as RV
    from iris_amd.model.crf import EmorCRF
    from iris_amd.render import render_view
    from iris_amd.utils import jpeg, png
    from iris_amd.utils.dataset import real_ldr
    from iris_amd.utils.denoise import Denoiser
    from tools import synth
    from tools.bench_pt_single import ngp_material
    dev = torch.device("cuda:0")
    t0 = time.time()
    _, slf, _, scene, emitter = bench.build_workload(SimpleNamespace(scene_seed=1, tris=args.tris, slf_res=256, layout=0, long_walls=False), dev)
    emitter = emitter.to(dev) if hasattr(emitter, "to") else emitter
    H, W = args.height, args.width
    s = torch.linspace(0, 1, 1024)
    crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (k + 1)) * 0.05 for k in range(3)])).to(dev)
    K, c2w = synth.camera(H, W, 0, n_views=32)
    rays = real_ldr.to_world(real_ldr.get_direction(K, (H, W)), c2w, True, K, device=dev)
    out = render_view(scene, emitter, ngp_material(slf, dev), crf, rays, (H, W), args.spp, args.spp, denoiser=Denoiser((W, H), dev))
    torch.cuda.synchronize()
    print("# workload and one round in %.1f s" % (time.time() - t0), file=sys.stderr, flush=True)
    images = [out[key] for _, _, key, _, _ in RV.FRAME_FILES]
    divisors = [d for _, _, _, d, _ in RV.FRAME_FILES]
    magma = [m for _, _, _, _, m in RV.FRAME_FILES]
    names = [n for _, n, _, _, _ in RV.FRAME_FILES]
    qt = jpeg.quant_tables(args.quality)
    pinned = {}

    def events(n):
        return [torch.cuda.Event(enable_timing=True) for _ in range(n)]

    def jpeg_arm():
        t = time.perf_counter()
        e = events(5)
        e[0].record()
        buf, layout = jpeg.enqueue_frames_device(images, divisors, magma, args.quality)
        e[1].record()
        if "head" not in pinned:
            pinned["head"] = torch.empty(layout["head"], dtype=torch.uint8).pin_memory()
        pinned["head"].copy_(buf[:layout["head"]], non_blocking=True)
        e[2].record()
        e[2].synchronize()
        sizes = jpeg.group_sizes(pinned["head"].numpy(), layout)
        if "data" not in pinned or pinned["data"].numel() < sum(sizes):
            pinned["data"] = torch.empty(sum(sizes) * 5 // 4, dtype=torch.uint8).pin_memory()
        data, o = [], 0
        e[3].record()
        for g, size in zip(layout["groups"], sizes):
            data.append(pinned["data"][o:o + size])
            data[-1].copy_(buf[g["pos"]:g["pos"] + size], non_blocking=True)
            o += size
        e[4].record()
        torch.cuda.synchronize()
        t_dev = time.perf_counter()
        files = jpeg.files_from_host(pinned["head"].numpy(), [d.numpy() for d in data], layout, len(images))
        t_end = time.perf_counter()
        return files, {"encode_ms": e[0].elapsed_time(e[1]), "offsets_copy_ms": e[1].elapsed_time(e[2]), "data_copy_ms": e[3].elapsed_time(e[4]), "copy_bytes": sum(sizes),
                       "worst_case_bytes": buf.numel(), "headers_ms": (t_end - t_dev) * 1e3, "wall_ms": (t_end - t) * 1e3}

    def png_arm():
        t = time.perf_counter()
        e = events(3)
        e[0].record()
        buf, layout = png.enqueue_frames_device(images, divisors, magma)
        e[1].record()
        if "png" not in pinned:
            pinned["png"] = torch.empty(buf.numel(), dtype=torch.uint8).pin_memory()
        pinned["png"].copy_(buf, non_blocking=True)
        e[2].record()
        torch.cuda.synchronize()
        t_dev = time.perf_counter()
        files = png.files_from_host(pinned["png"].numpy(), layout, len(images))
        t_end = time.perf_counter()
        return files, {"encode_ms": e[0].elapsed_time(e[1]), "copy_ms": e[1].elapsed_time(e[2]), "copy_bytes": buf.numel(), "containers_ms": (t_end - t_dev) * 1e3,
                       "wall_ms": (t_end - t) * 1e3}

    def maps_to_host():
        keys = sorted({key for _, _, key, _, _ in RV.FRAME_FILES})
        if "maps" not in pinned:
            pinned["maps"] = {k: torch.empty(out[k].shape, dtype=out[k].dtype).pin_memory() for k in keys}
        e = events(2)
        e[0].record()
        for k in keys:
            pinned["maps"][k].copy_(out[k], non_blocking=True)
        e[1].record()
        torch.cuda.synchronize()
        return {k: pinned["maps"][k].numpy() for k in keys}, e[0].elapsed_time(e[1])

    def pil_file(maps, j):
        _, _, key, d, m = RV.FRAME_FILES[j]
        px = png.quantize_host(maps[key], d, m)
        b = io.BytesIO()
        Image.fromarray(px if px.ndim == 3 else np.repeat(px[..., None], 3, 2)).save(b, format="JPEG", qtables=qt, subsampling=2, optimize=False)
        return b.getvalue()

    pool = ThreadPoolExecutor(max_workers=16)

    def pil_arm(threads):
        maps, copy_ms = maps_to_host()
        t = time.perf_counter()
        files = list(pool.map(lambda j: pil_file(maps, j), range(8))) if threads > 1 else [pil_file(maps, j) for j in range(8)]
        return files, {"maps_copy_ms": copy_ms, "encode_ms": (time.perf_counter() - t) * 1e3}

    if args.only_device:
        jpeg_arm()
        for _ in range(args.only_device):
            jpeg_arm()
        print(json.dumps({"only_device": args.only_device, "frames_including_warm_up": args.only_device + 1}))
        return
    arms = {"jpeg_device": jpeg_arm, "png_device": png_arm, "pil_1": lambda: pil_arm(1), "pil_16": lambda: pil_arm(16)}
    files, rows = {}, {k: [] for k in arms}
    for k, fn in arms.items():                                             # warm-up: code objects, pinned buffers, the allocator's blocks, the pool's threads
        files[k], _ = fn()
    for r in range(args.repeats):                                          # interleaved
        for k, fn in arms.items():
            if k.startswith("pil") and r >= args.pil_repeats:
                continue
            rows[k].append(fn()[1])

    def decoded(f):
        return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"), np.float64)
    px = [decoded(f) for f in files["png_device"]]                         # the coded pixels: the PNG files are lossless

    def psnr(a, b):
        mse = np.mean((a - b) ** 2)
        return None if mse == 0 else round(float(10 * np.log10(255.0 ** 2 / mse)), 2)
    res = {"case": f"the eight JPEG files (quality {args.quality}) of one {W} x {H} frame of the bench room ({args.tris} triangles), maps of one render_view round at spp {args.spp}",
           "files": names, "arms": {}}
    for k in arms:
        med = {f: round(median([r[f] for r in rows[k]]), 3) for f in rows[k][0]}
        med["passes"] = len(rows[k])
        med["bytes_per_file"] = [len(f) for f in files[k]]
        med["total_bytes"] = sum(len(f) for f in files[k])
        med["ms_per_frame"] = round(med["wall_ms"] if k.endswith("device") else med["maps_copy_ms"] + med["encode_ms"], 3)
        if k != "png_device":
            med["psnr_db_per_file"] = [psnr(decoded(f), p) for f, p in zip(files[k], px)]
        res["arms"][k] = med
    res["jpeg_device_bytes_over_pil"] = [round(a / b, 4) for a, b in zip(res["arms"]["jpeg_device"]["bytes_per_file"], res["arms"]["pil_1"]["bytes_per_file"])]
    dev_arm = res["arms"]["jpeg_device"]
    res["stages_ms"] = {"transform": None, "entropy": None, "compaction": None, "device_total": dev_arm["encode_ms"],
                        "copies": round(dev_arm["offsets_copy_ms"] + dev_arm["data_copy_ms"], 3), "host_headers": dev_arm["headers_ms"]}
    if args.kernel_stats:
        groups = len({(tuple(t.shape[:2]), t.shape[2] if t.dim() == 3 else 1, t.dtype) for t in images})
        stages, frames = kernel_stages(args.kernel_stats, groups)
        res["stages_ms"].update(stages)
        res["stages_ms"]["kernel_times_from"] = f"rocprofv3 --kernel-trace --stats over {frames:g} frames of --only_device (a run of its own)"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
