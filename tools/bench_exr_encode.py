#!/usr/bin/env python3
"""Device-side EXR deflate (utils/exr.zip_encode_torch, csrc/iris_deflate.h) on the 13 maps of 1080p bench views: the room of bench.py (synthetic room
seed 1, 1 M triangles, SLF H=256), cameras on its circle of 32, SPP 128 per lobe as bench.py bakes, denoised as the CLI writes them.  Per compression:
  * device encode time per view (HIP events around scanline_blocks_torch + zip_encode_torch, after a warm-up, over --reps passes of all baked views)
    and GB/s of predicted bytes;
  * total file bytes against host zlib on the same predicted blocks: level 4 (the host writer's default) and level 4 with the Z_RLE strategy (the parse the
    device encoder makes), each with OpenEXR's raw fallback.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.  One JSON line per compression.

    python tools/bench_exr_encode.py [--views 2] [--reps 40] [--spp 128]
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def bake_views(args, dev):
    """the 13 maps (R,G,B) of args.views bench views, as the CLI hands them to its writer"""
    from types import SimpleNamespace
    import bench
    from tools import synth
    from iris_amd import bake_shading as bs
    from iris_amd.utils.dataset import real_ldr
    from iris_amd.utils.denoise import Denoiser
    ns = SimpleNamespace(scene_seed=1, tris=args.tris, slf_res=256, layout=0, long_walls=False)
    _, _, _, scene, emitter = bench.build_workload(ns, dev)
    H, W = args.height, args.width
    den = Denoiser((W, H), dev)
    out = []
    for i in range(args.views):
        K, c2w = synth.camera(H, W, (i * 32) // args.views, n_views=32)
        xs, ds = real_ldr.to_world(real_ldr.get_direction(K, (H, W)), c2w, False, device=dev)
        r = bs.bake_view(scene, emitter, xs.reshape(-1, 3), ds.reshape(-1, 3), args.spp, [args.spp] * bs.N_ROUGHNESS, seed=bs.view_seed(0, i), image_width=W,
                         denoiser=den)
        out.append(torch.stack([r["diffuse"]] + [r[k][j] for j in range(bs.N_ROUGHNESS) for k in ("specular0", "specular1")]).reshape(13, H, W, 3))
    torch.cuda.synchronize()
    return out


def host_bytes(full, tail, level, strategy):
    """file data bytes host zlib would store for these predicted blocks (OpenEXR's rule: the stream, or the raw block when that is not shorter)"""
    n = 0
    for m in range(full.shape[0]):
        for p in [full[m, i].tobytes() for i in range(full.shape[1])] + ([tail[m].tobytes()] if tail.shape[1] else []):
            c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
            n += min(len(c.compress(p) + c.flush()), len(p))
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--reps", type=int, default=40, help="timed passes over the baked views")
    ap.add_argument("--spp", type=int, default=128)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--compressions", type=str, default="zip,zips")
    ap.add_argument("--no-host", action="store_true", help="skip the host zlib size comparison (a kernel-trace run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_exr_encode needs the GPU")
    from iris_amd.utils import exr
    dev = torch.device("cuda:0")
    t0 = time.time()
    views = bake_views(args, dev)
    print("# %d views baked in %.1f s" % (len(views), time.time() - t0), file=sys.stderr)
    for comp in args.compressions.split(","):
        def encode(maps):
            full, tail = exr.scanline_blocks_torch(maps, comp)
            return full, tail, exr.zip_encode_torch(full, tail, comp)
        for v in views:                                                  # warm-up: code objects, allocator
            encode(v)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        # the predictor alone (scanline_blocks_torch) is what the host path runs on the device too: timed separately, so the deflate's share is known
        p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        p0.record()
        for _ in range(args.reps):
            for v in views:
                exr.scanline_blocks_torch(v, comp)
        p1.record()
        e0.record()
        for _ in range(args.reps):
            for v in views:
                encode(v)
        e1.record()
        torch.cuda.synchronize()
        n = args.reps * len(views)
        ms = e0.elapsed_time(e1) / n
        ms_pred = p0.elapsed_time(p1) / n
        full, tail, (rec, offs) = encode(views[0])
        torch.cuda.synchronize()
        pred_bytes = full.numel() + tail.numel()
        dev_bytes = int(offs[-1]) - 8 * 13 * (full.shape[1] + (1 if tail.shape[1] else 0))
        res = {"compression": comp, "image": [args.width, args.height], "maps_per_view": 13, "spp": args.spp, "views": len(views), "timed_encodes": n,
               "predicted_bytes_per_view": pred_bytes,
               "device_ms_per_view": round(ms, 3), "device_predict_only_ms_per_view": round(ms_pred, 3), "device_deflate_ms_per_view": round(ms - ms_pred, 3),
               "GB_per_s_of_predicted_bytes": round(pred_bytes / (ms * 1e-3) / 1e9, 1), "device_data_bytes_view0": dev_bytes}
        if not args.no_host:
            hf, ht = full.cpu().numpy(), tail.cpu().numpy()
            h4 = host_bytes(hf, ht, 4, zlib.Z_DEFAULT_STRATEGY)
            hr = host_bytes(hf, ht, 4, zlib.Z_RLE)
            res.update({"host_level4_data_bytes_view0": h4, "host_zrle_data_bytes_view0": hr, "device_over_level4": round(dev_bytes / h4, 4),
                        "device_over_zrle": round(dev_bytes / hr, 4), "level4_ratio": round(h4 / pred_bytes, 4)})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
