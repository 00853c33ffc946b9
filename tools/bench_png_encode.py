#!/usr/bin/env python3
"""What the eight PNG files of one 1080p video frame cost, encoder by encoder, on the maps of one `render_view` of the bench scene (the room of
bench.py: seed 1, 1 M triangles, SLF H = 256; material = NGPBRDF with random parameters; the response model is a gamma curve with a small EMoR-like basis).
Everything in ONE process, arms interleaved, after a warm-up of each:
  device      utils.png.enqueue_frames_device + one copy into a pinned buffer + the containers (CRC-32): HIP events per stage (rows / deflate / copy), a host
              clock around the whole arm (ends in a synchronise)
  pil_1       utils.png.quantize_host + PIL's Image.save at its default level, one thread: what the reference calls
  pil_16      the same eight files in a pool of 16 threads
  host_1      utils.png.quantize_host + encode_png_host(level 1), one thread
  host_pool   the same in a pool of 16 threads (what --png_encoder host runs)
The host arms start from the float maps in pinned host memory; that copy is timed on its own (maps_copy_ms) and belongs to each of them.
Then `render_view` itself at --SPP / --spp (256 / 16 as scripts/*/render.sh) and the stage's own loop -- render_view + FrameWriter.submit per frame, both encoders
-- at ONE round per frame (SPP = spp: the case in which the writer has the least render time to hide behind).
Writes profiles/png_encode_1080p.json and prints it as one JSON line.  Needs the GPU; nothing is estimated: a figure that was not taken is null."""
import argparse
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


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--SPP", type=int, default=256); ap.add_argument("--spp", type=int, default=16); ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--height", type=int, default=1080); ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--repeats", type=int, default=5, help="timed passes of the device and host arms"); ap.add_argument("--pil_repeats", type=int, default=2)
    ap.add_argument("--frames", type=int, default=6, help="frames of the stage loop per encoder")
    ap.add_argument("--full_view_limit_s", type=float, default=150.0, help="render_view at --SPP is run only if one round times --SPP // --spp stays below this")
    ap.add_argument("--out", type=str, default=os.path.join(REPO, "profiles", "png_encode_1080p.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_encode needs the GPU")
    import tempfile
    from PIL import Image
    import bench
    from iris_amd import _lib as L
    from iris_amd import render_video as RV
    from iris_amd.model.crf import EmorCRF
    from iris_amd.render import render_view
    from iris_amd.utils import png
    from iris_amd.utils.dataset import real_ldr
    from iris_amd.utils.denoise import Denoiser
    from tools import synth
    from tools.bench_pt_single import ngp_material
    dev = torch.device("cuda:0")
    t0 = time.time()
    _, slf, _, scene, emitter = bench.build_workload(SimpleNamespace(scene_seed=1, tris=args.tris, slf_res=256, layout=0, long_walls=False), dev)
    emitter = emitter.to(dev) if hasattr(emitter, "to") else emitter
    H, W = args.height, args.width
    net = ngp_material(slf, dev)
    s = torch.linspace(0, 1, 1024)
    crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (k + 1)) * 0.05 for k in range(3)])).to(dev)
    den = Denoiser((W, H), dev)

    def rays_of(i):
        K, c2w = synth.camera(H, W, i % 32, n_views=32)
        return real_ldr.to_world(real_ldr.get_direction(K, (H, W)), c2w, True, K, device=dev)

    def view(i, SPP):
        return render_view(scene, emitter, net, crf, rays_of(i), (H, W), SPP, args.spp, denoiser=den)
    out = view(0, args.spp)
    torch.cuda.synchronize()
    print("# workload and one round in %.1f s" % (time.time() - t0), file=sys.stderr, flush=True)
    images = [out[key] for _, _, key, _, _ in RV.FRAME_FILES]
    divisors = [d for _, _, _, d, _ in RV.FRAME_FILES]
    magma = [m for _, _, _, _, m in RV.FRAME_FILES]
    names = [n for _, n, _, _, _ in RV.FRAME_FILES]

    # ---- arms
    pinned = {}

    def device_arm():
        t = time.perf_counter()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        with L.StageTimer() as tm:
            buf, layout = png.enqueue_frames_device(images, divisors, magma)
        if "buf" not in pinned:
            pinned["buf"] = torch.empty(buf.numel(), dtype=torch.uint8).pin_memory()
        e[0].record()
        pinned["buf"].copy_(buf, non_blocking=True)
        e[1].record()
        torch.cuda.synchronize()
        t_dev = time.perf_counter()
        files = png.files_from_host(pinned["buf"].numpy(), layout, len(images))
        t_end = time.perf_counter()
        st = tm.ms()
        return files, {"rows_ms": st.get("png rows", 0.0), "deflate_ms": st.get("png deflate", 0.0), "copy_ms": e[0].elapsed_time(e[1]), "copy_bytes": buf.numel(),
                       "containers_ms": (t_end - t_dev) * 1e3, "wall_ms": (t_end - t) * 1e3}

    def maps_to_host():
        keys = sorted({key for _, _, key, _, _ in RV.FRAME_FILES})
        if "maps" not in pinned:
            pinned["maps"] = {k: torch.empty(out[k].shape, dtype=out[k].dtype).pin_memory() for k in keys}
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        for k in keys:
            pinned["maps"][k].copy_(out[k], non_blocking=True)
        e[1].record()
        torch.cuda.synchronize()
        return {k: pinned["maps"][k].numpy() for k in keys}, e[0].elapsed_time(e[1])

    def pil_file(maps, j):
        _, _, key, d, m = RV.FRAME_FILES[j]
        b = io.BytesIO()
        Image.fromarray(png.quantize_host(maps[key], d, m)).save(b, format="PNG")
        return b.getvalue()

    def host_file(maps, j):
        _, _, key, d, m = RV.FRAME_FILES[j]
        return png.encode_png_host(png.quantize_host(maps[key], d, m), 1)

    pool = ThreadPoolExecutor(max_workers=16)

    def host_arm(fn, threads):
        maps, copy_ms = maps_to_host()
        t = time.perf_counter()
        files = list(pool.map(lambda j: fn(maps, j), range(8))) if threads > 1 else [fn(maps, j) for j in range(8)]
        return files, {"maps_copy_ms": copy_ms, "encode_ms": (time.perf_counter() - t) * 1e3}

    arms = {"device": device_arm, "pil_1": lambda: host_arm(pil_file, 1), "pil_16": lambda: host_arm(pil_file, 16), "host_1": lambda: host_arm(host_file, 1),
            "host_pool": lambda: host_arm(host_file, 16)}
    files, rows = {}, {k: [] for k in arms}
    for k, fn in arms.items():                                             # warm-up: code objects, pinned buffers, the pool's threads
        files[k], _ = fn()
    for r in range(args.repeats):                                          # interleaved
        for k, fn in arms.items():
            if k.startswith("pil") and r >= args.pil_repeats:
                continue
            rows[k].append(fn()[1])
    decoded = {k: [np.asarray(Image.open(io.BytesIO(f))) for f in files[k]] for k in files}
    same = all(np.array_equal(a, b) for k in decoded for a, b in zip(decoded[k], decoded["pil_1"]))
    res = {"case": f"the eight PNG files of one {W} x {H} frame of the bench room ({args.tris} triangles), maps of one render_view round at spp {args.spp}",
           "files": names, "all_arms_decode_to_the_same_pixels": bool(same), "arms": {}}
    for k in arms:
        med = {f: round(median([r[f] for r in rows[k]]), 3) for f in rows[k][0]}
        med["passes"] = len(rows[k])
        med["bytes_per_file"] = [len(f) for f in files[k]]
        med["total_bytes"] = sum(len(f) for f in files[k])
        med["ms_per_frame"] = round(med["wall_ms"] if k == "device" else med["maps_copy_ms"] + med["encode_ms"], 3)
        res["arms"][k] = med
    res["device_bytes_over_pil"] = round(res["arms"]["device"]["total_bytes"] / res["arms"]["pil_1"]["total_bytes"], 4)
    print("# arms done: " + json.dumps({k: v["ms_per_frame"] for k, v in res["arms"].items()}), file=sys.stderr, flush=True)

    # ---- render_view itself
    def timed_view(SPP):
        torch.cuda.synchronize()
        t = time.perf_counter()
        view(1, SPP)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    timed_view(args.spp)
    one_round = median([timed_view(args.spp) for _ in range(3)])
    rounds = args.SPP // args.spp
    full = timed_view(args.SPP) if one_round * rounds * 1e-3 < args.full_view_limit_s else None
    res["render_view"] = {"one_round_ms": round(one_round, 1), "spp": args.spp, "SPP": args.SPP, "rounds": rounds, "ms_per_frame_at_SPP": None if full is None else round(full, 1),
                          "note": "measured once" if full is not None else "not measured: one round times the round count exceeds --full_view_limit_s"}
    if full is not None:
        res["share_of_a_serial_stage"] = {k: round(v["ms_per_frame"] / (full + v["ms_per_frame"]), 4) for k, v in res["arms"].items()}

    # ---- the stage's loop, one round per frame
    loops = {}
    with tempfile.TemporaryDirectory() as tmp:
        for enc in ("device", "host", "device", "host"):
            writer = RV.FrameWriter(dev, enc)
            writer.submit(os.path.join(tmp, enc + "_warm"), 0, view(0, args.spp)); writer.close()
            writer = RV.FrameWriter(dev, enc)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i in range(args.frames):
                writer.submit(os.path.join(tmp, enc), i, view(i, args.spp))
            writer.close()
            torch.cuda.synchronize()
            loops.setdefault(enc, []).append((time.perf_counter() - t) * 1e3 / args.frames)
    res["stage_loop_one_round_per_frame"] = {"frames": args.frames, "render_only_ms_per_frame": round(one_round, 1),
                                             "device_ms_per_frame": [round(x, 1) for x in loops["device"]], "host_ms_per_frame": [round(x, 1) for x in loops["host"]],
                                             "serial_pil_16_ms_per_frame": round(one_round + res["arms"]["pil_16"]["ms_per_frame"], 1),
                                             "serial_pil_1_ms_per_frame": round(one_round + res["arms"]["pil_1"]["ms_per_frame"], 1)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
