#!/usr/bin/env python3
"""The scannetpp layout's --res_scale 0.5 on one view's three images (photograph, albedo prior, segment ids) on one MI355X -> profiles/resize_scannetpp.json.

Two size pairs: 1168 x 1752 -> 584 x 876 (both axes exactly 2: the rounded 2 x 2 mean) and 1169 x 1753 -> 584 x 876 (the general fixed-point path); seeded
8-bit images; photograph and prior resized linear, the ids nearest (iris_amd/utils/resize.py, iris_amd/csrc/iris_resize.h).  In the same process, the arms
taking turns call by call (--warmup calls, then the median and the half distance between the 16th and 84th percentile of --steps calls):

  upload_resize   what a stage does per view: the three full-size host arrays to the device and the three resize_u8 calls (host clock around a synchronise)
  kernel          the three resize_u8 calls on device-resident images (HIP events; also the host clock, which adds the launches' host side)
  host_ref        tests/resize_ref.py on the host: the same contract in numpy (host clock)
  pil_bilinear    PIL's BILINEAR (an antialiased triangle filter: DIFFERENT pixels, here for scale only) and NEAREST on the host (host clock)

Beside the kernel's time: the bytes it reads (every source byte once; the tables) and writes, computed from the shapes, and the rate they give.  Before
anything is timed the device result is compared with resize_ref (linear) and PIL (nearest) byte for byte.  No time here is an acceptance threshold."""
import argparse, json, os, statistics, sys, time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

PAIRS = {"exact2": ((1168, 1752), (584, 876)), "general": ((1169, 1753), (584, 876))}


def med(ms):
    return round(statistics.median(ms), 4)


def half_spread(ms):
    s = sorted(ms)
    return round((s[min(len(s) - 1, int(round(0.84 * (len(s) - 1))))] - s[int(round(0.16 * (len(s) - 1)))]) / 2, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resize_scannetpp.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    import resize_ref
    from iris_amd import _lib as L
    from iris_amd.utils.resize import resize_u8
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize needs a HIP device: nothing here is measured on a CPU")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "build": L.build_id(), "steps": args.steps, "warmup": args.warmup, "pairs": {}}
    for label, (src, dst) in PAIRS.items():
        g = np.random.default_rng([7, *src])
        rgb, albedo = (g.integers(0, 256, (*src, 3), dtype=np.uint8) for _ in range(2))
        seg = g.integers(0, 256, src, dtype=np.uint8)
        host = (rgb, albedo, seg)
        modes = ("linear", "linear", "nearest")
        resident = [torch.from_numpy(a).to(dev) for a in host]

        def kernel():
            return [resize_u8(t, dst, m) for t, m in zip(resident, modes)]

        def upload_resize():
            return [resize_u8(torch.from_numpy(a).to(dev), dst, m) for a, m in zip(host, modes)]

        def host_ref():
            return [resize_ref.resize_linear_u8(rgb, dst), resize_ref.resize_linear_u8(albedo, dst), resize_ref.resize_nearest_u8(seg, dst)]

        def pil_bilinear():
            return [np.array(Image.fromarray(a).resize(dst[::-1], Image.BILINEAR)) for a in (rgb, albedo)] + [np.array(Image.fromarray(seg).resize(dst[::-1], Image.NEAREST))]

        want = host_ref()
        got = [t.cpu().numpy() for t in kernel()]
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), label + ": the device result differs from tests/resize_ref.py"
        assert np.array_equal(got[2], pil_bilinear()[2]), label + ": nearest differs from PIL"
        arms = {"upload_resize": upload_resize, "kernel": kernel, "host_ref": host_ref, "pil_bilinear": pil_bilinear}
        wall, events = {k: [] for k in arms}, []
        for step in range(args.warmup + args.steps):
            for name, fn in arms.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                if step >= args.warmup:
                    wall[name].append((time.perf_counter() - t0) * 1e3)
                    if name == "kernel":
                        events.append(e0.elapsed_time(e1))
        n_src, n_dst = src[0] * src[1], dst[0] * dst[1]
        tables = 0 if label == "exact2" else 2 * (dst[0] + dst[1]) * (4 + 4) + 2 * (dst[0] + dst[1]) * 4          # ofs + coef per axis, linear; ofs, nearest
        # the two linear images need every source byte (at a scale of 2 the taps cover the source), the ids one byte per output pixel: between that and every
        # source byte once is what has to come from memory
        bytes_read_max, bytes_read_min, bytes_written = 7 * n_src + tables, 6 * n_src + n_dst + tables, 7 * n_dst
        k_ms = med(events)
        result["pairs"][label] = {
            "source_hw": list(src), "target_hw": list(dst), "images": "rgb (H,W,3) linear, albedo (H,W,3) linear, seg (H,W) nearest", "launches_per_view": 3,
            **{name + "_ms": med(ms) for name, ms in wall.items()}, **{name + "_ms_half_spread": half_spread(ms) for name, ms in wall.items()},
            "kernel_events_ms": k_ms, "kernel_events_ms_half_spread": half_spread(events),
            "kernel_bytes_read_at_most": bytes_read_max, "kernel_bytes_read_at_least": bytes_read_min,
            "kernel_bytes_written": bytes_written, "kernel_GBps_at_most": round((bytes_read_max + bytes_written) / (k_ms * 1e-3) / 1e9, 2),
            "per_colour_image_bytes": 3 * n_src + 3 * n_dst,
            "speedup_kernel_over_host_ref": round(med(wall["host_ref"]) / med(wall["kernel"]), 1),
            "speedup_upload_resize_over_pil_bilinear": round(med(wall["pil_bilinear"]) / med(wall["upload_resize"]), 2)}
        print(label, json.dumps(result["pairs"][label]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
