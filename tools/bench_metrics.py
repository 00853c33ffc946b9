#!/usr/bin/env python3
"""SSIM / PSNR on the device (iris_amd/utils/metrics.py, iris_amd/csrc/iris_metrics.h) at the size the render stage calls it at, 1080 x 1920 x 3, for one
image and for a stack of eight, beside the host path it replaces.

  device   image_metrics(a, b) -- both launches and the float64 epilogue -- between a pair of HIP events: warm-up calls, then the median of --steps >= 20
           calls; also with full=True (the map of S written)
  host     the images copied device -> host (timed apart), then
             * the float64 reference of tests/ssim_ref64.py (explicit windows; in row strips so that the windows fit in memory), one timed run
             * when scipy imports: skimage's formula as skimage evaluates it, scipy.ndimage.uniform_filter in float32, median of three runs
           both for one image; host clock

The measurement runs in a fresh child process under `timeout` (this process never touches the GPU); the child's one JSON line is written to --out (default
profiles/metrics_1080p.json) and printed.  The device and the host results are compared in the same run: a benchmark of something that computes another
number would be worthless.
"""
import argparse, json, os, statistics, subprocess, sys, time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, C = 1080, 1920, 3


def images(n, seed=0):
    """n pairs of a smooth bright image with texture and its noisy copy, float32 in [0, 1] (the timings do not depend on the values)"""
    import numpy as np
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    a = np.empty((n, H, W, C), np.float32)
    for i in range(n):
        for c in range(C):
            a[i, :, :, c] = 0.6 + 0.3 * np.sin(0.01 * (i + 1) * xx + 0.3 * c) * np.cos(0.013 * yy) + 0.02 * g.standard_normal((H, W), np.float32)
    a = np.clip(a, 0, 1)
    b = np.clip(a + 0.03 * g.standard_normal(a.shape, np.float32), 0, 1)
    return a, b


def ref64_strips(a, b, rows=60):
    """mssim of one image pair through tests/ssim_ref64.ssim_ref64, `rows` window rows at a time"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from ssim_ref64 import ssim_ref64
    total = 0.0
    for y0 in range(0, H - 6, rows):
        y1 = min(y0 + rows, H - 6)
        S, _ = ssim_ref64(a[y0:y1 + 6], b[y0:y1 + 6], 1.0)
        total += float(S.sum())
    return total / ((H - 6) * (W - 6) * C)


def scipy_f32(a, b):
    """skimage.metrics.structural_similarity(a, b, data_range=1, channel_axis=-1) on float32 images, as skimage evaluates it; None without scipy"""
    try:
        from scipy.ndimage import uniform_filter
    except ImportError:
        return None
    import numpy as np
    cov_norm, c1, c2 = 49.0 / 48.0, 0.01 ** 2, 0.03 ** 2
    m = []
    for c in range(C):
        x, y = a[..., c], b[..., c]
        ux, uy = uniform_filter(x, size=7), uniform_filter(y, size=7)
        uxx, uyy, uxy = uniform_filter(x * x, size=7), uniform_filter(y * y, size=7), uniform_filter(x * y, size=7)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        m.append(S[3:-3, 3:-3].mean(dtype=np.float64))
    return float(np.mean(m))


def child(steps, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from iris_amd import _lib as L
    from iris_amd.utils.metrics import image_metrics
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    a8, b8 = images(8)
    ta, tb = torch.from_numpy(a8).to(dev), torch.from_numpy(b8).to(dev)

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)

    res = {}
    for n in (1, 8):
        x, y = ta[:n], tb[:n]
        for full in (False, True):
            med, lo, hi = timed(lambda: image_metrics(x, y, 1.0, full=full))
            res[f"device_N{n}{'_with_map' if full else ''}_ms"] = med
            res[f"device_N{n}{'_with_map' if full else ''}_min_max_ms"] = [lo, hi]
    got = image_metrics(ta, tb, 1.0)
    ssim_dev, psnr_dev = got["ssim"].cpu().numpy(), got["psnr"].cpu().numpy()

    # the host path, one image
    torch.cuda.synchronize()
    t = time.perf_counter(); ha, hb = ta[0].cpu().numpy(), tb[0].cpu().numpy(); res["copy_to_host_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    t = time.perf_counter(); m64 = ref64_strips(ha, hb); res["host_ref64_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    ms, m32 = [], None
    for _ in range(3):
        t = time.perf_counter(); m32 = scipy_f32(ha, hb); ms.append((time.perf_counter() - t) * 1e3)
    res["host_scipy_f32_ms"] = None if m32 is None else round(statistics.median(ms), 1)
    psnr64 = 10 * np.log10(1.0 / np.mean((ha.astype(np.float64) - hb.astype(np.float64)) ** 2))
    out = {"what": "image_metrics (SSIM + PSNR, fused HIP) at 1080 x 1920 x 3: medians of per-call HIP event times, beside the host path it replaces (copy + numpy / scipy), one image",
           "box": torch.cuda.get_device_name(0), "build": L.build_id(), "H": H, "W": W, "C": C, "steps": steps, "warmup": warmup, **res,
           "ssim_device_image0": float(ssim_dev[0]), "ssim_ref64_image0": m64, "ssim_scipy_f32_image0": m32, "psnr_device_image0": float(psnr_dev[0]), "psnr_ref64_image0": float(psnr64),
           "taps_per_call_N1": (H - 6) * (W - 6) * C * 49 * 2,
           "note": "device times include the host's two launches and the torch epilogue (a few small float64 ops); host_ref64 is a numpy restatement written for clarity, "
                   "not speed; host times are host-clock, single process"}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the child process may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "metrics_1080p.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 20:
        raise SystemExit("--steps: at least 20 timed calls")
    if args.child:
        return child(args.steps, args.warmup)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.stdout.write(p.stdout)
        raise SystemExit(f"bench_metrics: the measurement ended with status {p.returncode}; nothing written")
    line = lines[-1][len("RESULT "):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
