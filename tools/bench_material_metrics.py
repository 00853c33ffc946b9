#!/usr/bin/env python3
"""The material metrics (iris_amd/utils/material_metrics.py, iris_amd/csrc/iris_matmetrics.h) on eight views of 1080 x 1920, the size the render stage
writes: the fused launch beside the same sums composed from torch operations on the device and beside numpy on the host.

  fused_u8 / fused_f32   material_metrics(gt, est) of the eight-view stack -- both launches and the float64 epilogue --, the estimates as the PNGs' code
                         values / as float32 maps; fused_u8_N1: one view per call (the launch-bound case the batching is for)
  torch                  the same eight words per view from elementwise torch operations and per-view sums on the device (uint8 estimates)
  numpy                  tests/material_metrics_ref.exact on the host, the arrays already in memory: a restatement written for clarity, not for speed

The device arms are timed between HIP events, interleaved call by call (fused_u8, fused_f32, fused_u8_N1, torch, then again) after warm-up calls of each;
median, minimum and maximum of --steps calls.  The numpy arm is one run on the host clock.  All arms must give the same seven integers per view, and S_emit
to 1e-12 relative, or nothing is written.  The measurement runs in a fresh child process under `timeout`; its one JSON line goes to --out (default
profiles/material_metrics_1080p.json).  The command line python -m iris_amd.utils.metric_brdf is not what this times: it is bound by decoding the files on
the host.
"""
import argparse, json, os, statistics, subprocess, sys, time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 8, 1080, 1920


def torch_composed(g, e):
    """the kernel's eight words per view from torch operations: (N,7) int64 and (N,) float64"""
    import torch
    zero, one = torch.zeros((), device=g["emit"].device), torch.ones((), device=g["emit"].device)
    q = lambda x: (torch.fmin(torch.fmax(x, zero), one) * 255.0).to(torch.int64)
    code = lambda x: x.to(torch.int64) if x.dtype == torch.uint8 else q(x)
    mask = lambda x: ((x[..., 0] + x[..., 1]) + x[..., 2]) > 0
    m, m_est = mask(g["emit"]), mask(e["emit"])
    keep = ~m
    p = g["rough"] * 255.0
    r_gt = torch.where(torch.isnan(p), zero, p).clamp(51.0, 255.0).to(torch.int64) * keep
    r = code(e["rough"]).clamp(51, 255) * keep
    diff = (r_gt == 255)[..., None]
    a = (code(e["albedo"]) - q(g["albedo"])) * keep[..., None]
    k = (code(e["kd"]) - q(g["kd"])) * diff
    d = torch.log(e["emit"].double() + 1.0) - torch.log(g["emit"].double() + 1.0)
    ints = torch.stack([(a * a).sum((1, 2, 3)), (k * k).sum((1, 2, 3)), ((r - r_gt) ** 2).sum((1, 2)), m.sum((1, 2)), m_est.sum((1, 2)), (m & m_est).sum((1, 2)),
                        (m | m_est).sum((1, 2))], 1)
    return ints, (d * d).sum((1, 2, 3))


def child(steps, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import material_metrics_ref as R
    from iris_amd import _lib as L
    from iris_amd.utils.material_metrics import material_metrics
    if not torch.cuda.is_available():
        raise SystemExit("bench_material_metrics needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    gt, u8, f32 = R.make_inputs(N, H, W, 2024)
    t = time.perf_counter(); ref = R.exact(gt, u8); numpy_ms = (time.perf_counter() - t) * 1e3
    ref_f32 = R.exact(gt, f32)
    up = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    g, e8, ef = up(gt), up(u8), up(f32)
    g1, e1 = {k: v[:1] for k, v in g.items()}, {k: v[:1] for k, v in e8.items()}
    arms = {"fused_u8": lambda: material_metrics(g, e8), "fused_f32": lambda: material_metrics(g, ef), "fused_u8_N1": lambda: material_metrics(g1, e1),
            "torch": lambda: torch_composed(g, e8)}

    # every arm computes the same numbers
    def words(res):
        s = res["sums"].cpu().numpy()
        return s[:, :7], np.ascontiguousarray(s[:, 7]).view(np.float64)
    for name, want in (("fused_u8", ref), ("fused_f32", ref_f32)):
        ints, s_emit = words(arms[name]())
        if not ((ints == want["sums"]).all() and np.allclose(s_emit, want["s_emit"], rtol=1e-12, atol=0)):
            raise SystemExit(f"bench_material_metrics: {name} disagrees with the numpy restatement; nothing written")
    t_ints, t_emit = arms["torch"]()
    if not ((t_ints.cpu().numpy() == ref["sums"]).all() and np.allclose(t_emit.cpu().numpy(), ref["s_emit"], rtol=1e-12, atol=0)):
        raise SystemExit("bench_material_metrics: the torch arm disagrees with the numpy restatement; nothing written")

    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(steps):
        for name, fn in arms.items():
            e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1_.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1_))
    res = {}
    for name, v in ms.items():
        res[name + "_ms"] = round(statistics.median(v), 4)
        res[name + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
    pixels = N * H * W
    bytes_u8, bytes_f32 = pixels * (52 + 7), pixels * (52 + 28)          # 4 float32 RGB maps and rough_gt, plus the three estimate maps
    out = {"what": "material_metrics (fused HIP) on 8 views of 1080 x 1920: medians of per-call HIP event times, arms interleaved call by call, beside the same sums "
                   "from torch operations on the device and from numpy on the host",
           "box": torch.cuda.get_device_name(0), "build": L.build_id(), "N": N, "H": H, "W": W, "steps": steps, "warmup": warmup, **res,
           "numpy_host_ms": round(numpy_ms, 1), "numpy_host_runs": 1,
           "bytes_read_u8": bytes_u8, "bytes_read_f32": bytes_f32,
           "fused_u8_call_GBps": round(bytes_u8 / (res["fused_u8_ms"] * 1e-3) / 1e9, 1), "fused_f32_call_GBps": round(bytes_f32 / (res["fused_f32_ms"] * 1e-3) / 1e9, 1),
           "launches_per_call": 2,
           "note": "call times include the host's two launches, the workspace allocation and the torch epilogue (a few small float64 ops); *_call_GBps is the bytes the "
                   "maps hold over the CALL time, not a kernel's rate; the numpy arm is a restatement written for clarity, one run on the host clock; the "
                   "command line (python -m iris_amd.utils.metric_brdf) is bound by decoding the EXR and PNG files on the host and was not timed here"}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the child process may take")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "material_metrics_1080p.json"))
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
        raise SystemExit(f"bench_material_metrics: the measurement ended with status {p.returncode}; nothing written")
    line = lines[-1][len("RESULT "):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
