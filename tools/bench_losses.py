#!/usr/bin/env python3
"""The trainers' albedo regulariser (train_brdf_crf.py:292-306, initialize.py:188-201) at the trainer's shape: the fused HIP path
(iris_amd.utils.losses.segment_albedo_loss, forward + backward) against the reference's lines restated in plain torch on the same GPU, in one process.

Shape: N = 8192 pixels in a fixed seeded layout of 40 segments, both modes (mse: initialize.py; scale_invariant at la = 0.01: train_brdf_crf.py).
Timed under HIP events: one window over --steps iterations after --warmup, for the fused call with the sort inside (raw ids) and with a prebuilt
SegmentRuns (what a step that also calls a propagation loss pays), and for the yardstick: segmentation.unique, index_add_ in the place of the three
torch_scatter calls, compute_scale's .item() (a host round trip per step) and mse_loss, autograd for the backward.  Each arm is timed twice, the fused
one again after the other: the spread of the same code in one process is reported beside the ratio.  The times include the host's launches: at this
size both arms are launch- and latency-bound, so they are times per call, not kernel times.
Writes one JSON object (and prints it): --out, default profiles/losses.json.
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

N, SEGMENTS, LA = 8192, 40, 0.01


def layout():
    """40 segment sizes summing to N: seeded cuts"""
    g = torch.Generator().manual_seed(0)
    cut = torch.sort(torch.randperm(N - 1, generator=g)[:SEGMENTS - 1] + 1).values.tolist()
    return [b - a for a, b in zip([0] + cut, cut + [N])]


def torch_step(albedo, prior, seg, scale_invariant):
    """the reference's lines (torch_scatter's sums as index_add_)"""
    seg_idxs, inv_idxs = seg.unique(return_inverse=True)
    weight_seg_ = torch.ones(len(seg), device=seg.device)
    weight_seg = torch.zeros(len(seg_idxs), device=seg.device).index_add_(0, inv_idxs, weight_seg_).unsqueeze(-1)
    mean = torch.zeros(len(seg_idxs), 3, device=seg.device).index_add_(0, inv_idxs, prior * weight_seg_.unsqueeze(-1))
    mean = (mean / weight_seg)[inv_idxs]
    if not scale_invariant:
        return torch.nn.functional.mse_loss(albedo, mean)
    s, t = mean.view(-1), albedo.view(-1)
    scale = (torch.dot(s, t) / torch.dot(s, s)).item()
    return LA * torch.nn.functional.mse_loss(mean * scale, albedo)


def timed(fn, steps, warmup):
    """ms per call: one event window over `steps` calls, after `warmup` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000); ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "losses.json"))
    args = ap.parse_args()
    from iris_amd import _lib as L
    from iris_amd.utils.losses import segment_albedo_loss
    from iris_amd.utils.propagation import SegmentRuns
    dev = torch.device("cuda:0")
    sizes = layout()
    g = torch.Generator().manual_seed(1)
    seg = torch.cat([torch.full((c,), 7 * k + 3, dtype=torch.int64) for k, c in enumerate(sizes)])[torch.randperm(N, generator=g)].to(dev)
    albedo = (0.05 + 0.9 * torch.rand(N, 3, generator=g)).to(dev).requires_grad_(True)
    prior = (torch.randint(0, 256, (N, 3), generator=g).float() / 255.0).to(dev)
    sr = SegmentRuns(seg)
    out = {"what": "albedo regulariser, forward + backward: fused HIP call vs the reference's lines in plain torch (index_add_, .item()) on the same GPU",
           "box": torch.cuda.get_device_name(0), "build": L.build_id(), "N": N, "segments": sorted(sizes, reverse=True), "steps": args.steps,
           "warmup": args.warmup, "note": "ms per call under HIP events, host launches included; each arm twice, the fused one around the torch one"}
    for mode, si, w in (("mse", False, 1.0), ("scale_invariant", True, LA)):
        def fused(s=seg):
            albedo.grad = None
            segment_albedo_loss(albedo, prior, s, weight=w, scale_invariant=si).backward()

        def restated():
            albedo.grad = None
            torch_step(albedo, prior, seg, si).backward()

        f1, s1 = timed(fused, args.steps, args.warmup), timed(lambda: fused(sr), args.steps, args.warmup)
        t1, t2 = timed(restated, args.steps, args.warmup), timed(restated, args.steps, args.warmup)
        f2, s2 = timed(fused, args.steps, args.warmup), timed(lambda: fused(sr), args.steps, args.warmup)
        ref = float(torch_step(albedo, prior, seg, si).detach())
        got = float(segment_albedo_loss(albedo, prior, seg, weight=w, scale_invariant=si).detach())
        out[mode] = {"fused_ms_per_step": [round(f1, 4), round(f2, 4)], "fused_shared_runs_ms_per_step": [round(s1, 4), round(s2, 4)],
                     "torch_ms_per_step": [round(t1, 4), round(t2, 4)], "torch_over_fused": round(min(t1, t2) / max(f1, f2), 2),
                     "torch_over_fused_shared_runs": round(min(t1, t2) / max(s1, s2), 2), "loss_fused": got, "loss_torch": ref}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
