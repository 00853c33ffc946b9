#!/usr/bin/env python3
"""The BRDF trainer's propagation regulariser (train_brdf_crf.py:243-290, semantic branch) at the trainer's shape: the fused HIP path
(iris_amd.utils.propagation.semantic_propagation_loss, forward + backward) against the reference's lines restated in plain torch on the same GPU.

Shape: N = 8192 pixels, K = 1024 partners, a fixed seeded layout of 24 segments: one of 3000 pixels, two above K, the rest below (those are exhaustive).
Timed under HIP events: the whole fused call (sort + runs + pack + forward + backward) in one window over --steps iterations, and its forward and backward
halves per iteration (medians).  The yardstick is the torch restatement -- the per-segment host loop with its `if sample_batch > seg_count` on a device
tensor, torch.where, torch.randint, the gathers and three index_add_ (the reference's scatter_add_), autograd for the backward -- not the code under test.
--sweep also times the backward under other workgroup chunkings and LDS limits (iris_debug_set "prop_bwd_targets", "prop_lds_members").
Writes one JSON object (and prints it): --out, default profiles/propagation_bench.json.
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

N, K, SIGMA_A, SIGMA_P, LS = 8192, 1024, 0.05 / 3, 0.1, 1e-3


def layout():
    """24 segment sizes summing to N: 3000, 1400, 1100 and 21 seeded ones below K"""
    g = torch.Generator().manual_seed(0)
    rest = N - 3000 - 1400 - 1100
    cut = torch.sort(torch.randperm(rest - 1, generator=g)[:20] + 1).values.tolist()
    small = [b - a for a, b in zip([0] + cut, cut + [rest])]
    return [3000, 1400, 1100] + small


def torch_step(r, m, albedo, pos, seg):
    """train_brdf_crf.py:247-290 as the reference writes it (torch_scatter's segment mean as an index_add_ and a division)"""
    seg_idxs, inv_idxs, seg_counts = seg.unique(return_inverse=True, return_counts=True)
    ii, jj = [], []
    for seg_idx, seg_count in zip(seg_idxs, seg_counts):
        sample_batch = 1024
        i = torch.where(seg == seg_idx)[0]
        if sample_batch > seg_count:
            sample_batch = seg_count
            j = torch.arange(seg_count, device=seg.device)[None].repeat_interleave(sample_batch, 0).reshape(-1)
        else:
            j = torch.randint(0, seg_count, (seg_count * sample_batch,), device=seg.device)
        jj.append(i[j]); ii.append(i.repeat_interleave(sample_batch, 0))
    ii, jj = torch.cat(ii, 0), torch.cat(jj, 0)
    w = torch.exp(-((albedo.data[ii] - albedo.data[jj]).pow(2).sum(-1) / SIGMA_A ** 2) / 2.0)
    w = w * torch.exp(-((pos[ii] - pos[jj]).pow(2).sum(-1) / SIGMA_P ** 2) / 2.0)
    W = torch.zeros(len(pos), device=pos.device) + 1e-4
    rbar = torch.zeros(len(r), device=r.device).index_add_(0, ii, r[jj].squeeze(-1) * w)
    mbar = torch.zeros(len(m), device=m.device).index_add_(0, ii, m[jj].squeeze(-1) * w)
    W = W.index_add_(0, ii, w)
    l = (rbar / W - r.squeeze(-1)).abs() + (mbar / W - m.squeeze(-1)).abs()
    per_seg = torch.zeros(len(seg_idxs), device=seg.device).index_add_(0, inv_idxs, l) / seg_counts
    return LS * per_seg.sum()


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
    ap.add_argument("--steps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--torch-steps", type=int, default=10)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "propagation_bench.json"))
    args = ap.parse_args()
    from iris_amd import _lib as L
    from iris_amd.utils.propagation import SegmentRuns, semantic_propagation_loss
    dev = torch.device("cuda:0")
    sizes = layout()
    g = torch.Generator().manual_seed(1)
    seg = torch.cat([torch.full((c,), 7 * k + 3, dtype=torch.int64) for k, c in enumerate(sizes)])[torch.randperm(N, generator=g)].to(dev)
    albedo = (0.4 + 0.05 * torch.rand(N, 3, generator=g)).to(dev)
    pos = ((torch.rand(N, 3, generator=g) * 2 - 1) * 0.15).to(dev)
    r = (0.02 + 0.98 * torch.rand(N, 1, generator=g)).to(dev).requires_grad_(True)
    m = torch.rand(N, 1, generator=g).to(dev).requires_grad_(True)
    pairs = sum(c * min(c, K) for c in sizes)
    kw = dict(sigma_albedo=SIGMA_A, sigma_pos=SIGMA_P, ls=LS, n_samples=K)
    step = [0]

    def fused():
        step[0] += 1
        r.grad = m.grad = None
        semantic_propagation_loss(r, m, albedo, pos, seg, seed=step[0], **kw).backward()

    def restated():
        r.grad = m.grad = None
        torch_step(r, m, albedo, pos, seg).backward()

    fused_ms = timed(fused, args.steps, args.warmup)
    torch_ms = timed(restated, args.torch_steps, 2)
    fused_ms2 = timed(fused, args.steps, args.warmup)              # again after the other arm: the spread of the same code in one process

    def halves():
        """medians of the forward and the backward call of one iteration (runs prebuilt), each between its own events"""
        sr = SegmentRuns(seg)
        f, b = [], []
        for it in range(args.warmup + args.steps):
            r.grad = m.grad = None
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            loss = semantic_propagation_loss(r, m, albedo, pos, sr, seed=it, **kw)
            e[1].record()
            loss.backward()
            e[2].record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                f.append(e[0].elapsed_time(e[1])); b.append(e[1].elapsed_time(e[2]))
        return statistics.median(f), statistics.median(b)

    fwd_ms, bwd_ms = halves()
    out = {"what": "propagation regulariser, semantic branch, forward + backward: fused HIP call vs the reference's lines in plain torch on the same GPU",
           "box": torch.cuda.get_device_name(0), "build": L.build_id(), "N": N, "K": K, "segments": sorted(sizes, reverse=True), "pairs": pairs,
           "steps": args.steps, "fused_ms_per_step": round(fused_ms, 4), "fused_ms_per_step_repeat": round(fused_ms2, 4),
           "torch_ms_per_step": round(torch_ms, 4), "torch_over_fused": round(torch_ms / fused_ms, 2),
           "fused_forward_call_ms_median": round(fwd_ms, 4), "fused_backward_call_ms_median": round(bwd_ms, 4),
           "backward_over_forward": round(bwd_ms / fwd_ms, 2),
           "gather_bytes_one_pass": pairs * 32, "note": "call times include the host's launches; kernel times: rocprofv3 --kernel-trace --stats in a run of its own"}
    if args.sweep:
        out["sweep_backward_call_ms_median"] = {}
        for targets, members in ((32, 8192), (16, 8192), (64, 8192), (128, 8192), (32, 2048), (32, 0), (32, 8192)):
            L.debug_set("prop_bwd_targets", targets); L.debug_set("prop_lds_members", members)
            out["sweep_backward_call_ms_median"].setdefault(f"targets{targets}_lds{members}", []).append(round(halves()[1], 4))
        L.debug_set("prop_bwd_targets", -1); L.debug_set("prop_lds_members", -1)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
