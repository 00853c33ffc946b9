#!/usr/bin/env python3
"""The camera response model (iris_amd/model/crf.py) at the shapes it runs at: the fused HIP calls against the same interpolator contract composed of
plain torch ops on the same GPU in the same process (tools/crf_restatement.py: per channel a bucketize, clamps, masked selects, two gathers and a
division; autograd for the backward) -- the code a user would write without the kernels, not the code under test.

  forward            model(L, exposure)                        B = 8192 (the BRDF trainer's batch), per-pixel exposure
  forward+backward   ... .sum().backward() into L and weight   B = 8192
  inverse            model.inverse(rgbs, exposure)             B = 2 073 600 (one 1080p view), the inverse table rebuilt per call as the reference does

Median of --steps timed calls after --warmup calls, each between its own pair of HIP events.  Writes one JSON line (and prints it): --out, default
profiles/crf_bench.json.  EMoR curves are data the user brings: without --emor a smooth synthetic f0 / basis of the same shape is used (the timings do not
depend on the values).
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

B_TRAIN, B_VIEW, DIM, N = 8192, 1920 * 1080, 11, 1024


def timed(fn, steps, warmup):
    """median ms of `steps` calls, each between its own events, after `warmup` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--emor", default=None, help="emor.txt; default: synthetic curves")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "crf_bench.json"))
    args = ap.parse_args()
    if args.steps < 20:
        raise SystemExit("--steps: at least 20 timed calls")
    from iris_amd import _lib as L
    from iris_amd.model.crf import EmorCRF
    from tools import crf_restatement as R
    dev = torch.device("cuda:0")
    if args.emor:
        model = EmorCRF(dim=DIM, emor_path=args.emor)
    else:
        s = torch.linspace(0, 1, N)
        model = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin((k + 1) * torch.pi * s) / (k + 1) for k in range(DIM)]))
    model = model.to(dev)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        model.weight.copy_(0.02 * torch.randn(3, DIM, generator=g))
    hdr = (torch.rand(B_TRAIN, 3, generator=g) * 1.4 - 0.1).to(dev).requires_grad_(True)
    e_train = (torch.rand(B_TRAIN, 1, generator=g) * 1.5 + 0.5).to(dev)
    ldr_view = torch.rand(B_VIEW, 3, generator=g).to(dev)
    e_view = 1.3

    def composed_forward(h, e):
        return R.forward(model.get_crf(), h, e)

    def fused_fwd():
        with torch.no_grad():
            model(hdr, e_train)

    def torch_fwd():
        with torch.no_grad():
            composed_forward(hdr, e_train)

    def fused_fwd_bwd():
        hdr.grad = model.weight.grad = None
        model(hdr, e_train).sum().backward()

    def torch_fwd_bwd():
        hdr.grad = model.weight.grad = None
        composed_forward(hdr, e_train).sum().backward()

    def fused_inverse():
        model.inverse(ldr_view, e_view)

    def torch_inverse():
        with torch.no_grad():
            R.inverse(R.inv_table(model.get_crf()), ldr_view, e_view)

    # the two arms compute the same thing (lookups bit for bit; see tests/test_crf.py for the sums)
    with torch.no_grad():
        same_fwd = bool(torch.equal(model(hdr, e_train), composed_forward(hdr, e_train)))
        inv_dev = float((model.inverse(ldr_view, e_view) - R.inverse(R.inv_table(model.get_crf()), ldr_view, e_view)).abs().max())
    res = {}
    for name, fn in (("fused_forward", fused_fwd), ("torch_forward", torch_fwd), ("fused_forward_backward", fused_fwd_bwd),
                     ("torch_forward_backward", torch_fwd_bwd), ("fused_inverse_1080p", fused_inverse), ("torch_inverse_1080p", torch_inverse),
                     ("fused_forward_repeat", fused_fwd)):
        res[name + "_ms"] = round(timed(fn, args.steps, args.warmup), 4)
    out = {"what": "EmorCRF: fused HIP calls vs the same interpolator contract composed of plain torch ops on the same GPU; medians of per-call event times",
           "box": torch.cuda.get_device_name(0), "build": L.build_id(), "B_train": B_TRAIN, "B_view": B_VIEW, "n": N, "dim": DIM, "steps": args.steps,
           "warmup": args.warmup, "curves": "emor.txt" if args.emor else "synthetic", **res,
           "torch_over_fused_forward": round(res["torch_forward_ms"] / res["fused_forward_ms"], 2),
           "torch_over_fused_forward_backward": round(res["torch_forward_backward_ms"] / res["fused_forward_backward_ms"], 2),
           "torch_over_fused_inverse": round(res["torch_inverse_1080p_ms"] / res["fused_inverse_1080p_ms"], 2),
           "inverse_bytes_moved": B_VIEW * 3 * 4 * 2, "inverse_GBps": round(B_VIEW * 24 / (res["fused_inverse_1080p_ms"] * 1e-3) / 1e9, 1),
           "forward_bit_identical": same_fwd, "inverse_max_abs_difference": inv_dev,
           "note": "call times include the host's launches (the 8192 shapes are launch-bound); the fused calls include get_crf's matmul, the inverse also the table kernel"}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
