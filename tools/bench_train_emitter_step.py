#!/usr/bin/env python3
"""Times the emitter stage's training step with the fused photometric loss and with the composition it replaces -> profiles/train_emitter_step.json.

    python tools/bench_train_emitter_step.py [--steps 40] [--warmup 6] [--rays 8192] [--spp 32] [--calls 4] [--tris 1000000] [--out profiles/train_emitter_step.json]

The step is RadianceTrainer's in mode 'emitter' at the reference's size (8192 rays, spp 32, SPP // spp = 4: train_emitter.py:181-195) on bench.py's synthetic
1.0 M-triangle room, through NGPBRDF with random parameters: path_tracing_single_step, the loss, backward, the Adam step of emitter.radiance.  Two arms over
the same scene, rays, emitter, response model and optimizer:
    fused      photometric_loss(L_sum, n, ...): one call for loss, psnr and d loss / d L_sum
    composed   mse_loss(model_crf(L_sum / n, e), gt) and -10 log10(clamp_min(loss, 1e-5)): the division, the lookup, the mse and their autograd nodes
The arms are interleaved step by step in one process after the warm-up, the order alternating; the whole step and its parts (integrator forward, loss forward,
backward + optimizer) are timed with device events; medians and quartiles are recorded.  Needs a HIP device: there is nothing to measure without one."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_emitter_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_emitter_step: no HIP device: nothing is measured without one")
    import bench
    from iris_amd import _lib as L
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils.losses import photometric_loss
    from iris_amd.utils.optim import FusedAdam
    from iris_amd.utils.path_tracing import path_tracing_single_step
    from tools.bench_pt_single import _workload
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    room, slf, emi, scene, emitter0 = bench.build_workload(argparse.Namespace(scene_seed=1, tris=args.tris, slf_res=256, layout=0), dev)
    em, (o, d, dx, dy), mat, gt = _workload(slf, emi, emitter0, dev, args.rays, "ngp")
    s = torch.linspace(0, 1, 1024)
    crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (j + 1)) * 0.05 for j in range(3)])).to(dev)
    crf.weight.requires_grad_(False)
    exposure = (0.5 + torch.rand(args.rays, 1, generator=torch.Generator().manual_seed(3))).to(dev)
    optimizer = FusedAdam([em.radiance], lr=1e-6)
    n = args.calls

    def fused(L_sum):
        out = photometric_loss(L_sum, n, crf=crf, exposure=exposure, rgbs_gt=gt)
        return out["loss_c"], out["psnr"]

    def composed(L_sum):
        loss = torch.nn.functional.mse_loss(crf(L_sum / n, exposure), gt)
        return loss, -10.0 * torch.log10(loss.detach().clamp_min(1e-5))

    arms = {"fused": fused, "composed": composed}
    events = {k: [] for k in arms}
    last = {}

    def step(name, record):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        L_sum = path_tracing_single_step(scene, em, mat, o, d, dx, dy, args.spp, n)
        ev[1].record()
        loss, psnr = arms[name](L_sum)
        ev[2].record()
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        optimizer.step()
        ev[3].record()
        last[name] = (loss.detach(), psnr)
        if record:
            events[name].append(ev)

    for k in range(args.warmup + args.steps):
        for name in (list(arms) if k % 2 == 0 else list(arms)[::-1]):           # interleaved, the order alternating
            step(name, k >= args.warmup)
    torch.cuda.synchronize()
    if not all(bool(torch.isfinite(v[0])) for v in last.values()):
        raise SystemExit("bench_train_emitter_step: the loss is not finite")

    def stats(x):
        q1, med, q3 = np.percentile(np.asarray(x), [25, 50, 75])
        return dict(median_ms=float(med), q1_ms=float(q1), q3_ms=float(q3), iqr_ms=float(q3 - q1), min_ms=float(np.min(x)), n=len(x))
    res = {name: dict(step=stats([e[0].elapsed_time(e[3]) for e in evs]), integrator_forward=stats([e[0].elapsed_time(e[1]) for e in evs]),
                      loss_forward=stats([e[1].elapsed_time(e[2]) for e in evs]), backward_and_optimizer=stats([e[2].elapsed_time(e[3]) for e in evs]))
           for name, evs in events.items()}
    f, c = res["fused"], res["composed"]
    saved = c["step"]["median_ms"] - f["step"]["median_ms"]
    noise = max(f["step"]["iqr_ms"], c["step"]["iqr_ms"])
    out = dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, build=L.build_id(), rays=args.rays, spp=args.spp, calls_per_step=n,
               triangles=int(room["faces"].shape[0]), material="NGPBRDF, random parameters", crf_knots=1024, warmup=args.warmup, steps=args.steps, arms=res,
               loss_values={k: float(v[0]) for k, v in last.items()},
               loss_share_of_the_fused_step=(f["loss_forward"]["median_ms"]) / f["step"]["median_ms"],
               step_ms_saved_by_the_fused_loss=saved, larger_iqr_of_the_two_steps_ms=noise,
               difference_exceeds_the_noise=bool(abs(saved) > noise),
               note="device events inside one process, arms interleaved step by step; loss_forward is the span between the integrator's return and the loss value; "
                    "backward_and_optimizer holds the loss's backward, the integrator's gradient scatter and the Adam step of emitter.radiance in both arms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
