#!/usr/bin/env python3
"""Times the BRDF-CRF training step and its optimizer part on one GPU -> profiles/train_brdf_crf_step.json.

    python tools/bench_train_step.py [--steps 60] [--warmup 10] [--views 8] [--res 128] [--batch 8192] [--out profiles/train_brdf_crf_step.json]

The step is BRDFCRFTrainer's (brdf_crf_loss on a PixelSet batch of the reference's size, 8192 pixels, backward, optimizer) on a synthetic scene: the open
box, random 8-bit images, a random shading cache.  Three arms, each with its own material network, CRF and optimizer over the same pixel set:
    fused        iris_amd.utils.optim.FusedAdam(networks=[material]): the update and the half copy the forward reads, in one pass
    torch        torch.optim.Adam with its defaults (the reference's configuration), then the forward's refresh (iris_ngp_set_params_dev)
    torch_fused  torch.optim.Adam(fused=True), then the same refresh
The optimizer part is `optimizer.step()` plus whatever makes the next forward see the new parameters (`material._handle(device)`: nothing for the first
arm); it is timed with device events inside the whole step, which is timed the same way.  The arms are interleaved step by step in one process after the
warm-up; medians and quartiles are recorded.  Needs a HIP device: there is nothing to measure without one."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    f = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(np.asarray(up, np.float64), f)
    r /= np.linalg.norm(r)
    return np.concatenate([np.stack([r, np.cross(f, r), f], 1), np.asarray(eye, np.float64).reshape(3, 1)], 1).astype(np.float32)


def build(args, dev):
    from iris_amd.utils.dataset import PixelSet
    from iris_amd.utils.path_tracing import Scene
    from iris_amd.utils.shading_cache import ShadingCache
    g = np.random.default_rng(0)
    H = W = args.res
    n = args.views * H * W
    cams = []
    for v in range(args.views):
        eye = g.uniform(-0.4, 0.4, 3)
        target = eye + np.array([np.cos(v * 2.39996), 0.3 * np.sin(v), np.sin(v * 2.39996) - 0.2])
        cams.append(dict(kind="real", K=np.array([[0.8 * W, 0, W / 2], [0, 0.8 * W, H / 2], [0, 0, 1]], np.float32), c2w=look_at(eye, target)))
    ps = PixelSet(cams, (H, W), g.integers(0, 256, (n, 3)).astype(np.uint8), segmentation=g.integers(0, 24, n).astype(np.int32),
                  int_albedo=g.integers(0, 256, (n, 3)).astype(np.uint8), exposure=(0.5 + g.random(args.views)).astype(np.float32), batch_size=args.batch, device=dev)
    cache = ShadingCache(n, 6, dev)
    cache.rows.copy_(torch.rand(cache.rows.shape, generator=torch.Generator().manual_seed(1)).to(dev))
    ps.attach_cache(cache)
    box_v = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float32)
    box_f = np.array([t for a, b, c, d in [(0, 1, 3, 2), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)] for t in ((a, b, c), (a, c, d))], np.int32)
    kept = ps.restrict_to_hits(Scene(box_v, box_f, device=dev), store_positions=True)
    if kept < 2 * args.batch:
        raise SystemExit(f"only {kept} pixels hit the box: raise --views or --res")
    return ps, kept


class Arm:
    def __init__(self, name, ps, dev):
        from iris_amd.model.brdf import NGPBRDF
        from iris_amd.model.crf import EmorCRF
        from iris_amd.train_brdf_crf import BRDFCRFTrainer, default_hparams
        from iris_amd.utils.optim import FusedAdam
        s = torch.linspace(0, 1, 256)
        material = NGPBRDF(-1.5, 1.5).init_parameters(seed=5).to(dev)
        crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (j + 1)) * 0.05 for j in range(3)])).to(dev)
        self.trainer = tr = BRDFCRFTrainer(material, crf, ps, default_hparams(batch_size=ps.batch_size, has_part=0, la=0.01, experiment_name=None))
        params = [material.mlp.params, crf.weight]
        if name == "fused":
            assert isinstance(tr.optimizer, FusedAdam)
        elif name == "torch":
            tr.optimizer = torch.optim.Adam(params, lr=1e-3)
        elif name == "torch_fused":
            tr.optimizer = torch.optim.Adam(params, lr=1e-3, fused=True)
        self.name, self.dev, self.material, self.n_steps, self.events = name, dev, material, 0, []

    def step(self, record):
        tr, ps = self.trainer, self.trainer.ps
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        batch = ps[self.n_steps % (len(ps) - 1)]                     # (never the short last batch)
        ev[0].record()
        out = tr.training_step(batch, self.n_steps)
        tr.optimizer.zero_grad(set_to_none=True)
        out["loss"].backward()
        ev[1].record()
        tr.optimizer.step()
        self.material._handle(self.dev)                              # what the next forward would do first: the refresh (a no-op after the fused step)
        ev[2].record()
        self.n_steps += 1
        if record:
            self.events.append(ev)
        return out["loss"]

    def summary(self):
        def stats(x):
            q1, med, q3 = np.percentile(np.asarray(x), [25, 50, 75])
            return dict(median_ms=float(med), q1_ms=float(q1), q3_ms=float(q3), iqr_ms=float(q3 - q1), min_ms=float(np.min(x)), n=len(x))
        return dict(step=stats([e[0].elapsed_time(e[2]) for e in self.events]), optimizer_part=stats([e[1].elapsed_time(e[2]) for e in self.events]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_brdf_crf_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_step: no HIP device: nothing is measured without one")
    from iris_amd import _lib as L
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ps, kept = build(args, dev)
    ps.resample(torch.Generator(device=dev).manual_seed(2))
    arms = [Arm(name, ps, dev) for name in ("fused", "torch", "torch_fused")]
    for k in range(args.warmup + args.steps):
        for arm in (arms if k % 2 == 0 else arms[::-1]):           # interleaved, the order alternating
            loss = arm.step(record=k >= args.warmup)
    torch.cuda.synchronize()
    if not bool(torch.isfinite(loss)):
        raise SystemExit("bench_train_step: the loss is not finite")
    n = int(L.lib().iris_ngp_n_params())
    res = {a.name: a.summary() for a in arms}
    fused = res["fused"]["optimizer_part"]
    best = min(("torch", "torch_fused"), key=lambda k: res[k]["optimizer_part"]["median_ms"])
    base = res[best]["optimizer_part"]
    out = dict(device=torch.cuda.get_device_name(dev), torch=torch.__version__, build=L.build_id(), batch=args.batch, views=args.views, res=args.res,
               pixels_on_the_mesh=kept, warmup=args.warmup, steps=args.steps, n_params=n, arms=res,
               bytes_model=dict(fused_step_bytes=30 * n, note="fused: reads p, g, m, v and writes p, m, v (28 B) plus the half copy (2 B) per parameter; "
                                "torch fused: 28 B per parameter, then the refresh's 4 B read + 2 B written; the backward's torch.zeros of the gradient "
                                "(4 B per parameter) is part of every arm's step, not of the optimizer part"),
               fused_optimizer_GBps=30 * n / (fused["median_ms"] * 1e-3) / 1e9,
               faster_baseline=best,
               fused_not_slower_than_faster_baseline_plus_its_iqr=bool(fused["median_ms"] <= base["median_ms"] + base["iqr_ms"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
