#!/usr/bin/env python3
"""Writes tests/golden/ngp_train_curve.npz: the loss curve of a 20-step Adam fit of the material network through the ORACLE's autograd
(oracle/ngp_torch.py on the CPU, about 3 minutes), which tests/test_ngp_backward.py::test_training_curve_follows_the_oracle repeats through the
HIP path (NGPBRDF under autograd + torch.optim.Adam on the GPU).

    python tools/make_ngp_train_golden.py [--out tests/golden/ngp_train_curve.npz]

The problem (`problem()`, imported by the test so that both sides state it once): 256 fixed points in the box [-1, 1]^3, a smooth
albedo / roughness / metallic target, parameters drawn from a seeded CPU generator (uniform, +-0.3: a network whose outputs are not saturated; not
NGPBRDF.init_parameters, whose tables start at 1e-4), loss = SUM of squared errors over the 256 x 5 outputs (a sum, not a mean: the oracle's autograd
rounds gradients to half without a loss scale, and a mean's 1/1280 would push them into the half subnormals), Adam with torch's defaults at the
learning rate below.  Stored: the 21 losses (before each step and after the last), the seeds and the settings -- a few hundred bytes.
The script refuses to write a curve whose final loss is not under half its first."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PARAM_SEED, POINT_SEED, N_POINTS, N_STEPS, LR = 20, 21, 256, 20, 3e-3
VOXEL_MIN, VOXEL_MAX, PARAM_SCALE = -1.0, 1.0, 0.3


def problem(n_params):
    """(params float32[n_params], positions (256, 3), target (256, 5) = albedo rgb | roughness | metallic), all on the CPU"""
    g = torch.Generator().manual_seed(PARAM_SEED)
    params = (torch.rand(n_params, generator=g) * 2 - 1) * PARAM_SCALE
    g = torch.Generator().manual_seed(POINT_SEED)
    pos = torch.rand(N_POINTS, 3, generator=g) * 2 - 1
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    target = torch.stack([0.5 + 0.4 * torch.sin(2 * x), 0.5 + 0.4 * torch.sin(2 * y + 1), 0.5 + 0.4 * torch.sin(2 * z + 2),
                          0.5 + 0.3 * torch.cos(3 * y), 0.5 + 0.4 * torch.sin(x + z)], dim=1)
    return params, pos, target


def loss_of(out, target):
    """sum of squared errors of the concatenated outputs (albedo 3 | roughness 1 | metallic 1)"""
    pred = torch.cat([out["albedo"], out["roughness"], out["metallic"]], dim=-1)
    return ((pred - target) ** 2).sum()


def main():
    from oracle import ngp_torch as ng
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "ngp_train_curve.npz"))
    ap.add_argument("--lr", type=float, default=LR)
    args = ap.parse_args()
    params, pos, target = problem(ng.n_params())
    params = params.clone().requires_grad_(True)
    opt = torch.optim.Adam([params], lr=args.lr)
    losses = []
    for step in range(N_STEPS + 1):
        opt.zero_grad(set_to_none=True)
        loss = loss_of(ng.forward(params, pos, VOXEL_MIN, VOXEL_MAX), target)
        losses.append(float(loss.detach()))
        print(step, losses[-1], flush=True)
        if step < N_STEPS:
            loss.backward()
            opt.step()
    if not losses[-1] < 0.5 * losses[0]:
        raise SystemExit(f"final loss {losses[-1]} is not under half the first {losses[0]}: no golden written (change the learning rate)")
    np.savez(args.out, losses=np.asarray(losses, np.float64), param_seed=PARAM_SEED, point_seed=POINT_SEED, n_points=N_POINTS, n_steps=N_STEPS,
             lr=np.float64(args.lr), voxel_min=VOXEL_MIN, voxel_max=VOXEL_MAX, param_scale=PARAM_SCALE)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
