#!/usr/bin/env python3
"""Writes tests/golden/crf_emor.npz: the reference's own EmorCRF (crf/model_crf.py, imported unmodified with stub modules, working directory set to the
reference as SURVEY.md's appendix describes) run on the CPU in float32 over three weight cases and one set of inputs.

    python tools/make_crf_golden.py --reference /path/to/reference [--out tests/golden/crf_emor.npz]

The reference interpolates with torch_interpolations, which is not available; tools/crf_restatement.py's RegularGridInterpolator (the project's interpolator
contract) is installed under that name.  Everything else is the reference's code: the clip, the table, the channel loop, the exposure handling,
mono_increase_constraint and the three regularisers.  Build container only: the reference does not travel with the repository.

Inputs (N rows of three channels, the same for every case; `block` gives the row ranges):
  knots    every float32 knot of linspace(0, 1, 1024), the float below and the float above it, the same value in the three channels, then exact 0 and 1,
           negatives and values above 1; python-float exposure 1.0 (so the product is the value itself)
  scalar   uniform draws in [-0.1, 1.3], exposure 1.7 as a python float
  pixel    uniform draws in [-0.1, 1.3], exposure (B, 1) uniform in [0.5, 2]
Size.  The fixture holds 8 547 rows: the knots block has 3 085, each uniform block holds DRAWS_PER_BLOCK = 8 192 numbers, that is 2 731 rows of three
channels.  This is fewer than the about 20 000 rows (8 192 rows per uniform block) the fixture was planned with, and the file is 753 KB, more than the
few hundred KB planned.  The reason is that per case three (N, 3) float32 outputs are stored (ldr, ghdr, hdr) beside x, and uniform draws do not
compress: 19 469 rows would come to 19 469 * 12 B * (1 + 3 * 3) = 2.3 MB, above the 1 MiB a committed file may have.  Every knot, both its float
neighbours and the special values are all kept; only the number of uniform draws is smaller, and tests/test_crf.py's shape cases add 200 003 further
draws checked against the restatement.
The cotangent of the gradients is tools/crf_restatement.py's `cotangent(N)`: multiples of 1/4, exact in float32, so it is not stored.
Per case k: weight_k, table_k = get_crf(), inv_k = get_inv_crf(), ldr_k = forward, ghdr_k and gweight_k = autograd of sum(ldr * cotangent),
hdr_k = inverse of the same inputs read as LDR, regs_k = (reg_weight, reg_monotonically_increasing, reg_smoothness), fit_k = cal_weight_fitting_crf(table).
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DIM, DRAWS_PER_BLOCK = 11, 8192


def make_inputs():
    x = torch.linspace(0, 1, 1024)
    lo, hi = torch.nextafter(x, torch.full_like(x, -1.0)), torch.nextafter(x, torch.full_like(x, 2.0))
    special = torch.tensor([0.0, 1.0, -0.0, -1e-30, -0.5, -3.0, 1.0 + 2.0 ** -23, 1.5, 7.0, 1e30, 0.5, 2.0 ** -149, 1.0 - 2.0 ** -24])
    knots = torch.cat([x, lo, hi, special])[:, None].repeat(1, 3)
    g = torch.Generator().manual_seed(0)
    rows = (DRAWS_PER_BLOCK + 2) // 3
    scalar = torch.rand(rows, 3, generator=g) * 1.4 - 0.1
    pixel = torch.rand(rows, 3, generator=g) * 1.4 - 0.1
    e_pixel = torch.rand(rows, 1, generator=g) * 1.5 + 0.5
    block = np.cumsum([0, len(knots), rows, rows]).astype(np.int64)
    return torch.cat([knots, scalar, pixel]), e_pixel, block


def import_reference(reference):
    from tools import crf_restatement
    for name in ("cv2", "kornia", "torchvision", "tinycudann"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torch_interpolations"] = crf_restatement
    tq = types.ModuleType("tqdm"); tq.tqdm = lambda it, *a, **k: it
    sys.modules.setdefault("tqdm", tq)
    sys.path.insert(0, reference)
    os.chdir(reference)
    from crf.model_crf import EmorCRF
    return EmorCRF, crf_restatement.cotangent, crf_restatement.by_block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "crf_emor.npz"))
    args = ap.parse_args()
    out_path = os.path.abspath(args.out)
    EmorCRF, cotangent, by_block = import_reference(os.path.abspath(args.reference))
    x, e_pixel, block = make_inputs()
    torch.manual_seed(0)
    big = 0.3 * torch.randn(3, DIM)
    weights = [torch.zeros(3, DIM), 0.05 * torch.randn(3, DIM), big]
    model = EmorCRF(dim=DIM)
    out = {"f0": model.f0.numpy().copy(), "basis": model.basis.numpy().copy(), "x": x.numpy(), "e_pixel": e_pixel.numpy(), "block": block,
           "n_cases": np.int64(len(weights))}
    min_diffs = []
    for k, w in enumerate(weights):
        model.weight = torch.nn.Parameter(w.clone())
        table = model.get_crf().detach()
        min_diffs.append(float((table[:, 1:] - table[:, :-1]).min()))
        h = x.clone().requires_grad_(True)
        ldr = by_block(model, h, e_pixel, block)
        g_hdr, g_weight = torch.autograd.grad((ldr * cotangent(len(x))).sum(), (h, model.weight))
        with torch.no_grad():
            inv = model.get_inv_crf()
            hdr = by_block(model.inverse, x, e_pixel, block)
            regs = torch.stack([model.reg_weight(), model.reg_monotonically_increasing(), model.reg_smoothness()])
        fit = model.cal_weight_fitting_crf(table.numpy())
        for name, v in (("weight", w), ("table", table), ("inv", inv), ("ldr", ldr.detach()), ("ghdr", g_hdr), ("gweight", g_weight), ("hdr", hdr),
                        ("regs", regs), ("fit", torch.as_tensor(fit))):
            out[f"{name}_{k}"] = v.numpy().astype(np.float32)
        assert np.isfinite(out[f"ldr_{k}"]).all() and np.isfinite(out[f"hdr_{k}"]).all() and np.isfinite(out[f"ghdr_{k}"]).all()
        print(f"case {k}: min difference {min_diffs[-1]:.4g}, regs {regs.tolist()}")
    assert min(min_diffs) < 0 and max(min_diffs) >= 0, "one case has to exercise the gap branch and one has to leave it alone"
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, os.path.getsize(out_path), "bytes,", len(x), "rows")


if __name__ == "__main__":
    main()
