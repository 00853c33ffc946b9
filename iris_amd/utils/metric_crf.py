"""python -m iris_amd.utils.metric_crf --crf_gt crf.npy --ckpt last_1.ckpt: the reference's utils/metric_crf.py (run by scripts/metric.sh) -- the L2
distance between the camera response recovered by the BRDF-CRF stage and the dataset's <LDR_IMG_DIR>/cam/crf.npy, both (3, 1024) curves.

The checkpoint's 'model_crf.' entries go into EmorCRF (stage.read_checkpoint, stage.load_crf; the reference hard-codes 3 basis curves: --crf_basis), the
predicted curves are get_crf(), and the printed number is np.linalg.norm(crf_gt - crf_pred).  --dir_save DIR writes the predicted curves as DIR/crf.npy.
The reference's matplotlib / plotly figures are dead code there (its two calls are commented out) and are not built.
"""
import os

import numpy as np

from .. import _lib as L
from .stage import exit_status

NAME = "metric_crf"


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="python -m iris_amd.utils.metric_crf: the reference's utils/metric_crf.py on MI355X")
    parser.add_argument("--crf_gt", type=str, required=True, help="path to LDR_IMG_DIR/cam/crf.npy")
    parser.add_argument("--ckpt", type=str, required=True, help="path to checkpoint last_1.ckpt")
    parser.add_argument("--crf_basis", type=int, default=3)
    parser.add_argument("--emor_path", type=str, default=None, help="the EMoR basis file (default: crf/emor.txt under the working directory, else the curves the checkpoint carries)")
    parser.add_argument("--dir_save", type=str, default=None, metavar="DIR", help="write the predicted curves to DIR/crf.npy")
    parser.add_argument("--device", type=int, default=0)
    return parser


def crf_l2(crf_gt, crf_pred):
    """metric_crf.py:49 -- np.linalg.norm(crf_gt - crf_pred) -- of two curve tables of one shape"""
    crf_gt, crf_pred = np.asarray(crf_gt), np.asarray(crf_pred)
    if crf_gt.shape != crf_pred.shape:
        raise L.IrisError(f"the ground-truth curves are {crf_gt.shape}, the checkpoint's {crf_pred.shape}")
    return float(np.linalg.norm(crf_gt - crf_pred))


def main(argv=None):
    import torch
    from . import stage
    args = build_parser().parse_args(argv)
    for path in (args.crf_gt, args.ckpt):
        if not os.path.isfile(path):
            raise L.IrisError(f"{path}: no such file")
    crf_gt = np.load(args.crf_gt)
    crf_state = stage.read_checkpoint(args.ckpt)["model_crf"]
    if not crf_state:
        raise L.IrisError(f"{args.ckpt}: the checkpoint holds no 'model_crf.' entry")
    device = stage.open_device(args.device, NAME)
    model_crf = stage.load_crf(crf_state, args.crf_basis, args.emor_path, device)
    with torch.no_grad():
        crf_pred = model_crf.get_crf().detach().cpu().numpy()
    print("L2: {:.5f}".format(crf_l2(crf_gt, crf_pred)))
    if args.dir_save:
        os.makedirs(args.dir_save, exist_ok=True)
        np.save(os.path.join(args.dir_save, "crf.npy"), crf_pred)
    return 0


def cli(argv=None):
    return exit_status(NAME, main, argv)


if __name__ == "__main__":
    raise SystemExit(cli())
