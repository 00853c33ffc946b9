"""``python -m iris_amd.slf_refine``: the reference's slf_refine.py command.  Loads <output>/<load>, pools the train split's photographs anew through the
checkpoint's response model into the same voxel grid (iris_amd.slf_bake.refine_slf, one fused launch per view) and writes <output>/<save>."""
import os

import torch

from . import _lib as L
from .slf_bake import add_prebake_options, open_prebake, refine_slf
from .utils.stage import exit_status


def parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m iris_amd.slf_refine", description="re-pool vslf.npz with the trained response model")
    add_prebake_options(ap)
    ap.add_argument("--load", type=str, default="vslf.npz")
    ap.add_argument("--save", type=str, default="vslf.npz")
    ap.add_argument("--voxel_num", type=int, default=256, help="(accepted, unused: the grid is the loaded file's, as in the reference)")
    ap.add_argument("--ckpt", type=str, help="checkpoint to load CRF model")
    ap.add_argument("--crf_basis", type=int, help="number of CRF basis")
    return ap


def main(argv=None):
    from .model.crf import EmorCRF
    from .utils import stage
    from .utils.path_tracing import load_scene
    args = parser().parse_args(argv)
    mesh, img_hw, views, photographs = open_prebake(args, "slf_refine", need_exposure=True)
    if args.crf_basis is None:
        raise L.IrisError("--crf_basis is needed: the number of EMoR basis curves of the response model (the reference's EmorCRF(args.crf_basis))")
    # model_crf.* of the checkpoint; without --ckpt the fresh model's own state: zero weights (slf_refine.py:72-79)
    crf_state = stage.read_checkpoint(args.ckpt)["model_crf"] if args.ckpt else EmorCRF(args.crf_basis, emor_path=args.emor_path).state_dict()
    state = stage.load_pickled(os.path.join(args.output, args.load))
    device = stage.open_device(args.device, "slf_refine")
    model_crf = stage.load_crf(crf_state, args.crf_basis, args.emor_path, device)
    scene = load_scene(mesh, device=device)
    batches = stage.photograph_batches(views, img_hw, photographs, device, resize=stage.layout_resizes(args.dataset, args.cameras))
    out = refine_slf(state, scene, batches, device=device, crf=model_crf)
    torch.save(out, os.path.join(args.output, args.save))
    print(f"slf_refine: {len(views)} views, {int(out['weight']['count'].sum())} hits pooled -> {os.path.join(args.output, args.save)}", flush=True)
    return 0


def cli(argv=None):
    return exit_status("slf_refine", main, argv)


if __name__ == "__main__":
    raise SystemExit(cli())
