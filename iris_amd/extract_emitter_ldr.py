"""``python -m iris_amd.extract_emitter_ldr``: the reference's extract_emitter_ldr.py command.

  --mode export   the raw LDR values of the train split's photographs pooled per triangle (no response model), thresholded -> <output>/emitter.pth
                  (iris_amd.slf_bake.extract_emitters, one fused launch per view)
  --mode update   host only: emitter.pth's 'emitter_radiance' <- the checkpoint's 'emitter.radiance' (extract_emitter_ldr.py:117-122)
  --mode test     accepted; does nothing, as in the reference
"""
import os

import torch

from . import _lib as L
from .slf_bake import add_prebake_options, extract_emitters, open_prebake
from .utils.stage import exit_status


def parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m iris_amd.extract_emitter_ldr", description="find the emitter triangles from the LDR photographs")
    add_prebake_options(ap)
    ap.add_argument("--mode", type=str, default="export", choices=["export", "update", "test"])
    ap.add_argument("--ckpt", type=str, help="checkpoint path")
    ap.add_argument("--spp", type=int, default=100, help="(accepted, unused, as in the reference)")
    ap.add_argument("--threshold", type=float, default=0.99, help="threshold for emitter")
    return ap


def update(output, ckpt):
    """mode 'update': no device is opened"""
    from .utils import stage
    if not ckpt:
        raise L.IrisError("--mode update needs --ckpt")
    state = stage.load_pickled(ckpt)["state_dict"]
    if "emitter.radiance" not in state:
        raise L.IrisError(f"{ckpt}: the checkpoint's state_dict has no 'emitter.radiance' (an emitter-training checkpoint carries it; the checkpoints "
                          "python -m iris_amd.train_brdf_crf writes do not)")
    path = os.path.join(output, "emitter.pth")
    emitter = stage.load_pickled(path)
    emitter["emitter_radiance"] = state["emitter.radiance"]
    torch.save(emitter, path)
    return path


def main(argv=None):
    from .utils import stage
    from .utils.path_tracing import Scene, load_mesh
    args = parser().parse_args(argv)
    if args.mode == "update":
        print(f"extract_emitter_ldr: emitter_radiance updated in {update(args.output, args.ckpt)}", flush=True)
        return 0
    if args.mode == "test":
        return 0
    mesh, img_hw, views, photographs = open_prebake(args, "extract_emitter_ldr", need_exposure=False)
    vertices, faces = load_mesh(mesh)
    device = stage.open_device(args.device, "extract_emitter_ldr")
    scene = Scene(vertices, faces, device=device)
    batches = stage.photograph_batches(views, img_hw, photographs, device, resize=stage.layout_resizes(args.dataset, args.cameras))
    out = extract_emitters(scene, vertices, faces, batches, args.threshold, device=device)
    os.makedirs(args.output, exist_ok=True)
    torch.save(out, os.path.join(args.output, "emitter.pth"))
    print(f"extract_emitter_ldr: {len(views)} views, {int(out['is_emitter'].sum())} of {len(faces)} triangles emit -> {os.path.join(args.output, 'emitter.pth')}", flush=True)
    return 0


def cli(argv=None):
    return exit_status("extract_emitter_ldr", main, argv)


if __name__ == "__main__":
    raise SystemExit(cli())
