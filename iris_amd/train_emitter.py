"""The emitter training stage (reference: train_emitter.py) and, through iris_amd.initialize, the initialisation stage (initialize.py): the two stages
that train `emitter.radiance` through the one-bounce path tracer, and that write the checkpoints `extract_emitter_ldr --mode update` reads.

    python -m iris_amd.train_emitter --experiment_name EXP --dataset real DIR --ldr_img_dir ldr --voxel_path OUT/vslf.npz --emitter_path OUT/emitter.pth \
        --ckpt_path checkpoints/EXP/last_0.ckpt --SPP 128 --spp 32 --max_epochs 1 --checkpoint_path checkpoints --log_path logs

takes the reference's arguments (configs/config.py and train_emitter.py:390-403).  One class, RadianceTrainer, runs both stages:

  mode 'emitter'     train_emitter.py:158-216.  Material network and response model come from --ckpt_path and are frozen; the only trainable tensor is
                     emitter.radiance.  A step is L_sum = path_tracing_single_step(scene, emitter, material, xs, ds, dxdu, dydv, spp, SPP // spp), then
                     photometric_loss(L_sum, SPP // spp, ...): loss = loss_c.  Logged: train/loss, train/loss_c, train/psnr.
  mode 'initialize'  initialize.py:150-225.  The response model is EmorCRF(dim=crf_basis) at its defaults, frozen; the material network is trained through
                     the albedo term alone: mat = material(the jittered primary hit's positions) with grad, the integrator run with the network's
                     parameters switched to requires_grad = False (:170-186), loss = segment_albedo_loss(albedo, int_albedo, segmentation) + loss_c.
                     Logged: init/loss, init/loss_c, init/loss_a, init/psnr.  The optimizer holds the material parameters and emitter.radiance.

The batches come from a PixelSet(..., ray_diff=True) after restrict_to_hits(scene): all-valid and of a fixed size, in place of the reference's per-step
`valid` filter (the BRDF-CRF stage's documented deviation).  The photometric term, with the response model frozen in both stages, is one
call that returns the loss, the psnr and the gradient by L_sum (iris_amd.utils.losses.photometric_loss).  The loop, the schedule, metrics.jsonl and
last.ckpt are iris_amd/utils/trainer.py's; the checkpoint holds `material.*` and `model_crf.*` (in the emitter mode: as loaded, so the file serves
slf_refine, refine_shading and render as the reference's does) and `emitter.radiance`.

`--validate metric|images|all` (an addition; default none) turns on the reference's validation (validation_step, validation() and the val/loss-monitored
checkpoint; iris_amd/utils/validation.py): val/loss and val/psnr over the validation views after every epoch with `best.ckpt` beside last.ckpt, and the
validation images of view --val_frame every --val_step steps under outputs/<experiment_name>/<dir_val>/, rendered under the emitter being trained.

Not built: the validation images' crfs.png and crfs_weight.png (matplotlib), TensorBoard / W&B logging (the scalars go to metrics.jsonl under the
reference's names), the synthetic layout's `albedo` / `roughness` ground-truth scalars, the `Ranger` optimizer, `--res_scale` other than 1 for the real
and synthetic layouts (the scannetpp layout takes any: its 8-bit files are resized on the device, iris_amd/utils/resize.py); `--num_workers` is accepted
and ignored, and so are `--val_step`, `--dir_val` and `--val_frame` without --validate.
"""
import argparse
import os

import torch
import torch.nn.functional as NF

from . import _lib as L
from .utils import stage, trainer as base
from .utils.stage import read_checkpoint
from .utils.trainer import DEFAULT_OPTIONS, make_optimizer, multistep_lr          # noqa: F401  (where tools and tests look for them)

PROGRAM_DEFAULTS = base.PROGRAM_DEFAULTS          # (--emor_path is the command line's, not a hyper-parameter)
MODES = {"emitter": ("train", ("loss", "loss_c", "psnr")),                       # train_emitter.py:206-208
         "initialize": ("init", ("loss", "loss_c", "loss_a", "psnr"))}           # initialize.py:214-217


def default_hparams(**changes):
    """a plain dict of every option with its default"""
    return base.default_hparams(PROGRAM_DEFAULTS, **changes)


class RadianceTrainer(base.Trainer):
    """scene: the Scene of the mesh; emitter: an SLFEmitterLearn; material: an NGPBRDF (loaded, or init_parameters() in mode 'initialize'); model_crf: an
    EmorCRF; all on the pixel set's device (the emitter is moved there).  pixel_set: a PixelSet(ray_diff=True) with exposure (and, in mode 'initialize',
    segmentation and int_albedo) that has been through restrict_to_hits(scene).  hparams: a dict or Namespace of options (default_hparams()).
    mode: 'emitter' | 'initialize' (the module docstring).  validation: the utils.validation.ValidationSet of hparams['validate'], or None; its images are
    rendered under `emitter`.
    training_step(batch) -> dict of 0-d device tensors under the names the mode logs; the checkpoint also holds `emitter.radiance`; everything else is
    utils.trainer.Trainer's."""

    def __init__(self, scene, emitter, material, model_crf, pixel_set, hparams, mode, validation=None):
        if mode not in MODES:
            raise L.IrisError(f"RadianceTrainer: mode {mode!r}, expected 'emitter' or 'initialize'")
        super().__init__(pixel_set, hparams, PROGRAM_DEFAULTS, validation=validation)
        hp, self.mode, self.scene, self.emitter, self.material, self.model_crf = self.hparams, mode, scene, emitter, material, model_crf
        self.prefix, self.logged = MODES[mode]
        self.spp = int(hp["spp"])
        self.n_calls = int(hp["SPP"]) // max(self.spp, 1)
        if self.spp < 1 or self.n_calls < 1:
            raise L.IrisError(f"RadianceTrainer: --SPP {hp['SPP']} --spp {hp['spp']}: expected 1 <= spp <= SPP (a step traces SPP // spp calls of spp samples)")
        if not pixel_set.ray_diff or pixel_set.kept is None:
            raise L.IrisError("RadianceTrainer: the pixel set needs ray_diff=True and restrict_to_hits(scene)")
        if pixel_set.exposure is None or (mode == "initialize" and (pixel_set.segmentation is None or pixel_set.int_albedo is None)):
            raise L.IrisError("RadianceTrainer: the pixel set needs exposure (and, in mode 'initialize', segmentation and int_albedo)")
        if not hasattr(emitter, "radiance") or not isinstance(emitter.radiance, torch.nn.Parameter):
            raise L.IrisError("RadianceTrainer: the emitter has no trainable `radiance` (expected an SLFEmitterLearn)")
        dev = pixel_set.device
        p = material.mlp.params
        if not p.is_cuda or p.device != dev or model_crf.weight.device != dev:
            raise L.IrisError(f"RadianceTrainer: material ({p.device}), model_crf ({model_crf.weight.device}) and the pixel set ({dev}) must share a HIP device")
        emitter.to(dev)
        model_crf.weight.requires_grad_(False)                                   # train_emitter.py:94-95, initialize.py:86-87
        p.requires_grad_(mode == "initialize")                                   # train_emitter.py:75-76
        emitter.radiance.requires_grad_(True)
        self._start(([p] if mode == "initialize" else []) + [emitter.radiance], networks=[material] if mode == "initialize" else [])

    def _extra_state(self):
        return {"radiance": self.emitter.radiance}

    def _load_extra(self, ck, path):
        if "radiance" not in ck["emitter"]:
            raise L.IrisError(f"{path}: the checkpoint's state_dict has no 'emitter.radiance': it was not written by this stage")
        with torch.no_grad():
            self.emitter.radiance.copy_(ck["emitter"]["radiance"])

    @staticmethod
    def _rays(batch):
        rays = batch["rays"]
        return rays[:, :3].contiguous(), NF.normalize(rays[:, 3:6], dim=-1), rays[:, 6:9].contiguous(), rays[:, 9:12].contiguous()

    def jittered_positions(self, batch):
        """initialize.py:158-160: the hit positions of the batch's rays jittered by du, dv in [-0.5, 0.5), one sample each (the step's first draw)"""
        from .utils.path_tracing import jittered_primary_hit
        xs, ds, dxdu, dydv = self._rays(batch)
        dudv = torch.rand(2, xs.shape[0], 1, device=xs.device)                   # (iris_pt_primary subtracts the 0.5)
        return jittered_primary_hit(self.scene, self.emitter, xs, ds, dxdu, dydv, dudv)["position"]

    def _photometric(self, batch):
        from .utils.losses import photometric_loss
        from .utils.path_tracing import path_tracing_single_step
        xs, ds, dxdu, dydv = self._rays(batch)
        L_sum = path_tracing_single_step(self.scene, self.emitter, self.material, xs, ds, dxdu, dydv, self.spp, self.n_calls)
        return photometric_loss(L_sum, self.n_calls, crf=self.model_crf, exposure=batch["exposure"], rgbs_gt=batch["rgbs"])

    def training_step(self, batch, global_step=None):
        """train_emitter.py:158-216 / initialize.py:150-225 on an all-valid batch -> {'loss', 'loss_c', 'psnr'} (and 'loss_a' in mode 'initialize')"""
        if self.mode == "emitter":
            out = self._photometric(batch)
            return dict(loss=out["loss_c"], loss_c=out["loss_c"], psnr=out["psnr"])
        from .utils.losses import segment_albedo_loss
        p = self.material.mlp.params
        albedo = self.material(self.jittered_positions(batch))["albedo"]
        p.requires_grad_(False)                                                  # only the emitter is optimised through the integrator (:170-186)
        try:
            out = self._photometric(batch)
        finally:
            p.requires_grad_(True)
        loss_a = segment_albedo_loss(albedo, batch["int_albedo"], batch["segmentation"], weight=1.0, scale_invariant=False)
        return dict(loss=loss_a + out["loss_c"], loss_c=out["loss_c"], loss_a=loss_a, psnr=out["psnr"])


# ---- the command line (shared with iris_amd.initialize)
def parser(prog="train_emitter", description="the emitter training stage"):
    ap = argparse.ArgumentParser(prog="python -m iris_amd." + prog, description=description)
    base.add_trainer_options(ap)
    stage.add_common_options(ap, "emor_path")
    return ap


def cli_parser(prog="train_emitter", description="the emitter training stage"):
    """parser() and --validate: what main() parses.  They stand apart because parser()'s option table is pinned option for option
    (tests/test_stage_setup_cpu.py) as the table the stage had before it validated."""
    return base.add_validate_option(parser(prog, description))


def run(args, mode, stage_name):
    """main() of both stages: refuse, open the device, load, train"""
    from .model.brdf import NGPBRDF
    from .model.crf import EmorCRF
    from .model.emitter import SLFEmitterLearn
    val_files = stage.refuse_unbuilt_training(args)   # everything that can be refused is refused before the device is touched
    if not args.emitter_path:
        raise L.IrisError("--emitter_path is needed: the emitter.pth of python -m iris_amd.extract_emitter_ldr, whose radiance this stage trains")
    if not args.voxel_path or not os.path.isfile(args.voxel_path):
        raise L.IrisError(f"--voxel_path {args.voxel_path}: the vslf.npz of python -m iris_amd.slf_bake is needed (the radiance cache and the material network's range)")
    if not os.path.isfile(args.emitter_path):
        raise L.IrisError(f"--emitter_path {args.emitter_path}: no such file")
    if mode == "emitter" and not args.ckpt_path:
        raise L.IrisError("--ckpt_path is needed: the stage trains the emitters under the material network and the response model of a BRDF-CRF checkpoint "
                          "(python -m iris_amd.train_brdf_crf)")
    if int(args.spp) < 1 or int(args.SPP) // int(args.spp) < 1:
        raise L.IrisError(f"--SPP {args.SPP} --spp {args.spp}: expected 1 <= spp <= SPP (a step traces SPP // spp calls of spp samples)")
    if getattr(args, "validate", "none") == "none":
        print(f"{stage_name}: --val_step, --num_workers, --dir_val and --val_frame are accepted and ignored (no in-training validation images, no loader "
              "workers: the batches are made on the device)", flush=True)
    else:
        print(base.validation_notice(stage_name, args, val_files), flush=True)
    device = stage.open_device(args.device, stage_name)
    files, scene, ps, n = stage.open_training_set(args, device, ray_diff=True)
    material = NGPBRDF(*stage.voxel_range(args.voxel_path))
    ck = read_checkpoint(args.ckpt_path) if args.ckpt_path else None
    if mode == "emitter":
        material.load_state_dict(ck["material"])
        model_crf = stage.load_crf(ck["model_crf"], args.crf_basis, args.emor_path, device)
    else:
        material.init_parameters()
        if ck is not None:
            material.load_state_dict(ck["material"])
        model_crf = EmorCRF(dim=args.crf_basis, emor_path=args.emor_path).to(device)        # at its defaults (initialize.py:85)
    material.to(device)
    emitter = SLFEmitterLearn(args.emitter_path, args.voxel_path).to(device)
    validation = None
    if val_files is not None:
        from .utils.validation import ValidationSet
        validation = ValidationSet.load(val_files, scene, device)
    trainer = RadianceTrainer(scene, emitter, material, model_crf, ps, args, mode, validation=validation)
    print(f"{stage_name}: {len(files['views'])} views of {files['img_hw'][0]} x {files['img_hw'][1]}, {n} pixels on the mesh, {len(ps)} steps per epoch of "
          f"{trainer.n_calls} x {trainer.spp} samples; starting at epoch {trainer.epoch}, step {trainer.global_step}", flush=True)
    trainer.fit(args.max_epochs)
    last = next((e for e in reversed(trainer.history) if trainer.prefix + "/loss" in e), {})
    print(f"{stage_name}: {trainer.epoch} epochs, {trainer.global_step} steps; last logged loss {last.get(trainer.prefix + '/loss')}; checkpoint {trainer.ckpt_file}",
          flush=True)
    if trainer.best is not None:
        print(f"{stage_name}: best val/loss {trainer.best['val/loss']} after epoch {trainer.best['epoch']}; checkpoint {trainer.best_file}", flush=True)
    return 0


def main(argv=None):
    return run(cli_parser().parse_args(argv), "emitter", "train_emitter")


def cli(argv=None):
    return stage.exit_status("train_emitter", main, argv)


if __name__ == "__main__":
    raise SystemExit(cli())
