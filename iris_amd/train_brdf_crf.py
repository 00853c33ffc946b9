"""The BRDF-CRF training stage (reference: train_brdf_crf.py): the stage that writes the checkpoint `render`, `render_relight`, `refine_shading` and
`utils.export` load with --ckpt.

    python -m iris_amd.train_brdf_crf --experiment_name EXP --dataset real DIR --ldr_img_dir ldr --voxel_path OUT/vslf.npz --cache_dir OUT/shading \
        --max_epochs 2 --checkpoint_path checkpoints --log_path logs

takes the reference's arguments (configs/config.py and train_brdf_crf.py:511-531).  A step is `brdf_crf_loss(material(batch['positions']), ...)` on a
`PixelSet` batch (every view traced once at construction: `restrict_to_hits`), `backward`, and `FusedAdam` -- the Adam update of the 27 963 328 material
parameters and the refresh of the half copy the forward reads, in one pass (iris_amd/utils/optim.py).  The loop, the schedule, metrics.jsonl and
`<checkpoint_path>/<experiment_name>/last.ckpt` (`['state_dict']` with `material.*` and `model_crf.*` keys, as the reference's loaders read it) are
iris_amd/utils/trainer.py's.

`--validate metric|images|all` (an addition; default none) turns on the reference's validation (train_brdf_crf.py:331-499,539; iris_amd/utils/validation.py):
val/loss and val/psnr over the validation views after every epoch with `best.ckpt` beside last.ckpt, and the validation images of view --val_frame every
--val_step steps under outputs/<experiment_name>/<dir_val>/.  The images are path-traced, so `--validate images|all` also needs --emitter_path (emitter.pth;
the radiance cache is --voxel_path's), which this stage does not otherwise read.

Not built: the validation images' crfs.png and crfs_weight.png (matplotlib), TensorBoard / W&B logging (the scalars go to metrics.jsonl under the
reference's names), the `Ranger` optimizer, `--res_scale` other than 1 for the real and synthetic layouts (`--dataset scannetpp ROOT --scene S` takes any:
its 8-bit files are resized on the device, iris_amd/utils/resize.py); `--num_workers` is accepted and ignored, and so is `--val_step` without --validate.
"""
import argparse
import os

from . import _lib as L
from .utils import stage, trainer as base
from .utils.stage import read_checkpoint, write_checkpoint          # noqa: F401  (where tools and tests look for them)
from .utils.trainer import DEFAULT_OPTIONS, make_optimizer, multistep_lr          # noqa: F401  (likewise)

PROGRAM_DEFAULTS = dict(base.PROGRAM_DEFAULTS, cache_dir=None)


def default_hparams(**changes):
    """a plain dict of every option with its default"""
    return base.default_hparams(PROGRAM_DEFAULTS, **changes)


class BRDFCRFTrainer(base.Trainer):
    """material: an NGPBRDF on the GPU (init_parameters() or loaded); model_crf: an EmorCRF on the same device; pixel_set: a PixelSet with its cache attached
    that has been through restrict_to_hits(scene, store_positions=True); hparams: a dict or Namespace of options (default_hparams()); validation: the
    utils.validation.ValidationSet of hparams['validate'] (with its own emitter when images are written), or None.
    training_step(batch, global_step) -> brdf_crf_loss's dict; everything else is utils.trainer.Trainer's."""
    prefix, logged = "train", ("loss", "loss_c", "loss_d", "loss_seg", "loss_a", "psnr")          # train_brdf_crf.py:324-329, as 'train/<name>'

    def __init__(self, material, model_crf, pixel_set, hparams, validation=None):
        super().__init__(pixel_set, hparams, PROGRAM_DEFAULTS, validation=validation)
        hp, self.material, self.model_crf = self.hparams, material, model_crf
        if pixel_set.cache is None or pixel_set.positions is None:
            raise L.IrisError("BRDFCRFTrainer: the pixel set needs attach_cache(cache) and restrict_to_hits(scene, store_positions=True)")
        if pixel_set.segmentation is None or pixel_set.exposure is None or (hp["la"] > 0 and pixel_set.int_albedo is None):
            raise L.IrisError("BRDFCRFTrainer: the pixel set needs segmentation and exposure (and int_albedo when la > 0)")
        p = material.mlp.params
        if not p.is_cuda or p.device != pixel_set.device or model_crf.weight.device != p.device:
            raise L.IrisError(f"BRDFCRFTrainer: material ({p.device}), model_crf ({model_crf.weight.device}) and the pixel set ({pixel_set.device}) must share a HIP device")
        p.requires_grad_(True)
        model_crf.weight.requires_grad_(not hp["freeze_crf"])
        self._start([p] + ([] if hp["freeze_crf"] else [model_crf.weight]), networks=[material])

    def training_step(self, batch, global_step):
        """train_brdf_crf.py:163-337 on an all-valid batch -> {'loss', 'loss_c', 'loss_d', 'loss_seg', 'loss_a', 'reg_crf', 'psnr'}, device tensors"""
        from .utils.losses import brdf_crf_loss
        hp, m = self.hparams, self.material
        return brdf_crf_loss(m(batch["positions"]), cache=self.ps.cache, idx=batch["idx"], crf=self.model_crf, exposure=batch["exposure"], rgbs_gt=batch["rgbs"],
                             segmentation=batch["segmentation"], positions=batch["positions"], albedo_prior=batch["int_albedo"], has_part=hp["has_part"],
                             ld=hp["ld"], lp=hp["lp"], ls=hp["ls"], la=hp["la"], sigma_albedo=hp["sigma_albedo"], sigma_pos=hp["sigma_pos"],
                             l_crf_increasing=hp["l_crf_increasing"], l_crf_weight=hp["l_crf_weight"], seed=global_step, voxel_min=m.voxel_min,
                             voxel_max=m.voxel_max)


# ---- the command line
def parser():
    ap = argparse.ArgumentParser(prog="python -m iris_amd.train_brdf_crf", description="the BRDF-CRF training stage")
    base.add_trainer_options(ap)
    ap.add_argument("--cache_dir", type=str)
    return ap


def cli_parser():
    """parser() and --validate: what main() parses.  They stand apart because parser()'s option table is pinned option for option
    (tests/test_stage_setup_cpu.py) as the table the stage had before it validated."""
    return base.add_validate_option(parser())


def main(argv=None):
    args = cli_parser().parse_args(argv)
    from .model.brdf import NGPBRDF
    from .model.crf import EmorCRF
    val_files = stage.refuse_unbuilt_training(args)   # everything that can be refused is refused before the device is touched
    if args.cache_dir is None:
        raise L.IrisError("--cache_dir is needed: the stage trains on the baked shadings (python -m iris_amd.bake_shading --output DIR)")
    images = args.validate in ("images", "all")
    if images:
        if not args.emitter_path:
            raise L.IrisError(f"--validate {args.validate} needs --emitter_path (emitter.pth): the validation images are path-traced under the emitter, "
                              "which this stage does not otherwise load")
        for path in (args.emitter_path, args.voxel_path):
            if not path or not os.path.isfile(path):
                raise L.IrisError(f"{path}: no such file (--validate {args.validate} reads --emitter_path and --voxel_path)")
    if args.validate == "none":
        print("train_brdf_crf: --val_step and --num_workers are accepted and ignored (no in-training validation images, no loader workers: the batches are "
              "made on the device)", flush=True)
    else:
        print(base.validation_notice("train_brdf_crf", args, val_files), flush=True)
    device = stage.open_device(args.device, "train_brdf_crf")
    files, scene, ps, n = stage.open_training_set(args, device, cache_dir=args.cache_dir)
    validation = None
    if val_files is not None:
        from .utils.validation import ValidationSet
        emitter = None
        if images:
            from .model.emitter import SLFEmitter
            emitter = SLFEmitter(args.emitter_path, args.voxel_path).to(device)
            stage.freeze(emitter)
        validation = ValidationSet.load(val_files, scene, device, emitter=emitter)
    material = NGPBRDF(*stage.voxel_range(args.voxel_path)).init_parameters()
    model_crf = EmorCRF(dim=args.crf_basis)
    if args.ckpt_path:
        ck = read_checkpoint(args.ckpt_path)
        material.load_state_dict(ck["material"])
        if args.load_crf:
            model_crf.load_state_dict(ck["model_crf"])
    material.to(device)
    model_crf.to(device)
    trainer = BRDFCRFTrainer(material, model_crf, ps, args, validation=validation)
    print(f"train_brdf_crf: {len(files['views'])} views of {files['img_hw'][0]} x {files['img_hw'][1]}, {n} pixels on the mesh, {len(ps)} steps per epoch; "
          f"starting at epoch {trainer.epoch}, step {trainer.global_step}", flush=True)
    trainer.fit(args.max_epochs)
    last = next((e for e in reversed(trainer.history) if "train/loss" in e), {})
    print(f"train_brdf_crf: {trainer.epoch} epochs, {trainer.global_step} steps; last logged loss {last.get('train/loss')}; checkpoint {trainer.ckpt_file}", flush=True)
    if trainer.best is not None:
        print(f"train_brdf_crf: best val/loss {trainer.best['val/loss']} after epoch {trainer.best['epoch']}; checkpoint {trainer.best_file}", flush=True)
    return 0


def cli(argv=None):
    return stage.exit_status("train_brdf_crf", main, argv)


if __name__ == "__main__":
    raise SystemExit(cli())
