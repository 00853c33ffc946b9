"""What the three training stages (train_brdf_crf, train_emitter, initialize) share: the option table of configs/config.py, the program options their
command lines register, the learning-rate schedule, the optimizer choice, and `Trainer`, the loop with its logging, checkpoints and --resume.
Host code: it imports and runs without a GPU (a subclass's constructor checks the devices of what it is given).
"""
import argparse
import json
import math
import os

import torch

from .. import _lib as L
from .stage import read_checkpoint, write_checkpoint          # (the checkpoint's layout lives with its other readers)

# configs/config.py, option by option
DEFAULT_OPTIONS = {
    "batch_size": dict(type=int, default=1024 * 8),
    "dataset": dict(type=str, nargs=2, default=["synthetic", "../data/indoor_synthetic/kitchen"]),
    "scene": dict(type=str, default=""),
    "voxel_path": dict(type=str, default="outputs/kitchen/vslf.npz"),
    "num_workers": dict(type=int, default=12),
    "dir_val": dict(type=str, default="val"),
    "val_step": dict(type=int, default=250),
    "has_part": dict(type=int, default=1),
    "res_scale": dict(type=float, default=1.0),
    "optimizer": dict(type=str, choices=["SGD", "Ranger", "Adam"], default="Adam"),
    "learning_rate": dict(type=float, default=1e-3),
    "weight_decay": dict(type=float, default=0),
    "scheduler_rate": dict(type=float, default=0.5),
    "milestones": dict(type=int, nargs="*", default=[1000]),
    "le": dict(type=float, default=1.0),
    "ld": dict(type=float, default=5e-4),
    "lp": dict(type=float, default=5e-3),
    "ls": dict(type=float, default=1e-3),
    "la": dict(type=float, default=0.0),
    "sigma_albedo": dict(type=float, default=0.05 / 3.0),
    "sigma_pos": dict(type=float, default=0.3 / 3.0),
    "ckpt_path": dict(type=str, default=None),
    "emitter_path": dict(type=str, default=None),
    "freeze_emitter": dict(type=int, default=0),
    "freeze_crf": dict(type=int, default=0),
    "indir_depth": dict(type=int, default=5),
    "SPP": dict(type=int, default=512),
    "spp": dict(type=int, default=8),
    "ldr_img_dir": dict(type=str, default=None),
    "crf_basis": dict(type=int, default=3),
    "load_crf": dict(type=int, default=0),
    "l_crf_increasing": dict(type=float, default=0.1),
    "l_crf_weight": dict(type=float, default=0.001),
}
# train_brdf_crf.py:517-526 and train_emitter.py:396-403, and what the trainers here add; a stage with an option of its own extends the dict
PROGRAM_DEFAULTS = dict(experiment_name=None, max_epochs=500, log_path="./logs", checkpoint_path="./checkpoints", resume=False, device=0, val_frame=0,
                        log_every=50, validate="none")
VALIDATE_MODES = ("none", "metric", "images", "all")


def add_validate_option(parser):
    """--validate: what a trainer's cli_parser() adds to its parser() (whose option table is pinned as it was before the trainers validated)"""
    parser.add_argument("--validate", type=str, default=PROGRAM_DEFAULTS["validate"], choices=VALIDATE_MODES,
                        help="metric: val/loss and val/psnr over the validation views after every epoch (metrics.jsonl) and best.ckpt, the epoch of the lowest "
                             "val/loss; images: the validation images of view --val_frame every --val_step steps under outputs/<experiment_name>/<dir_val>; "
                             "all: both; none (default): neither")
    return parser


def validation_notice(stage_name, args, files):
    """the line a trainer prints, under --validate other than none, where it otherwise says that the validation options are ignored"""
    parts = []
    if args.validate in ("metric", "all"):
        parts.append(f"val/loss and val/psnr over {len(files['views'])} validation views of {files['img_hw'][0]} x {files['img_hw'][1]} after every epoch "
                     "(metrics.jsonl), best.ckpt and best.json beside last.ckpt")
    if args.validate in ("images", "all"):
        parts.append(f"the validation images of view {args.val_frame} every {args.val_step} steps under "
                     f"{os.path.join('outputs', args.experiment_name, args.dir_val)} ({int(args.SPP) // int(args.spp)} rounds of {args.spp} samples)")
    return f"{stage_name}: --validate {args.validate}: " + "; ".join(parts) + "; --num_workers is accepted and ignored (the batches are made on the device)"


def add_trainer_options(parser):
    """configs/config.py's options, then the program options all three command lines register; a stage adds --cache_dir or --emor_path after the call"""
    for name, o in DEFAULT_OPTIONS.items():
        parser.add_argument("--" + name, **o)
    parser.add_argument("--experiment_name", type=str, required=True)
    parser.add_argument("--max_epochs", type=int, default=PROGRAM_DEFAULTS["max_epochs"])
    parser.add_argument("--log_path", type=str, default=PROGRAM_DEFAULTS["log_path"])
    parser.add_argument("--ft", type=str, default=None)
    parser.add_argument("--checkpoint_path", type=str, default=PROGRAM_DEFAULTS["checkpoint_path"])
    parser.add_argument("--resume", dest="resume", action="store_true")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--val_frame", type=int, default=0)
    parser.add_argument("--log_every", type=int, default=PROGRAM_DEFAULTS["log_every"], help="read and write the step's scalars every this many steps")
    parser.set_defaults(resume=False)


def default_hparams(program_defaults, **changes):
    """a plain dict of every option with its default"""
    hp = {name: (list(o["default"]) if isinstance(o["default"], list) else o["default"]) for name, o in DEFAULT_OPTIONS.items()}
    hp.update(program_defaults)
    unknown = set(changes) - set(hp)
    if unknown:
        raise KeyError(f"unknown options {sorted(unknown)}")
    hp.update(changes)
    return hp


def multistep_lr(lr0, milestones, gamma, epoch):
    """torch.optim.lr_scheduler.MultiStepLR stepped once per epoch: lr0 * gamma^(number of milestones <= epoch)"""
    return lr0 * gamma ** sum(1 for m in milestones if m <= epoch)


def make_optimizer(name, params, lr, weight_decay, networks):
    """train_brdf_crf.py:106-112.  Adam is the fused step; SGD is torch's, over the forward's own parameter refresh"""
    if name == "Adam":
        from .optim import FusedAdam
        return FusedAdam(params, lr=lr, weight_decay=weight_decay, networks=networks)
    if name == "SGD":
        return torch.optim.SGD(params, lr=lr, weight_decay=weight_decay)
    if name == "Ranger":
        raise L.IrisError("--optimizer Ranger is not built (the reference lists it but constructs only SGD and Adam): use Adam or SGD")
    raise L.IrisError(f"--optimizer {name}: expected Adam or SGD")


class Trainer:
    """The loop of every training stage.  A subclass sets `material` (its `mlp.params` is the tensor the checkpoint restores in place), `model_crf`, `prefix`
    and `logged` (the step's scalars go to the log as '<prefix>/<name>'; 'loss' is one of them), ends its constructor with `_start(params, networks)`
    and defines `training_step(batch, global_step)` -> dict of 0-d tensors holding at least the logged names.  What it adds to the checkpoint goes
    through `_extra_state` and `_load_extra`.

    fit(max_epochs) runs the epochs: the learning rate of the epoch (MultiStepLR under Lightning's default interval), resample, then zero_grad / backward /
    step per batch.  The logged scalars stay on their device; every `log_every` steps that step's are read in ONE synchronisation, appended to
    `<log_path>/<experiment_name>/metrics.jsonl` and to `self.history`; a non-finite loss at such a read raises FloatingPointError with the step number.
    `<checkpoint_path>/<experiment_name>/last.ckpt` is written at the end of every epoch, `epoch` counting the completed ones; with hparams['resume'] and
    that file in place the constructor restores parameters, optimizer state, epoch and global step from it, and the run continues as a straight one.

    Validation (train_brdf_crf.py:331-499,539): `validation` is an object with `evaluate(scene, material)` -> {'val/loss', 'val/psnr'} (0-d tensors or
    numbers) and `write_images(folder, step, frame, material, model_crf, SPP, spp, emitter=None)` (utils.validation.ValidationSet); hparams['validate']
    says what is done with it.  'none' (the default): nothing -- the same files, log lines and output as a trainer without the object.  'metric' / 'all':
    after every epoch's last.ckpt one line {'step', 'epoch', 'val/loss', 'val/psnr'} goes to metrics.jsonl and `history` ('step' and 'epoch' count the
    completed ones, as the checkpoint does), and when val/loss is STRICTLY below the best so far the same checkpoint is written as `best.ckpt` beside
    last.ckpt -- one fixed name where Lightning's ModelCheckpoint(monitor='val/loss', save_top_k=1) writes epoch=E-step=S.ckpt -- with `best.json`
    {'val/loss', 'epoch', 'step'}, which --resume reads back.  'images' / 'all': before every step with global_step % val_step == 0, step 0 included,
    the validation images of view val_frame are written to outputs/<experiment_name>/<dir_val>/ under the working directory.  Lightning's two-batch
    sanity check before training is not reproduced."""

    def __init__(self, pixel_set, hparams, program_defaults, validation=None):
        """hparams: a dict or Namespace of options; what is not among default_hparams(program_defaults) is dropped"""
        hp = default_hparams(program_defaults)
        given = vars(hparams) if isinstance(hparams, argparse.Namespace) else dict(hparams)
        hp.update({k: v for k, v in given.items() if k in hp})
        self.hparams, self.ps = hp, pixel_set
        self.epoch = self.global_step = 0
        self.history = []
        self.validation, self.best = validation, None
        if hp["validate"] not in VALIDATE_MODES:
            raise L.IrisError(f"validate = {hp['validate']!r}: expected one of {', '.join(VALIDATE_MODES)}")
        if hp["validate"] != "none" and validation is None:
            raise L.IrisError(f"validate = {hp['validate']!r} needs a validation object (utils.validation.ValidationSet)")
        if hp["validate"] in ("images", "all") and int(hp["val_step"]) < 1:
            raise L.IrisError(f"val_step = {hp['val_step']}: a positive number of steps is expected")

    def _start(self, params, networks):
        """the optimizer over the subclass's parameters (networks: FusedAdam's), the two files' names, --resume"""
        hp = self.hparams
        self.optimizer = make_optimizer(hp["optimizer"], params, hp["learning_rate"], hp["weight_decay"], networks=networks)
        name = hp["experiment_name"]
        self.ckpt_file = os.path.join(hp["checkpoint_path"], name, "last.ckpt") if name and hp["checkpoint_path"] else None
        self.log_file = os.path.join(hp["log_path"], name, "metrics.jsonl") if name and hp["log_path"] else None
        self.best_file = os.path.join(os.path.dirname(self.ckpt_file), "best.ckpt") if self.ckpt_file else None
        if hp["resume"] and self.ckpt_file and os.path.exists(self.ckpt_file):
            self.load(self.ckpt_file)
            best_json = os.path.join(os.path.dirname(self.ckpt_file), "best.json")
            if hp["validate"] in ("metric", "all") and os.path.exists(best_json):
                with open(best_json) as fh:
                    self.best = json.load(fh)

    def learning_rate(self, epoch):
        hp = self.hparams
        return multistep_lr(hp["learning_rate"], hp["milestones"], hp["scheduler_rate"], epoch)

    def _extra_state(self):
        """the tensors a subclass adds to the checkpoint under 'emitter.', or None"""
        return None

    def _load_extra(self, ck, path):
        """restores what _extra_state wrote from read_checkpoint's dict; IrisError, before anything is restored, for a file that lacks it"""

    def load(self, path):
        """--resume: everything the checkpoint holds"""
        ck = read_checkpoint(path)
        self._load_extra(ck, path)
        with torch.no_grad():
            self.material.mlp.params.copy_(ck["material"]["mlp.params"])         # (in place: the tensor the optimizer holds; the handle refreshes at the next forward)
        self.model_crf.load_state_dict(ck["model_crf"])
        self.optimizer.load_state_dict(ck["optimizer_states"][0])
        self.epoch, self.global_step = int(ck["epoch"]), int(ck["global_step"])

    def save(self, path=None):
        write_checkpoint(path or self.ckpt_file, self.material.state_dict(), self.model_crf.state_dict(), self.optimizer.state_dict(), epoch=self.epoch,
                         global_step=self.global_step, hyper_parameters=dict(self.hparams), emitter_state=self._extra_state())

    def _log(self, step, epoch, lr, out):
        values = torch.stack([out[k].detach().reshape(()).to(torch.float32) for k in self.logged]).tolist()         # the one synchronisation
        entry = {"step": step, "epoch": epoch, "lr": lr}
        entry.update({self.prefix + "/" + k: v for k, v in zip(self.logged, values)})
        loss = entry[self.prefix + "/loss"]
        if not math.isfinite(loss):
            raise FloatingPointError(f"the loss of step {step} (epoch {epoch}) is {loss}: " + json.dumps(entry))
        self._append(entry)

    def _append(self, entry):
        self.history.append(entry)
        if self.log_file:
            os.makedirs(os.path.dirname(os.path.abspath(self.log_file)), exist_ok=True)
            with open(self.log_file, "a") as fh:
                fh.write(json.dumps(entry) + "\n")

    def validate_epoch(self):
        """the end of an epoch under validate = metric | all: the val/* line, and best.ckpt + best.json when val/loss is strictly below the best so far"""
        out = self.validation.evaluate(getattr(self, "scene", None), self.material)
        loss, psnr = torch.stack([torch.as_tensor(out[k]).detach().reshape(()).to(torch.float64).cpu() for k in ("val/loss", "val/psnr")]).tolist()
        entry = {"step": self.global_step, "epoch": self.epoch, "val/loss": loss, "val/psnr": psnr}
        self._append(entry)
        if self.best_file and not math.isnan(loss) and (self.best is None or loss < self.best["val/loss"]):            # (a NaN is never the best)
            self.best = {"val/loss": loss, "epoch": self.epoch, "step": self.global_step}
            self.save(self.best_file)
            tmp = os.path.join(os.path.dirname(self.best_file), "best.json.tmp")
            with open(tmp, "w") as fh:
                json.dump(self.best, fh)
            os.replace(tmp, os.path.join(os.path.dirname(self.best_file), "best.json"))
        return entry

    def validation_images(self):
        """validation() at the current parameters: view val_frame into outputs/<experiment_name>/<dir_val>/ under the working directory (:345)"""
        hp = self.hparams
        folder = os.path.join("outputs", str(hp["experiment_name"]), str(hp["dir_val"]))
        return self.validation.write_images(folder, self.global_step, int(hp["val_frame"]), self.material, self.model_crf, int(hp["SPP"]), int(hp["spp"]),
                                            emitter=getattr(self, "emitter", None))

    def fit(self, max_epochs):
        every = max(1, int(self.hparams["log_every"]))
        mode = self.hparams["validate"]
        val_step = int(self.hparams["val_step"]) if mode in ("images", "all") else 0
        for epoch in range(self.epoch, int(max_epochs)):
            lr = self.learning_rate(epoch)
            for group in self.optimizer.param_groups:
                group["lr"] = lr
            self.ps.resample()
            for i in range(len(self.ps)):
                if val_step and self.global_step % val_step == 0:
                    self.validation_images()
                out = self.training_step(self.ps[i], self.global_step)
                self.optimizer.zero_grad(set_to_none=True)
                out["loss"].backward()
                self.optimizer.step()
                self.global_step += 1
                if self.global_step % every == 0:
                    self._log(self.global_step - 1, epoch, lr, out)
            self.epoch = epoch + 1
            if self.ckpt_file:
                self.save()
            if mode in ("metric", "all"):
                self.validate_epoch()
        return self
