"""The BRDF-CRF training stage (reference: train_brdf_crf.py): the stage that writes the checkpoint `render`, `render_relight`, `refine_shading` and
`utils.export` load with --ckpt.

    python -m iris_amd.train_brdf_crf --experiment_name EXP --dataset real DIR --ldr_img_dir ldr --voxel_path OUT/vslf.npz --cache_dir OUT/shading \
        --max_epochs 2 --checkpoint_path checkpoints --log_path logs

takes the reference's arguments (configs/config.py and train_brdf_crf.py:511-531).  A step is `brdf_crf_loss(material(batch['positions']), ...)` on a
`PixelSet` batch (every view traced once at construction: `restrict_to_hits`), `backward`, and `FusedAdam` -- the Adam update of the 27 963 328 material
parameters and the refresh of the half copy the forward reads, in one pass (iris_amd/utils/optim.py).  The learning rate follows `MultiStepLR` stepped
once per epoch (Lightning's default interval).  `<checkpoint_path>/<experiment_name>/last.ckpt` is written at the end of every epoch in the layout the
reference's loaders read: `['state_dict']` with `material.*` and `model_crf.*` keys.

Not built: the in-training validation images (train_brdf_crf.py:339-453; `python -m iris_amd.render --ckpt last.ckpt` shows the same thing), TensorBoard /
W&B logging (the scalars go to `<log_path>/<experiment_name>/metrics.jsonl` under the reference's names), the `val/loss`-monitored best checkpoint, the
`Ranger` optimizer, the scannetpp layout; `--val_step` and `--num_workers` are accepted and ignored.
"""
import argparse
import json
import math
import os

import torch

from . import _lib as L
from .utils.stage import read_checkpoint, write_checkpoint          # (the checkpoint's layout lives with its other readers)

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
# train_brdf_crf.py:517-526, and what this trainer adds
PROGRAM_DEFAULTS = dict(experiment_name=None, max_epochs=500, log_path="./logs", checkpoint_path="./checkpoints", resume=False, device=0, val_frame=0,
                        cache_dir=None, log_every=50)
LOGGED = ("loss", "loss_c", "loss_d", "loss_seg", "loss_a", "psnr")          # train_brdf_crf.py:324-329, as 'train/<name>'


def default_hparams(**changes):
    """a plain dict of every option with its default"""
    hp = {name: (list(o["default"]) if isinstance(o["default"], list) else o["default"]) for name, o in DEFAULT_OPTIONS.items()}
    hp.update(PROGRAM_DEFAULTS)
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
        from .utils.optim import FusedAdam
        return FusedAdam(params, lr=lr, weight_decay=weight_decay, networks=networks)
    if name == "SGD":
        return torch.optim.SGD(params, lr=lr, weight_decay=weight_decay)
    if name == "Ranger":
        raise L.IrisError("--optimizer Ranger is not built (the reference lists it but constructs only SGD and Adam): use Adam or SGD")
    raise L.IrisError(f"--optimizer {name}: expected Adam or SGD")


class BRDFCRFTrainer:
    """material: an NGPBRDF on the GPU (init_parameters() or loaded); model_crf: an EmorCRF on the same device; pixel_set: a PixelSet with its cache attached
    that has been through restrict_to_hits(scene, store_positions=True); hparams: a dict or Namespace of options (default_hparams()).

    training_step(batch, global_step) -> brdf_crf_loss's dict; fit(max_epochs) runs the epochs: resample, then zero_grad / backward / step per batch.
    The logged scalars stay on the device; every `log_every` steps that step's are read in ONE synchronisation, appended to metrics.jsonl and to
    `self.history`; a non-finite loss at such a read raises FloatingPointError with the step number.  With hparams['resume'] and a last.ckpt in place the
    constructor restores parameters, optimizer state, epoch and global step from it."""

    def __init__(self, material, model_crf, pixel_set, hparams):
        hp = default_hparams()
        given = vars(hparams) if isinstance(hparams, argparse.Namespace) else dict(hparams)
        hp.update({k: v for k, v in given.items() if k in hp})
        self.hparams, self.material, self.model_crf, self.ps = hp, material, model_crf, pixel_set
        if pixel_set.cache is None or pixel_set.positions is None:
            raise L.IrisError("BRDFCRFTrainer: the pixel set needs attach_cache(cache) and restrict_to_hits(scene, store_positions=True)")
        if pixel_set.segmentation is None or pixel_set.exposure is None or (hp["la"] > 0 and pixel_set.int_albedo is None):
            raise L.IrisError("BRDFCRFTrainer: the pixel set needs segmentation and exposure (and int_albedo when la > 0)")
        p = material.mlp.params
        if not p.is_cuda or p.device != pixel_set.device or model_crf.weight.device != p.device:
            raise L.IrisError(f"BRDFCRFTrainer: material ({p.device}), model_crf ({model_crf.weight.device}) and the pixel set ({pixel_set.device}) must share a HIP device")
        p.requires_grad_(True)
        model_crf.weight.requires_grad_(not hp["freeze_crf"])
        params = [p] + ([] if hp["freeze_crf"] else [model_crf.weight])
        self.optimizer = make_optimizer(hp["optimizer"], params, hp["learning_rate"], hp["weight_decay"], networks=[material])
        self.epoch = self.global_step = 0
        self.history = []
        name = hp["experiment_name"]
        self.ckpt_file = os.path.join(hp["checkpoint_path"], name, "last.ckpt") if name and hp["checkpoint_path"] else None
        self.log_file = os.path.join(hp["log_path"], name, "metrics.jsonl") if name and hp["log_path"] else None
        if hp["resume"] and self.ckpt_file and os.path.exists(self.ckpt_file):
            self.load(self.ckpt_file)

    def learning_rate(self, epoch):
        hp = self.hparams
        return multistep_lr(hp["learning_rate"], hp["milestones"], hp["scheduler_rate"], epoch)

    def load(self, path):
        """--resume: everything the checkpoint holds"""
        ck = read_checkpoint(path)
        with torch.no_grad():
            self.material.mlp.params.copy_(ck["material"]["mlp.params"])         # (in place: the tensor the optimizer holds; the handle refreshes at the next forward)
        self.model_crf.load_state_dict(ck["model_crf"])
        self.optimizer.load_state_dict(ck["optimizer_states"][0])
        self.epoch, self.global_step = int(ck["epoch"]), int(ck["global_step"])

    def save(self, path=None):
        hp = {k: v for k, v in self.hparams.items()}
        write_checkpoint(path or self.ckpt_file, self.material.state_dict(), self.model_crf.state_dict(), self.optimizer.state_dict(), epoch=self.epoch,
                         global_step=self.global_step, hyper_parameters=hp)

    def training_step(self, batch, global_step):
        """train_brdf_crf.py:163-337 on an all-valid batch -> {'loss', 'loss_c', 'loss_d', 'loss_seg', 'loss_a', 'reg_crf', 'psnr'}, device tensors"""
        from .utils.losses import brdf_crf_loss
        hp, m = self.hparams, self.material
        return brdf_crf_loss(m(batch["positions"]), cache=self.ps.cache, idx=batch["idx"], crf=self.model_crf, exposure=batch["exposure"], rgbs_gt=batch["rgbs"],
                             segmentation=batch["segmentation"], positions=batch["positions"], albedo_prior=batch["int_albedo"], has_part=hp["has_part"],
                             ld=hp["ld"], lp=hp["lp"], ls=hp["ls"], la=hp["la"], sigma_albedo=hp["sigma_albedo"], sigma_pos=hp["sigma_pos"],
                             l_crf_increasing=hp["l_crf_increasing"], l_crf_weight=hp["l_crf_weight"], seed=global_step, voxel_min=m.voxel_min,
                             voxel_max=m.voxel_max)

    def _log(self, step, epoch, lr, out):
        values = torch.stack([out[k].detach().reshape(()).to(torch.float32) for k in LOGGED]).tolist()         # the one synchronisation
        entry = {"step": step, "epoch": epoch, "lr": lr}
        entry.update({"train/" + k: v for k, v in zip(LOGGED, values)})
        if not math.isfinite(entry["train/loss"]):
            raise FloatingPointError(f"the loss of step {step} (epoch {epoch}) is {entry['train/loss']}: " + json.dumps(entry))
        self.history.append(entry)
        if self.log_file:
            os.makedirs(os.path.dirname(os.path.abspath(self.log_file)), exist_ok=True)
            with open(self.log_file, "a") as fh:
                fh.write(json.dumps(entry) + "\n")

    def fit(self, max_epochs):
        every = max(1, int(self.hparams["log_every"]))
        for epoch in range(self.epoch, int(max_epochs)):
            lr = self.learning_rate(epoch)
            for group in self.optimizer.param_groups:
                group["lr"] = lr
            self.ps.resample()
            for i in range(len(self.ps)):
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
        return self


# ---- the command line
def parser():
    ap = argparse.ArgumentParser(prog="python -m iris_amd.train_brdf_crf", description="the BRDF-CRF training stage")
    for name, o in DEFAULT_OPTIONS.items():
        ap.add_argument("--" + name, **o)
    ap.add_argument("--experiment_name", type=str, required=True)
    ap.add_argument("--max_epochs", type=int, default=PROGRAM_DEFAULTS["max_epochs"])
    ap.add_argument("--log_path", type=str, default=PROGRAM_DEFAULTS["log_path"])
    ap.add_argument("--ft", type=str, default=None)
    ap.add_argument("--checkpoint_path", type=str, default=PROGRAM_DEFAULTS["checkpoint_path"])
    ap.add_argument("--resume", dest="resume", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--val_frame", type=int, default=0)
    ap.add_argument("--cache_dir", type=str)
    ap.add_argument("--log_every", type=int, default=PROGRAM_DEFAULTS["log_every"], help="read and write the step's scalars every this many steps")
    ap.set_defaults(resume=False)
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    from .model.brdf import NGPBRDF
    from .model.crf import EmorCRF
    from .utils import stage
    from .utils.dataset import PixelSet
    from .utils.dataset.files import load_training_files
    from .utils.path_tracing import load_scene
    dataset, root = args.dataset
    # everything that can be refused is refused before the device is touched
    if dataset == "scannetpp" or float(args.res_scale) != 1.0 or not args.ldr_img_dir:
        load_training_files(dataset, root, args.ldr_img_dir, res_scale=args.res_scale)
    if args.optimizer == "Ranger":
        make_optimizer(args.optimizer, [], args.learning_rate, args.weight_decay, networks=())
    if args.cache_dir is None:
        raise L.IrisError("--cache_dir is needed: the stage trains on the baked shadings (python -m iris_amd.bake_shading --output DIR)")
    print("train_brdf_crf: --val_step and --num_workers are accepted and ignored (no in-training validation images, no loader workers: the batches are "
          "made on the device)", flush=True)
    device = stage.open_device(args.device, "train_brdf_crf")
    files = load_training_files(dataset, root, args.ldr_img_dir, has_part=args.has_part, res_scale=args.res_scale, cache_dir=args.cache_dir, device=device)
    scene = load_scene(files["mesh_path"], device=device)
    material = NGPBRDF(*stage.voxel_range(args.voxel_path)).init_parameters()
    model_crf = EmorCRF(dim=args.crf_basis)
    if args.ckpt_path:
        ck = read_checkpoint(args.ckpt_path)
        material.load_state_dict(ck["material"])
        if args.load_crf:
            model_crf.load_state_dict(ck["model_crf"])
    material.to(device)
    model_crf.to(device)
    ps = PixelSet(files["views"], files["img_hw"], files["rgb"], segmentation=files["segmentation"], int_albedo=files["int_albedo"], exposure=files["exposure"],
                  synthetic=files["synthetic"], batch_size=args.batch_size, device=device)
    ps.attach_cache(files["cache"])
    n = ps.restrict_to_hits(scene, store_positions=True)
    if n == 0:
        raise L.IrisError("no training pixel hits the mesh")
    trainer = BRDFCRFTrainer(material, model_crf, ps, args)
    print(f"train_brdf_crf: {len(files['views'])} views of {files['img_hw'][0]} x {files['img_hw'][1]}, {n} pixels on the mesh, {len(ps)} steps per epoch; "
          f"starting at epoch {trainer.epoch}, step {trainer.global_step}", flush=True)
    trainer.fit(args.max_epochs)
    last = trainer.history[-1] if trainer.history else {}
    print(f"train_brdf_crf: {trainer.epoch} epochs, {trainer.global_step} steps; last logged loss {last.get('train/loss')}; checkpoint {trainer.ckpt_file}", flush=True)
    return 0


def cli(argv=None):
    """main() as a process exit status: what is refused or not built is one line on stderr and status 2, not a traceback"""
    import sys
    try:
        return main(argv)
    except (L.IrisError, FileNotFoundError) as err:
        print(f"train_brdf_crf: {err}", file=sys.stderr)
        return 2


if __name__ == "__main__":
    raise SystemExit(cli())
