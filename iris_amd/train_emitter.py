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
call that returns the loss, the psnr and the gradient by L_sum (iris_amd.utils.losses.photometric_loss).  `<checkpoint_path>/<experiment_name>/last.ckpt` is
written at the end of every epoch with `material.*` and `model_crf.*` (in the emitter mode: as loaded, so the file serves slf_refine, refine_shading and
render as the reference's does) and `emitter.radiance`, the optimizer state, the epoch and the step.

Not built: the in-training validation images (the reference's validation(); `python -m iris_amd.render --ckpt last.ckpt` shows the same thing), TensorBoard /
W&B logging (the scalars go to `<log_path>/<experiment_name>/metrics.jsonl` under the reference's names), the `val/loss`-monitored best checkpoint, the
synthetic layout's `albedo` / `roughness` ground-truth scalars, the `Ranger` optimizer, the scannetpp layout, `--res_scale` other than 1; `--val_step`,
`--num_workers`, `--dir_val` and `--val_frame` are accepted and ignored.
"""
import argparse
import json
import math
import os

import torch
import torch.nn.functional as NF

from . import _lib as L
from .train_brdf_crf import DEFAULT_OPTIONS, make_optimizer, multistep_lr
from .utils.stage import read_checkpoint, write_checkpoint

# train_emitter.py:396-403, and what this trainer adds
PROGRAM_DEFAULTS = dict(experiment_name=None, max_epochs=500, log_path="./logs", checkpoint_path="./checkpoints", resume=False, device=0, val_frame=0,
                        log_every=50)
MODES = {"emitter": ("train", ("loss", "loss_c", "psnr")),                       # train_emitter.py:206-208
         "initialize": ("init", ("loss", "loss_c", "loss_a", "psnr"))}           # initialize.py:214-217


def default_hparams(**changes):
    """a plain dict of every option with its default"""
    hp = {name: (list(o["default"]) if isinstance(o["default"], list) else o["default"]) for name, o in DEFAULT_OPTIONS.items()}
    hp.update(PROGRAM_DEFAULTS)
    unknown = set(changes) - set(hp)
    if unknown:
        raise KeyError(f"unknown options {sorted(unknown)}")
    hp.update(changes)
    return hp


class RadianceTrainer:
    """scene: the Scene of the mesh; emitter: an SLFEmitterLearn; material: an NGPBRDF (loaded, or init_parameters() in mode 'initialize'); model_crf: an
    EmorCRF; all on the pixel set's device (the emitter is moved there).  pixel_set: a PixelSet(ray_diff=True) with exposure (and, in mode 'initialize',
    segmentation and int_albedo) that has been through restrict_to_hits(scene).  hparams: a dict or Namespace of options (default_hparams()).
    mode: 'emitter' | 'initialize' (the module docstring).

    training_step(batch) -> dict of 0-d device tensors under the names the mode logs; fit(max_epochs) runs the epochs: resample, then zero_grad / backward
    / step per batch.  Logging, the non-finite check, checkpoints and --resume are BRDFCRFTrainer's: every `log_every` steps that step's scalars are read in
    ONE synchronisation, appended to metrics.jsonl and to `self.history`; a non-finite loss at such a read raises FloatingPointError with the step number."""

    def __init__(self, scene, emitter, material, model_crf, pixel_set, hparams, mode):
        if mode not in MODES:
            raise L.IrisError(f"RadianceTrainer: mode {mode!r}, expected 'emitter' or 'initialize'")
        hp = default_hparams()
        given = vars(hparams) if isinstance(hparams, argparse.Namespace) else dict(hparams)
        hp.update({k: v for k, v in given.items() if k in hp})
        self.hparams, self.mode, self.scene, self.emitter, self.material, self.model_crf, self.ps = hp, mode, scene, emitter, material, model_crf, pixel_set
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
        params = ([p] if mode == "initialize" else []) + [emitter.radiance]
        self.optimizer = make_optimizer(hp["optimizer"], params, hp["learning_rate"], hp["weight_decay"], networks=[material] if mode == "initialize" else [])
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
        if "radiance" not in ck["emitter"]:
            raise L.IrisError(f"{path}: the checkpoint's state_dict has no 'emitter.radiance': it was not written by this stage")
        with torch.no_grad():
            self.material.mlp.params.copy_(ck["material"]["mlp.params"])         # (in place: the tensor the optimizer holds; the handle refreshes at the next forward)
            self.emitter.radiance.copy_(ck["emitter"]["radiance"])
        self.model_crf.load_state_dict(ck["model_crf"])
        self.optimizer.load_state_dict(ck["optimizer_states"][0])
        self.epoch, self.global_step = int(ck["epoch"]), int(ck["global_step"])

    def save(self, path=None):
        hp = {k: v for k, v in self.hparams.items()}
        write_checkpoint(path or self.ckpt_file, self.material.state_dict(), self.model_crf.state_dict(), self.optimizer.state_dict(), epoch=self.epoch,
                         global_step=self.global_step, hyper_parameters=hp, emitter_state={"radiance": self.emitter.radiance})

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

    def _log(self, step, epoch, lr, out):
        values = torch.stack([out[k].detach().reshape(()).to(torch.float32) for k in self.logged]).tolist()         # the one synchronisation
        entry = {"step": step, "epoch": epoch, "lr": lr}
        entry.update({self.prefix + "/" + k: v for k, v in zip(self.logged, values)})
        loss = entry[self.prefix + "/loss"]
        if not math.isfinite(loss):
            raise FloatingPointError(f"the loss of step {step} (epoch {epoch}) is {loss}: " + json.dumps(entry))
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


# ---- the command line (shared with iris_amd.initialize)
def parser(prog="train_emitter", description="the emitter training stage"):
    ap = argparse.ArgumentParser(prog="python -m iris_amd." + prog, description=description)
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
    ap.add_argument("--emor_path", type=str, default=None, help="the EMoR basis file (default: crf/emor.txt under the working directory, as the reference)")
    ap.add_argument("--log_every", type=int, default=PROGRAM_DEFAULTS["log_every"], help="read and write the step's scalars every this many steps")
    ap.set_defaults(resume=False)
    return ap


def run(args, mode, stage_name):
    """main() of both stages: refuse, open the device, load, train"""
    from .model.brdf import NGPBRDF
    from .model.crf import EmorCRF
    from .model.emitter import SLFEmitterLearn
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
    print(f"{stage_name}: --val_step, --num_workers, --dir_val and --val_frame are accepted and ignored (no in-training validation images, no loader "
          "workers: the batches are made on the device)", flush=True)
    device = stage.open_device(args.device, stage_name)
    files = load_training_files(dataset, root, args.ldr_img_dir, has_part=args.has_part, res_scale=args.res_scale, cache_dir=None, device=device)
    scene = load_scene(files["mesh_path"], device=device)
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
    ps = PixelSet(files["views"], files["img_hw"], files["rgb"], segmentation=files["segmentation"], int_albedo=files["int_albedo"], exposure=files["exposure"],
                  synthetic=files["synthetic"], batch_size=args.batch_size, device=device, ray_diff=True)
    n = ps.restrict_to_hits(scene)
    if n == 0:
        raise L.IrisError("no training pixel hits the mesh")
    trainer = RadianceTrainer(scene, emitter, material, model_crf, ps, args, mode)
    print(f"{stage_name}: {len(files['views'])} views of {files['img_hw'][0]} x {files['img_hw'][1]}, {n} pixels on the mesh, {len(ps)} steps per epoch of "
          f"{trainer.n_calls} x {trainer.spp} samples; starting at epoch {trainer.epoch}, step {trainer.global_step}", flush=True)
    trainer.fit(args.max_epochs)
    last = trainer.history[-1] if trainer.history else {}
    print(f"{stage_name}: {trainer.epoch} epochs, {trainer.global_step} steps; last logged loss {last.get(trainer.prefix + '/loss')}; checkpoint {trainer.ckpt_file}",
          flush=True)
    return 0


def main(argv=None):
    return run(parser().parse_args(argv), "emitter", "train_emitter")


def cli(argv=None, stage_name="train_emitter", main_fn=None):
    """main() as a process exit status: what is refused or not built is one line on stderr and status 2, not a traceback"""
    import sys
    try:
        return (main_fn or main)(argv)
    except (L.IrisError, FileNotFoundError) as err:
        print(f"{stage_name}: {err}", file=sys.stderr)
        return 2


if __name__ == "__main__":
    raise SystemExit(cli())
