"""The emitter training and initialisation stages on the GPU (iris_amd/train_emitter.py, iris_amd/initialize.py): RadianceTrainer's step against the literal
composition, what the initialisation step trains, recovery of a known radiance, the two command lines on a real-layout scene, resume.

Fixture: the open box of tests/test_train_brdf_crf.py (the cube [-1, 1]^3 without its +z face) at its image size; the +y face (two triangles) is the ceiling
light; an all-zero radiance cache; NGPBRDF(...).init_parameters(); an EmorCRF from arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as NF

from conftest import REPO, rel_l2
from test_train_brdf_crf import BATCH, BOX_F, BOX_V, H, N, VMAX, VMIN, W, cameras, emor_arrays, stores, write_real_scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CEILING = (4, 5)                                   # the +y face's two triangles in BOX_F
RADIANCE = np.array([[6.0, 5.0, 4.0], [6.0, 5.0, 4.0]], np.float32)


def write_emitter_files(root, radiance=RADIANCE):
    """emitter.pth (the layout extract_emitter_ldr writes) with the ceiling as the emitter, and a vslf.npz whose radiance cache is empty"""
    from iris_amd.model.slf import VoxelSLF
    is_emitter = torch.zeros(len(BOX_F), dtype=torch.bool)
    is_emitter[list(CEILING)] = True
    ev = torch.from_numpy(BOX_V)[torch.from_numpy(BOX_F).long()[is_emitter]]
    area = torch.cross(ev[:, 1] - ev[:, 0], ev[:, 2] - ev[:, 0], dim=-1)
    ep, sp = str(root / "emitter.pth"), str(root / "vslf.npz")
    torch.save({"is_emitter": is_emitter, "emitter_vertices": ev, "emitter_area": area.norm(dim=-1) / 2.0, "emitter_normal": NF.normalize(area, dim=-1),
                "emitter_radiance": torch.from_numpy(np.array(radiance, np.float32))}, ep)
    mask = torch.ones(8, 8, 8, dtype=torch.bool)
    torch.save({"mask": mask, "voxel_min": VMIN, "voxel_max": VMAX, "weight": VoxelSLF(mask, VMIN, VMAX).state_dict()}, sp)
    return ep, sp


def make_trainer(tmp_path, mode, rgb=None, batch_size=BATCH, radiance=RADIANCE, **hp):
    from iris_amd.model.brdf import NGPBRDF
    from iris_amd.model.crf import EmorCRF
    from iris_amd.model.emitter import SLFEmitterLearn
    from iris_amd.train_emitter import RadianceTrainer, default_hparams
    from iris_amd.utils.dataset import PixelSet
    from iris_amd.utils.path_tracing import Scene
    os.makedirs(tmp_path, exist_ok=True)
    torch.manual_seed(0)                                      # the epochs' orders (PixelSet.resample draws from torch's generator on the device)
    st = stores()
    ps = PixelSet(cameras(), (H, W), st["rgb"] if rgb is None else rgb, segmentation=st["segmentation"], int_albedo=st["int_albedo"], exposure=st["exposure"],
                  batch_size=batch_size, device=DEV, ray_diff=True)
    scene = Scene(BOX_V, BOX_F, device=DEV)
    n = ps.restrict_to_hits(scene)
    assert BATCH < n < N, n
    ep, sp = write_emitter_files(tmp_path, radiance)
    emitter = SLFEmitterLearn(ep, sp)
    material = NGPBRDF(VMIN, VMAX).init_parameters(seed=5).to(DEV)
    crf = EmorCRF.from_arrays(*emor_arrays()).to(DEV)
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
    hparams = default_hparams(**{**dict(batch_size=batch_size, experiment_name="exp", checkpoint_path=str(tmp_path / "checkpoints"), log_path=str(tmp_path / "logs"),
                                        log_every=1, SPP=16, spp=4, learning_rate=1e-2), **hp})
    return RadianceTrainer(scene, emitter, material, crf, ps, hparams, mode)


def seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


def test_emitter_step_equals_the_literal_composition(tmp_path):
    from iris_amd.utils.path_tracing import path_tracing_single_step
    tr = make_trainer(tmp_path, "emitter")
    assert [p is tr.emitter.radiance for p in tr.optimizer.param_groups[0]["params"]] == [True]
    assert not tr.material.mlp.params.requires_grad and not tr.model_crf.weight.requires_grad and tr.n_calls == 4
    batch = tr.ps[0]
    before = [t.detach().clone() for t in (tr.material.mlp.params, tr.model_crf.weight, tr.model_crf.f0, tr.model_crf.basis)]
    seed(7)
    out = tr.training_step(batch)
    assert set(out) == {"loss", "loss_c", "psnr"} and out["loss"] is out["loss_c"]
    out["loss"].backward()
    g_step = tr.emitter.radiance.grad.detach().clone()
    tr.emitter.radiance.grad = None
    # the reference's lines (train_emitter.py:181-193) on the same draws
    seed(7)
    xs, ds, dxdu, dydv = tr._rays(batch)
    L = path_tracing_single_step(tr.scene, tr.emitter, tr.material, xs, ds, dxdu, dydv, tr.spp, tr.n_calls) / tr.n_calls
    rgb = tr.model_crf(L, batch["exposure"])
    loss = NF.mse_loss(rgb, batch["rgbs"])
    loss.backward()
    g_comp = tr.emitter.radiance.grad.detach().clone()
    d = (rgb.detach() - batch["rgbs"]).double()
    loss64 = float((d * d).mean())
    err_comp = abs(float(loss.detach().double()) - loss64) / loss64                       # the composed float32 mean's own error, measured
    err = abs(float(out["loss"].detach().double()) - float(loss.detach().double())) / loss64
    print(f"loss: step {float(out['loss']):.9g}, composition {float(loss):.9g}, float64 {loss64:.9g}; composition's own error {err_comp:.3g}, difference {err:.3g}; "
          f"gradient rel L2 {rel_l2(g_step.cpu(), g_comp.cpu()):.3g}; psnr {float(out['psnr']):.4f}")
    assert err <= 2.0 ** -23 + err_comp
    assert abs(float(out["psnr"]) - (-10.0 * np.log10(max(float(out["loss"]), 1e-5)))) <= 1e-5
    assert float(g_comp.abs().max()) > 0 and g_step.shape == RADIANCE.shape
    assert rel_l2(g_step.cpu(), g_comp.cpu()) <= 1e-5                            # the project's tolerance for atomically summed gradients
    tr.optimizer.zero_grad(set_to_none=True)
    out = tr.training_step(batch)
    out["loss"].backward()
    tr.optimizer.step()
    after = (tr.material.mlp.params, tr.model_crf.weight, tr.model_crf.f0, tr.model_crf.basis)
    for a, b in zip(before, after):
        assert torch.equal(a.view(torch.int32), b.detach().view(torch.int32))
    assert tr.material.mlp.params.grad is None and tr.model_crf.weight.grad is None
    assert not torch.equal(tr.emitter.radiance.detach().cpu(), torch.from_numpy(RADIANCE))


def test_initialize_step_trains_the_material_through_the_albedo_term_only(tmp_path):
    from iris_amd.utils.losses import segment_albedo_loss
    from iris_amd.utils.optim import FusedAdam
    tr = make_trainer(tmp_path, "initialize")
    p = tr.material.mlp.params
    assert isinstance(tr.optimizer, FusedAdam) and tr.optimizer.networks == [tr.material]
    assert [q is p or q is tr.emitter.radiance for q in tr.optimizer.param_groups[0]["params"]] == [True, True] and p.requires_grad
    batch = tr.ps[0]
    seed(11)
    out = tr.training_step(batch)
    assert set(out) == {"loss", "loss_c", "loss_a", "psnr"} and p.requires_grad
    out["loss"].backward()
    g_mat = p.grad.detach().clone()
    assert bool(torch.isfinite(g_mat).all()) and float(g_mat.abs().max()) > 0
    assert float(tr.emitter.radiance.grad.abs().max()) > 0 and tr.model_crf.weight.grad is None
    assert abs(float(out["loss"]) - (float(out["loss_a"]) + float(out["loss_c"]))) <= 1e-6 * float(out["loss"])
    # the albedo term alone on the same jittered positions (the step's first draw)
    p.grad = None
    seed(11)
    pos = tr.jittered_positions(batch)
    assert pos.shape == (BATCH, 3) and bool(torch.isfinite(pos).all())
    loss_a = segment_albedo_loss(tr.material(pos)["albedo"], batch["int_albedo"], batch["segmentation"], weight=1.0, scale_invariant=False)
    assert torch.equal(loss_a.detach(), out["loss_a"].detach())
    loss_a.backward()
    err = rel_l2(g_mat.cpu(), p.grad.cpu())
    print(f"material gradient: |g| {float(g_mat.norm()):.6g}, rel L2 to the albedo term's alone {err:.3g}")
    assert err <= 1e-5                          # (the hash tables' gradient is summed with float atomics: not bitwise; the photometric term adds nothing)
    # the jitter stays inside the pixel: the positions are near the hits of the pixel centres, not equal to them
    from iris_amd.utils.path_tracing import ray_intersect
    xs, ds, _, _ = tr._rays(batch)
    centre = ray_intersect(tr.scene, xs, ds)[0]
    assert not torch.equal(pos, centre) and float((pos - centre).norm(dim=-1).median()) < 0.3
    tr.optimizer.step()
    assert tr.material._native.keys[0].fresh(p)


def photographs(tr, radiance, spp=64, n_calls=8):
    """what this project's own integrator and response model make of the scene at `radiance`: (N, 3) float32, zeros where a pixel misses the mesh"""
    from iris_amd.utils.path_tracing import path_tracing_single_step
    ps = tr.ps
    with torch.no_grad():
        keep = tr.emitter.radiance.detach().clone()
        tr.emitter.radiance.copy_(torch.from_numpy(radiance).to(DEV))
        batch = ps.gather(ps.kept)
        xs, ds, dxdu, dydv = tr._rays(batch)
        L = path_tracing_single_step(tr.scene, tr.emitter, tr.material, xs, ds, dxdu, dydv, spp, n_calls) / n_calls
        ps.rgb[ps.kept] = tr.model_crf(L, batch["exposure"])
        tr.emitter.radiance.copy_(keep)


# Chosen on the GPU: SPP 32 / spp 8, batches of 192 pixels, 40 epochs of 2 steps of Adam at learning rate 0.1, from 0.5 x the truth (a mean
# absolute error of 2.5).  End errors of seeds 1, 2, 3 on an MI355X: 0.0639, 0.0817, 0.0868.  (Learning rate 0.05 ends at 0.22, 0.2 at 0.10-0.13; 20 epochs
# at 0.1 at 0.16.)  The condition is only "closer".
RECOVERY = dict(SPP=32, spp=8, learning_rate=0.1, epochs=40, batch_size=192)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_recovery_moves_the_radiance_towards_the_truth(tmp_path, s):
    cfg = dict(RECOVERY)
    epochs, batch_size = cfg.pop("epochs"), cfg.pop("batch_size")
    tr = make_trainer(tmp_path, "emitter", rgb=np.zeros((N, 3), np.float32), batch_size=batch_size, radiance=0.5 * RADIANCE, log_every=1000, checkpoint_path=None,
                      log_path=None, **cfg)
    seed(100 + s)
    photographs(tr, RADIANCE)
    start = float(np.abs(tr.emitter.radiance.detach().cpu().numpy() - RADIANCE).mean())
    seed(s)
    tr.fit(epochs)
    end = float(np.abs(tr.emitter.radiance.detach().cpu().numpy() - RADIANCE).mean())
    print(f"seed {s}: mean absolute error of the emitter rows {start:.4f} -> {end:.4f} after {tr.global_step} steps; radiance {tr.emitter.radiance.detach().cpu().numpy().round(3).tolist()}")
    assert start == pytest.approx(0.5 * RADIANCE.mean(), rel=1e-6)
    assert end < start


# ---- the command lines on a real-layout scene
def cli_scene(tmp_path):
    """write_real_scene's files plus emitter.pth, a vslf.npz with a radiance cache, and the arguments both stages share"""
    pytest.importorskip("PIL")
    scene = write_real_scene(tmp_path)
    ep, sp = write_emitter_files(tmp_path)
    common = ["--dataset", "real", str(scene), "--ldr_img_dir", "ldr", "--voxel_path", sp, "--emitter_path", ep, "--batch_size", str(BATCH), "--max_epochs", "1",
              "--SPP", "8", "--spp", "4", "--crf_basis", "3", "--has_part", "0", "--checkpoint_path", str(tmp_path / "checkpoints"), "--log_path", str(tmp_path / "logs"),
              "--log_every", "1", "--val_frame", "0", "--dir_val", "val_0"]
    return scene, ep, sp, common


def run_module(module, args, cwd):
    p = subprocess.run([sys.executable, "-m", module] + args, env=dict(os.environ, PYTHONPATH=REPO), cwd=str(cwd), capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    return p


def update_emitter_file(tmp_path, scene, ckpt):
    from iris_amd import extract_emitter_ldr
    assert extract_emitter_ldr.cli(["--mode", "update", "--scene", str(scene), "--output", str(tmp_path), "--dataset", "real", "--ldr_img_dir", "ldr", "--ckpt", str(ckpt)]) == 0
    return torch.load(tmp_path / "emitter.pth", map_location="cpu", weights_only=False)["emitter_radiance"]


def test_train_emitter_cli_and_the_update_of_the_emitter_file(tmp_path):
    from iris_amd.model.brdf import NGPBRDF
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils.stage import read_checkpoint, write_checkpoint
    scene, ep, sp, common = cli_scene(tmp_path)
    material = NGPBRDF(VMIN, VMAX).init_parameters(seed=9)
    crf = EmorCRF(dim=3, emor_path=tmp_path / "crf" / "emor.txt")
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.2, -0.1, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.1, 0.2]]))
    write_checkpoint(tmp_path / "in.ckpt", material.state_dict(), crf.state_dict(), {}, epoch=1, global_step=5, hyper_parameters={})
    p = run_module("iris_amd.train_emitter", ["--experiment_name", "cli", "--ckpt_path", str(tmp_path / "in.ckpt")] + common, tmp_path)
    assert p.returncode == 0
    assert "accepted and ignored" in p.stdout
    ck = read_checkpoint(tmp_path / "checkpoints" / "cli" / "last.ckpt")
    rad = ck["emitter"]["radiance"]
    assert rad.shape == RADIANCE.shape and bool(torch.isfinite(rad).all()) and not torch.equal(rad, torch.from_numpy(RADIANCE))
    assert torch.equal(ck["material"]["mlp.params"].view(torch.int32), material.mlp.params.detach().view(torch.int32))
    assert torch.equal(ck["model_crf"]["weight"].view(torch.int32), crf.weight.detach().view(torch.int32))
    assert ck["epoch"] == 1 and ck["global_step"] >= 2 and len(ck["optimizer_states"][0]["state"]) == 1
    lines = [json.loads(l) for l in open(tmp_path / "logs" / "cli" / "metrics.jsonl")]
    assert len(lines) == ck["global_step"]
    for e in lines:
        assert {"train/loss", "train/loss_c", "train/psnr"} <= set(e) and np.isfinite(e["train/loss"])
    # the hole this stage closes: extract_emitter_ldr --mode update reads the checkpoint
    assert torch.equal(update_emitter_file(tmp_path, scene, tmp_path / "checkpoints" / "cli" / "last.ckpt"), rad)


def test_initialize_cli_writes_the_checkpoint_the_next_stages_load(tmp_path):
    from iris_amd.model.brdf import NGPBRDF
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils.stage import read_checkpoint
    scene, ep, sp, common = cli_scene(tmp_path)
    p = run_module("iris_amd.initialize", ["--experiment_name", "init"] + common, tmp_path)
    assert p.returncode == 0
    assert "accepted and ignored" in p.stdout
    path = tmp_path / "checkpoints" / "init" / "last.ckpt"
    ck = read_checkpoint(path)
    assert {"material.mlp.params", "model_crf.weight", "emitter.radiance"} <= set(ck["state_dict"])
    assert not ck["model_crf"]["weight"].any()                                          # the default response model, frozen
    lines = [json.loads(l) for l in open(tmp_path / "logs" / "init" / "metrics.jsonl")]
    assert len(lines) == ck["global_step"] >= 2
    for e in lines:
        assert {"init/loss", "init/loss_c", "init/loss_a", "init/psnr"} <= set(e) and np.isfinite(e["init/loss"])
    # train_brdf_crf --ckpt_path: read_checkpoint + load_state_dict
    material = NGPBRDF(VMIN, VMAX)
    material.load_state_dict(ck["material"])
    assert not torch.equal(material.mlp.params, NGPBRDF(VMIN, VMAX).init_parameters().mlp.params) and bool(torch.isfinite(material.mlp.params).all())
    crf = EmorCRF(dim=3, emor_path=tmp_path / "crf" / "emor.txt")
    crf.load_state_dict(ck["model_crf"])
    # extract_emitter_ldr --mode update
    rad = ck["emitter"]["radiance"]
    assert rad.shape == RADIANCE.shape and bool(torch.isfinite(rad).all()) and not torch.equal(rad, torch.from_numpy(RADIANCE))
    assert torch.equal(update_emitter_file(tmp_path, scene, path), rad)


def test_resume_counts_as_a_straight_run(tmp_path):
    first = make_trainer(tmp_path / "a", "emitter")
    first.fit(1)
    steps = first.global_step
    assert steps == len(first.ps) >= 2
    second = make_trainer(tmp_path / "a", "emitter", resume=True)
    assert second.epoch == 1 and second.global_step == steps
    assert torch.equal(second.emitter.radiance.detach().view(torch.int32), first.emitter.radiance.detach().view(torch.int32))
    st1, st2 = first.optimizer.state[first.emitter.radiance], second.optimizer.state[second.emitter.radiance]
    assert torch.equal(st1["exp_avg"], st2["exp_avg"]) and torch.equal(st1["exp_avg_sq"], st2["exp_avg_sq"]) and float(st2["step"]) == steps
    second.fit(2)
    straight = make_trainer(tmp_path / "b", "emitter")
    straight.fit(2)
    for tr in (second, straight):
        assert tr.epoch == 2 and tr.global_step == 2 * steps and float(tr.optimizer.state[tr.emitter.radiance]["step"]) == 2 * steps
    assert second.history[0]["step"] == steps and second.history[0]["epoch"] == 1
    a = torch.load(tmp_path / "a" / "checkpoints" / "exp" / "last.ckpt", map_location="cpu", weights_only=False)
    b = torch.load(tmp_path / "b" / "checkpoints" / "exp" / "last.ckpt", map_location="cpu", weights_only=False)
    assert (a["epoch"], a["global_step"]) == (b["epoch"], b["global_step"]) == (2, 2 * steps)
    fresh = make_trainer(tmp_path / "elsewhere", "emitter", resume=True)                # nothing to resume from: starts at zero
    assert fresh.epoch == 0 and fresh.global_step == 0
