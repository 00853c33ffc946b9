"""The trainers' validation without a GPU (iris_amd/utils/validation.py, iris_amd/utils/trainer.py): the numpy restatement of iris_val_kd_loss
(tests/validation_ref.py) against the reference's literal lines in float32 torch, the gamma table, the command lines' --validate, what is refused before a
device is opened, and the val/loss monitor of the shared loop on the host-only toy trainer of tests/test_trainer_loop_cpu.py."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as NF

import validation_ref as R
from iris_amd._lib import IrisError
from iris_amd.utils import trainer, validation
from test_trainer_loop_cpu import P0, W0, Batches, PlainToy, hparams

GAMMA = 2.2


def inputs(H, W, synthetic, seed):
    """one view: the network's outputs at every pixel, about 20 % misses, and either ground truth"""
    g = np.random.default_rng(1000 * seed + 7 * H + W + synthetic)
    n = H * W
    d = dict(albedo=g.random((n, 3), np.float32), metallic=g.random((n, 1), np.float32), valid=g.random(n) >= 0.2)
    if synthetic:
        emit = np.where(g.random((n, 1)) < 0.25, g.random((n, 3), np.float32) * np.float32(4.0), np.float32(0.0)).astype(np.float32)
        d.update(gt=g.random((n, 3), np.float32), emit=emit)
    else:
        d.update(codes=g.integers(0, 256, (n, 3)).astype(np.uint8))
    return d


def reference_loss(d, synthetic):
    """train_brdf_crf.py:459-494 on one view, in float32 torch: the network's outputs stand for self.material(position[b0:b1])"""
    valid = torch.from_numpy(d["valid"])
    albedo_net, metallic_net = torch.from_numpy(d["albedo"]), torch.from_numpy(d["metallic"])
    if synthetic:
        emission_mask_gt = torch.from_numpy(d["emit"]).mean(-1, keepdim=True) == 0
    else:
        emission_mask_gt = torch.ones(len(valid), 1)
    albedo_ = albedo_net[valid] * (1 - metallic_net[valid])
    albedo = torch.zeros(len(valid), 3)
    albedo[valid] = albedo_
    if synthetic:
        albedo_gt = torch.from_numpy(d["gt"])
    else:
        rgb_gt = torch.from_numpy(d["codes"]).to(torch.float32) / 255
        albedo_gt = rgb_gt.pow(1 / GAMMA).clamp(0, 1)
    albedo = albedo * emission_mask_gt
    albedo_gt = albedo_gt * emission_mask_gt
    return float(NF.mse_loss(albedo_gt, albedo).double())


@pytest.mark.parametrize("synthetic", [True, False], ids=["synthetic", "ldr"])
@pytest.mark.parametrize("hw", [(1, 1), (7, 73), (12, 16), (9, 57)])
def test_the_restatement_is_the_reference_lines_up_to_the_float32_mean(hw, synthetic):
    """|restatement - reference| <= loss 3HW 2^-24 (a float32 sum of 3HW terms against a float64 one) + 2 sqrt(loss) delta + delta^2 (every term's ground
    truth off by delta: 2^-23 through the gamma table, twice the table's measured distance to torch's pow; 0 for a synthetic scene)"""
    H, W = hw
    delta = 0.0 if synthetic else 2.0 ** -23
    worst = 0.0
    for seed in range(8):
        d = inputs(H, W, synthetic, seed)
        truth = dict(gt=d["gt"], emit=d["emit"]) if synthetic else dict(codes=d["codes"], lut=validation.gamma_table())
        loss = float(R.loss_and_psnr(R.kd_loss_sums(d["albedo"], d["metallic"], d["valid"], hw, **truth), hw)[0][0])
        ref = reference_loss(d, synthetic)
        bound = loss * 3 * H * W * 2.0 ** -24 + 2 * math.sqrt(loss) * delta + delta * delta
        print(f"{H} x {W} {'synthetic' if synthetic else 'ldr'} seed {seed}: restatement {loss:.9g}, reference {ref:.9g}, |difference| {abs(loss - ref):.3g}, bound {bound:.3g}")
        assert abs(loss - ref) <= bound
        worst = max(worst, abs(loss - ref) / bound if bound else 0.0)
    print(f"worst case: {worst:.3f} of the bound")


def test_the_restatement_masks_and_selects():
    """an invalid pixel's network output is never used (a NaN there costs nothing); an emissive pixel of a synthetic scene counts nothing"""
    d = inputs(5, 6, True, 0)
    S = R.kd_loss_sums(d["albedo"], d["metallic"], d["valid"], (5, 6), gt=d["gt"], emit=d["emit"])
    d["albedo"][~d["valid"]] = np.nan
    assert R.kd_loss_sums(d["albedo"], d["metallic"], d["valid"], (5, 6), gt=d["gt"], emit=d["emit"])[0] == S[0]
    assert R.kd_loss_sums(d["albedo"], d["metallic"], d["valid"], (5, 6), gt=d["gt"], emit=np.ones_like(d["emit"]))[0] == 0.0
    assert R.kd_loss_sums(d["albedo"], d["metallic"], np.zeros(30, bool), (5, 6), codes=np.zeros((30, 3), np.uint8), lut=validation.gamma_table())[0] == 0.0


def test_gamma_table():
    lut = validation.gamma_table()
    assert lut.shape == (256,) and lut.dtype == np.float32 and lut[0] == 0.0 and lut[255] == 1.0 and (np.diff(lut) > 0).all()
    x = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float64)
    assert np.array_equal(lut, np.clip(x ** (1.0 / 2.2), 0.0, 1.0).astype(np.float32))
    ref = (torch.arange(256, dtype=torch.float32) / 255).pow(1 / GAMMA).clamp(0, 1).numpy()
    far = float(np.abs(lut.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"gamma table against torch's float32 pow: {far * 2 ** 24:.3f} x 2^-24 at most")
    assert far <= 2.0 ** -23
    lut[3] = 9.0                                                   # a copy: the module's table is not the caller's to change
    assert validation.gamma_table()[3] != 9.0


def _options(parser):
    return {a.dest: (tuple(a.option_strings), a.type, a.default, a.choices, a.required, a.nargs) for a in parser._actions}


def test_cli_parser_adds_validate_and_parser_is_as_before():
    from iris_amd import initialize, train_brdf_crf, train_emitter
    for mod in (train_brdf_crf, train_emitter, initialize):
        plain, cli = _options(mod.parser()), _options(mod.cli_parser())
        assert "validate" not in plain and set(cli) - set(plain) == {"validate"}
        assert {k: v for k, v in cli.items() if k != "validate"} == plain
        assert cli["validate"][2] == "none" and tuple(cli["validate"][3]) == ("none", "metric", "images", "all")
        assert mod.cli_parser().prog == mod.parser().prog
        with pytest.raises(SystemExit):
            mod.cli_parser().parse_args(["--experiment_name", "x", "--validate", "sometimes"])
    assert trainer.PROGRAM_DEFAULTS["validate"] == "none"


def test_the_ctypes_structure_mirrors_the_header(tmp_path):
    """ValKdLossArgs has the size and the field offsets of iris_val_kd_loss_args as g++ lays out include/iris_hip.h"""
    import ctypes as C
    import subprocess
    from conftest import REPO
    from iris_amd import _lib as L
    fields = [name for name, _ in L.ValKdLossArgs._fields_]
    lines = ['    std::printf("%zu\\n", sizeof(iris_val_kd_loss_args));'] + [f'    std::printf("%zu\\n", offsetof(iris_val_kd_loss_args, {f}));' for f in fields]
    src, exe = tmp_path / "layout.cpp", str(tmp_path / "layout")
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "iris_hip.h"\nint main() {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", exe], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [C.sizeof(L.ValKdLossArgs)] + [getattr(L.ValKdLossArgs, f).offset for f in fields] and len(fields) == 13


def test_kd_validation_loss_refuses_what_it_cannot_score():
    a, m, v = torch.zeros(6, 3), torch.zeros(6), torch.ones(6, dtype=torch.bool)
    with pytest.raises(IrisError, match="either gt and emit"):
        validation.kd_validation_loss(a, m, v, img_hw=(2, 3))
    with pytest.raises(IrisError, match="either gt and emit"):
        validation.kd_validation_loss(a, m, v, gt=a, emit=a, codes=a.to(torch.uint8), img_hw=(2, 3))
    with pytest.raises(IrisError, match="both gt and emit"):
        validation.kd_validation_loss(a, m, v, gt=a, img_hw=(2, 3))
    with pytest.raises(IrisError, match="multiple of H W"):
        validation.kd_validation_loss(a, m, v, codes=a.to(torch.uint8), img_hw=(2, 4))
    with pytest.raises(IrisError, match="HIP device"):                     # CPU tensors: there is no CPU path
        validation.kd_validation_loss(a, m, v, codes=a.to(torch.uint8), img_hw=(2, 3))


# ---- what the command lines refuse before a device is opened
def real_scene(tmp_path):
    from test_train_brdf_crf import write_real_scene
    pytest.importorskip("PIL")
    return write_real_scene(tmp_path)


def brdf_args(tmp_path, scene, *more):
    return ["--experiment_name", "x", "--dataset", "real", str(scene), "--ldr_img_dir", "ldr", "--voxel_path", str(tmp_path / "vslf.npz"), "--cache_dir",
            str(tmp_path / "shading"), "--checkpoint_path", str(tmp_path / "c"), "--log_path", str(tmp_path / "l")] + list(more)


def test_the_refusals_come_before_any_device_call(tmp_path, capsys, monkeypatch):
    from iris_amd import initialize, train_brdf_crf, train_emitter
    from iris_amd.utils import stage
    from iris_amd.utils.texture import write_png
    from test_train_brdf_crf import H, W

    def no_device(*a, **k):
        raise AssertionError("the device was opened")
    monkeypatch.setattr(stage, "open_device", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    scene = real_scene(tmp_path)
    photo = scene / "ldr" / "000_0001.png"                          # view 0 is the validation split; write_real_scene writes the training views' files only
    for mode in ("metric", "images", "all"):
        assert train_brdf_crf.cli(brdf_args(tmp_path, scene, "--validate", mode)) == 2
        assert str(photo) in capsys.readouterr().err
    write_png(photo, np.zeros((H + 1, W, 3), np.uint8))
    assert train_brdf_crf.cli(brdf_args(tmp_path, scene, "--validate", "metric")) == 2
    assert f"{H + 1} x {W}, the training views {H} x {W}" in capsys.readouterr().err
    write_png(photo, np.zeros((H, W, 3), np.uint8))
    assert train_brdf_crf.cli(brdf_args(tmp_path, scene, "--validate", "images")) == 2
    assert "--emitter_path" in capsys.readouterr().err
    assert train_brdf_crf.cli(brdf_args(tmp_path, scene, "--validate", "all", "--emitter_path", str(tmp_path / "nowhere.pth"))) == 2
    assert "nowhere.pth" in capsys.readouterr().err
    assert train_brdf_crf.cli(brdf_args(tmp_path, scene, "--validate", "all", "--emitter_path", str(photo), "--val_frame", "1")) == 2
    assert "--val_frame 1" in capsys.readouterr().err
    assert train_brdf_crf.cli(brdf_args(tmp_path, scene, "--validate", "images", "--emitter_path", str(photo), "--val_step", "0")) == 2
    assert "--val_step 0" in capsys.readouterr().err
    os.remove(scene / "ldr" / "cam" / "exposure.npy")
    for mod in (train_emitter, initialize):
        args = [a for a in brdf_args(tmp_path, scene, "--validate", "metric") if a not in ("--cache_dir", str(tmp_path / "shading"))]      # (not an option of theirs)
        assert mod.cli(args + ["--emitter_path", str(photo)]) == 2
        assert "exposure.npy" in capsys.readouterr().err
    assert not (tmp_path / "c").exists() and not (tmp_path / "l").exists() and not os.path.exists("outputs")
    np.save(scene / "ldr" / "cam" / "exposure.npy", np.array([9.0, 0.6, 0.9, 1.2], np.float32))
    files = validation.validation_files("real", str(scene), None, "ldr", 1.0)
    assert files["img_hw"] == (H, W) and len(files["views"]) == 1 and files["photographs"] == [str(photo)] and files["exposure"].tolist() == [9.0]
    assert not files["synthetic"] and files["diffcol"] is None


# ---- the monitor of the shared loop
class Scripted:
    """a validation object whose val/loss follows a script"""

    def __init__(self, losses):
        self.losses, self.calls, self.images = list(losses), 0, []

    def evaluate(self, scene, material):
        loss = self.losses[self.calls]
        self.calls += 1
        return {"val/loss": torch.tensor(loss, dtype=torch.float64), "val/psnr": -10.0 * math.log10(max(loss, 1e-5))}

    def write_images(self, folder, step, frame, material, model_crf, SPP, spp, emitter=None):
        self.images.append((folder, step, frame, SPP, spp, [float(x) for x in material.mlp.params.detach()]))


def folder_of(tr):
    return os.path.dirname(tr.ckpt_file)


class Validated(PlainToy):
    """PlainToy (its model, batches and step) with a validation object handed to the loop"""

    def __init__(self, hparams, validation):
        trainer.Trainer.__init__(self, Batches(), hparams, trainer.PROGRAM_DEFAULTS, validation=validation)
        self.material, self.model_crf = torch.nn.Module(), torch.nn.Module()
        self.material.mlp = torch.nn.Module()
        self.material.mlp.params = torch.nn.Parameter(torch.tensor(P0))
        self.model_crf.weight = torch.nn.Parameter(torch.tensor(W0))
        self.seen, self.nan_at = torch.zeros(1), None
        self._start([self.material.mlp.params, self.model_crf.weight], networks=[])


def toy(hp, validation):
    return Validated(hp, validation)


def test_best_checkpoint_is_the_epoch_of_the_strict_minimum(tmp_path):
    from iris_amd.utils.stage import read_checkpoint
    script = Scripted([0.5, 0.3, 0.3, 0.4])
    tr = toy(hparams(tmp_path, validate="metric"), script).fit(4)
    assert script.calls == 4 and script.images == []
    val = [e for e in tr.history if "val/loss" in e]
    assert [(e["step"], e["epoch"], e["val/loss"]) for e in val] == [(3, 1, 0.5), (6, 2, 0.3), (9, 3, 0.3), (12, 4, 0.4)]
    assert all(set(e) == {"step", "epoch", "val/loss", "val/psnr"} and e["val/psnr"] == pytest.approx(-10 * math.log10(e["val/loss"])) for e in val)
    with open(tr.log_file) as fh:
        assert [json.loads(line) for line in fh] == tr.history
    assert sorted(os.listdir(folder_of(tr))) == ["best.ckpt", "best.json", "last.ckpt"]
    best, last = read_checkpoint(tr.best_file), read_checkpoint(tr.ckpt_file)
    assert (best["epoch"], best["global_step"]) == (2, 6) and (last["epoch"], last["global_step"]) == (4, 12)       # the FIRST 0.3: the second is not strictly below
    assert list(torch.load(tr.best_file, weights_only=False)) == ["state_dict", "optimizer_states", "epoch", "global_step", "hyper_parameters"]
    with open(os.path.join(folder_of(tr), "best.json")) as fh:
        assert json.load(fh) == {"val/loss": 0.3, "epoch": 2, "step": 6} == tr.best
    # best.ckpt holds epoch 2's parameters: a straight run of two epochs ends on them
    two = toy(hparams(tmp_path / "two", validate="metric"), Scripted([0.5, 0.3])).fit(2)
    assert torch.equal(best["material"]["mlp.params"], two.material.mlp.params.detach())
    assert not torch.equal(best["material"]["mlp.params"], last["material"]["mlp.params"])


def test_a_non_finite_val_loss_is_never_the_best(tmp_path):
    tr = toy(hparams(tmp_path, validate="all", val_step=1000), Scripted([float("nan"), 0.7, float("nan")])).fit(3)
    assert tr.best == {"val/loss": 0.7, "epoch": 2, "step": 6}


def test_resume_keeps_a_better_earlier_best(tmp_path):
    from iris_amd.utils.stage import read_checkpoint
    hp = hparams(tmp_path, validate="metric")
    first = toy(hp, Scripted([0.2, 0.5])).fit(2)
    assert first.best["epoch"] == 1
    tr = toy(dict(hp, resume=True), Scripted([0.3, 0.25]))
    assert tr.epoch == 2 and tr.best == {"val/loss": 0.2, "epoch": 1, "step": 3}
    tr.fit(4)
    assert tr.best["epoch"] == 1 and read_checkpoint(tr.best_file)["epoch"] == 1
    with open(os.path.join(folder_of(tr), "best.json")) as fh:
        assert json.load(fh)["val/loss"] == 0.2
    again = toy(dict(hp, resume=True), Scripted([0.1]))               # and a better later one replaces it
    again.fit(5)
    assert again.best == {"val/loss": 0.1, "epoch": 5, "step": 15} and read_checkpoint(again.best_file)["epoch"] == 5


def test_validate_none_changes_nothing(tmp_path):
    plain = PlainToy(hparams(tmp_path / "a")).fit(2)
    script = Scripted([0.1, 0.2])
    tr = toy(hparams(tmp_path / "b"), script).fit(2)                   # validate = 'none': the object is not touched
    assert script.calls == 0 and script.images == [] and tr.best is None
    assert tr.history == plain.history and os.listdir(folder_of(tr)) == ["last.ckpt"]
    with open(tr.log_file) as a, open(plain.log_file) as b:
        assert a.read() == b.read()
    with pytest.raises(IrisError, match="needs a validation object"):
        PlainToy(hparams(tmp_path / "c", validate="metric"))
    with pytest.raises(IrisError, match="expected one of"):
        PlainToy(hparams(tmp_path / "c", validate="yes"))


def test_images_come_before_every_val_step_th_step(tmp_path):
    script = Scripted([0.4, 0.3])
    tr = toy(hparams(tmp_path, validate="images", val_step=2, val_frame=3, dir_val="val_7", SPP=16, spp=4), script).fit(2)
    assert script.calls == 0 and not os.path.exists(os.path.join(folder_of(tr), "best.ckpt"))
    assert [(i[0], i[1], i[2], i[3], i[4]) for i in script.images] == [(os.path.join("outputs", "exp", "val_7"), s, 3, 16, 4) for s in (0, 2, 4)]
    assert script.images[0][5] == pytest.approx(P0) and script.images[1][5] != script.images[0][5]          # step 0: the initial parameters
    both = Scripted([0.4, 0.3])
    toy(hparams(tmp_path / "all", validate="all", val_step=4), both).fit(2)
    assert both.calls == 2 and [i[1] for i in both.images] == [0, 4]


def test_validation_files_of_a_synthetic_scene(tmp_path):
    """<root>/val: transforms.json, <ldr>/{i:03d}_0001.png, <ldr>/cam/exposure.npy, DiffCol and Emit maps; a missing or wrong-size map is refused"""
    pytest.importorskip("PIL")
    from iris_amd.utils.exr import write_exr
    from iris_amd.utils.texture import write_png
    val = tmp_path / "val"
    for d in (val / "ldr" / "cam", val / "DiffCol", val / "Emit"):
        os.makedirs(d)
    frames = [{"transform_matrix": np.eye(4).tolist()} for _ in range(2)]
    (val / "transforms.json").write_text(json.dumps({"camera_angle_x": 0.9, "frames": frames}))
    np.save(val / "ldr" / "cam" / "exposure.npy", np.array([0.5, 2.0], np.float32))
    for i in range(2):
        write_png(val / "ldr" / ("%03d_0001.png" % i), np.zeros((6, 8, 3), np.uint8))
        write_exr(val / "DiffCol" / ("%03d_0001.exr" % i), np.zeros((6, 8, 3), np.float32))
    write_exr(val / "Emit" / "000_0001.exr", np.zeros((6, 8, 3), np.float32))
    with pytest.raises(IrisError, match="Emit.*001_0001.exr"):
        validation.validation_files("synthetic", str(tmp_path), None, "ldr", 1.0)
    write_exr(val / "Emit" / "001_0001.exr", np.zeros((5, 8, 3), np.float32))
    with pytest.raises(IrisError, match="5 x 8, the validation views 6 x 8"):
        validation.validation_files("synthetic", str(tmp_path), None, "ldr", 1.0)
    write_exr(val / "Emit" / "001_0001.exr", np.zeros((6, 8, 3), np.float32))
    files = validation.validation_files("synthetic", str(tmp_path), None, "ldr", 1.0)
    assert files["synthetic"] and files["img_hw"] == (6, 8) and len(files["views"]) == 2 and files["exposure"].tolist() == [0.5, 2.0]
    assert [os.path.basename(p) for p in files["diffcol"] + files["emit"]] == ["000_0001.exr", "001_0001.exr"] * 2
    with pytest.raises(IrisError, match="res_scale"):
        validation.validation_files("synthetic", str(tmp_path), None, "ldr", 0.5)
    with pytest.raises(IrisError, match="ldr_img_dir"):
        validation.validation_files("synthetic", str(tmp_path), None, None, 1.0)
