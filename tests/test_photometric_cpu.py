"""Host-side checks of the photometric step loss and of the emitter / initialisation stages: the float64 restatement agrees with itself, photometric_loss
validates before any device is touched, checkpoints carry `emitter.*`, the two command lines take the reference's arguments and refuse what is not built
before the device is opened.  Nothing here needs a GPU."""
import os

import numpy as np
import pytest
import torch

import photometric_ref64 as P
from iris_amd import _lib as L
from iris_amd.model.crf import EmorCRF


def crf_arrays(n=64):
    s = torch.linspace(0, 1, n)
    return s ** 0.45, torch.stack([torch.sin(3.14159 * s * (j + 1)) * 0.05 for j in range(3)])


def frozen_crf(n=64):
    crf = EmorCRF.from_arrays(*crf_arrays(n))
    crf.weight.requires_grad_(False)
    return crf


# ---- the float64 restatement
def test_identity_response_has_a_known_loss_and_gradient():
    """table = the knots themselves: rgb = clip(L e, 0, 1).  B = 2, n_calls = 2, e = 0.5: L_sum = 2 -> L e = 0.5; L_sum = 8 -> clamped to 1; -1 -> clamped to 0"""
    n = 17
    table = torch.linspace(0, 1, n).double().repeat(3, 1)
    L_sum = torch.tensor([[2.0, 8.0, -1.0], [2.0, 2.0, 2.0]])
    gt = torch.tensor([[0.25, 0.5, 0.5], [0.5, 0.5, 0.0]])
    loss, psnr, g = P.restatement(L_sum, 2, table, 0.5, gt)
    d = np.array([[0.25, 0.5, -0.5], [0.0, 0.0, 0.5]])
    assert loss == pytest.approx((d ** 2).sum() / 6, rel=1e-12) and psnr == pytest.approx(-10 * np.log10((d ** 2).sum() / 6), rel=1e-12)
    want = 2 * d / 6 * 0.5 / 2                     # slope 1, e = 0.5, n_calls = 2 ...
    want[0, 1] = want[0, 2] = 0.0                  # ... and zero where the response clamps
    np.testing.assert_allclose(g.numpy(), want, rtol=1e-12, atol=0)
    assert P.psnr_of(1e-7) == 50.0


@pytest.mark.parametrize("n_calls", [1, 4])
@pytest.mark.parametrize("exposure", ["number", "one", "per_ray"])
def test_closed_form_equals_autograd_in_float64(n_calls, exposure):
    g = torch.Generator().manual_seed(3)
    B = 97
    crf = frozen_crf()
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
        table = crf.get_crf()
    L_sum = (torch.rand(B, 3, generator=g) * 3 - 0.5) * n_calls
    L_sum[::7] = 0.0
    gt = torch.rand(B, 3, generator=g)
    e = {"number": 0.8, "one": torch.tensor([1.3]), "per_ray": 0.4 + torch.rand(B, 1, generator=g)}[exposure]
    loss, psnr, grad = P.restatement(L_sum, n_calls, table, e, gt)
    closed = P.closed_form(L_sum, n_calls, table, e, gt)
    assert float(grad.abs().max()) > 0 and int((grad == 0).sum()) > 0          # both the sloped part and the clamped ends are in the batch
    np.testing.assert_allclose(closed.numpy(), grad.numpy(), rtol=1e-12, atol=1e-18)
    # from_pieces on float64-exact pieces is the same number
    with torch.no_grad():
        import tools.crf_restatement as R
        rgb = R.forward(table.double(), L_sum.double() / n_calls, P._exposure(e, B))
    assert loss == pytest.approx(float(((rgb - gt.double()) ** 2).mean()), rel=1e-13)


# ---- host validation: nothing here may reach a device
def test_photometric_loss_validates_on_the_host(monkeypatch):
    from iris_amd.utils.losses import photometric_loss
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("photometric_loss reached the library with arguments it has to refuse"))
    crf = frozen_crf()
    x, gt = torch.rand(8, 3), torch.rand(8, 3)
    ok = dict(crf=crf, exposure=1.0, rgbs_gt=gt)
    with pytest.raises(L.IrisError, match="n_calls"):
        photometric_loss(x, 0, **ok)
    with pytest.raises(L.IrisError, match="n_calls"):
        photometric_loss(x, -3, **ok)
    with pytest.raises(L.IrisError, match=r"\(B, 3\)"):
        photometric_loss(torch.rand(8, 4), 1, **ok)
    with pytest.raises(L.IrisError, match=r"\(B, 3\)"):
        photometric_loss(torch.rand(24), 1, **ok)
    with pytest.raises(L.IrisError, match="rgbs_gt"):
        photometric_loss(x, 1, crf=crf, exposure=1.0, rgbs_gt=torch.rand(7, 3))
    with pytest.raises(L.IrisError, match="at least 1"):
        photometric_loss(torch.rand(0, 3), 1, crf=crf, exposure=1.0, rgbs_gt=torch.rand(0, 3))
    with pytest.raises(L.IrisError, match="exposure"):
        photometric_loss(x, 1, crf=crf, exposure=torch.rand(5), rgbs_gt=gt)
    with pytest.raises(L.IrisError, match="HIP device"):           # well-formed, but on the CPU: there is no CPU path
        photometric_loss(x, 1, **ok)
    trainable = EmorCRF.from_arrays(*crf_arrays())
    assert trainable.weight.requires_grad
    with pytest.raises(L.IrisError, match="brdf_crf_loss / initialize_loss"):
        photometric_loss(x, 1, crf=trainable, exposure=1.0, rgbs_gt=gt)


def test_abi_of_the_new_entry_points():
    import re
    from conftest import REPO
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "iris_hip.h")).read(), flags=re.S)
    m = re.search(r"IRIS_API\s+int\s+iris_loss_photometric\s*\(([^;]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == len(L.PROTOTYPES["iris_loss_photometric"]) == 16
    lib = L.lib()
    assert lib.iris_loss_photometric_workspace_bytes(1) == 8 and lib.iris_loss_photometric_workspace_bytes(257) == 16
    assert lib.iris_loss_photometric_workspace_bytes(8195) == 8 * 33 and lib.iris_loss_photometric_workspace_bytes(1 << 30) == 8 * 4096
    assert lib.iris_loss_photometric_workspace_bytes(0) == 0
    # refused by the library itself too, before any launch: null pointers, B = 0, n_calls = 0
    assert lib.iris_loss_photometric(None, 1, None, None, 64, None, 1, 1.0, None, 8, None, None, None, None, 0, None) != 0
    assert "iris_loss_photometric" in lib.iris_last_error().decode()


# ---- checkpoints
def _states():
    g = torch.Generator().manual_seed(1)
    material = {"mlp.params": torch.rand(100, generator=g)}
    crf = {"f0": torch.rand(1, 16, generator=g), "basis": torch.rand(3, 16, generator=g), "weight": torch.rand(3, 3, generator=g)}
    optimizer = {"state": {0: {"step": torch.tensor(3.0), "exp_avg": torch.rand(100, generator=g)}}, "param_groups": [{"lr": 1e-3, "params": [0]}]}
    return material, crf, optimizer


def test_checkpoint_round_trip_with_emitter_state(tmp_path):
    from iris_amd.utils.stage import read_checkpoint, write_checkpoint
    material, crf, optimizer = _states()
    radiance = torch.nn.Parameter(torch.rand(5, 3))
    path = tmp_path / "a" / "last.ckpt"
    write_checkpoint(path, material, crf, optimizer, epoch=2, global_step=9, hyper_parameters={"spp": 8}, emitter_state={"radiance": radiance})
    ck = read_checkpoint(path)
    assert set(ck["state_dict"]) == {"material.mlp.params", "model_crf.f0", "model_crf.basis", "model_crf.weight", "emitter.radiance"}
    assert set(ck["emitter"]) == {"radiance"} and torch.equal(ck["emitter"]["radiance"], radiance.detach()) and not ck["emitter"]["radiance"].requires_grad
    assert torch.equal(ck["material"]["mlp.params"], material["mlp.params"]) and set(ck["model_crf"]) == {"f0", "basis", "weight"}
    assert ck["epoch"] == 2 and ck["global_step"] == 9 and ck["hyper_parameters"] == {"spp": 8}
    # what extract_emitter_ldr --mode update does with it
    from iris_amd.extract_emitter_ldr import update
    torch.save({"emitter_radiance": torch.zeros(5, 3), "is_emitter": torch.zeros(7, dtype=torch.bool)}, tmp_path / "emitter.pth")
    update(str(tmp_path), str(path))
    assert torch.equal(torch.load(tmp_path / "emitter.pth")["emitter_radiance"], radiance.detach())


def test_checkpoint_without_emitter_state_is_what_it_was(tmp_path):
    """the parent commit's file, restated: exactly these five entries, the state_dict holding the two prefixes only, in this order"""
    from iris_amd.utils.stage import read_checkpoint, write_checkpoint
    material, crf, optimizer = _states()
    write_checkpoint(tmp_path / "b.ckpt", material, crf, optimizer, epoch=1, global_step=4, hyper_parameters={"la": 0.01})
    raw = torch.load(tmp_path / "b.ckpt", map_location="cpu", weights_only=False)
    assert list(raw) == ["state_dict", "optimizer_states", "epoch", "global_step", "hyper_parameters"]
    assert list(raw["state_dict"]) == ["material.mlp.params", "model_crf.f0", "model_crf.basis", "model_crf.weight"]
    want = {"state_dict": {**{"material." + k: v for k, v in material.items()}, **{"model_crf." + k: v for k, v in crf.items()}},
            "optimizer_states": [optimizer], "epoch": 1, "global_step": 4, "hyper_parameters": {"la": 0.01}}

    def same(a, b):
        if torch.is_tensor(a):
            return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
        if isinstance(a, dict):
            return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
        if isinstance(a, list):
            return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return type(a) is type(b) and a == b
    assert same(raw, want)
    ck = read_checkpoint(tmp_path / "b.ckpt")
    assert ck["emitter"] == {} and not any(k.startswith("emitter.") for k in ck["state_dict"])
    from iris_amd.extract_emitter_ldr import update
    torch.save({"emitter_radiance": torch.zeros(5, 3)}, tmp_path / "emitter.pth")
    with pytest.raises(L.IrisError, match="emitter.radiance"):
        update(str(tmp_path), str(tmp_path / "b.ckpt"))


# ---- the command lines
EXP, ROOT = "fipt_syn_bathroom", "/data/indoor_synthetic/bathroom"
INITIALIZE_ARGS = ["--experiment_name", EXP, "--max_epochs", "6", "--dataset", "synthetic", ROOT, "--voxel_path", f"checkpoints/{EXP}/bake/vslf.npz",
                   "--emitter_path", f"checkpoints/{EXP}/bake/emitter.pth", "--has_part", "1", "--ldr_img_dir", "Image", "--val_frame", "10", "--SPP", "128",
                   "--spp", "32", "--crf_basis", "3"]                                                    # scripts/fipt/*/train.sh: python initialize.py ...
TRAIN_EMITTER_ARGS = ["--experiment_name", EXP, "--max_epochs", "1", "--dir_val", "val_0_emitter", "--ckpt_path", f"checkpoints/{EXP}/last_0.ckpt",
                      "--voxel_path", f"checkpoints/{EXP}/bake/vslf_0.npz", "--emitter_path", f"checkpoints/{EXP}/bake/emitter.pth", "--dataset", "synthetic", ROOT,
                      "--has_part", "1", "--ldr_img_dir", "Image", "--val_frame", "10", "--SPP", "128", "--spp", "32", "--crf_basis", "3"]     # python train_emitter.py ...


def test_parsers_take_the_reference_scripts_argument_lists():
    from iris_amd import initialize, train_emitter
    a = initialize.parser().parse_args(INITIALIZE_ARGS)
    assert (a.max_epochs, a.dataset, a.has_part, a.ldr_img_dir, a.val_frame, a.SPP, a.spp, a.crf_basis) == (6, ["synthetic", ROOT], 1, "Image", 10, 128, 32, 3)
    assert a.ckpt_path is None and a.emitter_path.endswith("emitter.pth") and a.resume is False and a.batch_size == 8192 and a.learning_rate == 1e-3
    b = train_emitter.parser().parse_args(TRAIN_EMITTER_ARGS)
    assert (b.max_epochs, b.dir_val, b.SPP, b.spp, b.ckpt_path) == (1, "val_0_emitter", 128, 32, f"checkpoints/{EXP}/last_0.ckpt")
    assert train_emitter.parser().parse_args(TRAIN_EMITTER_ARGS + ["--resume", "--num_workers", "4", "--val_step", "100"]).resume is True
    # the options are configs/config.py's, shared with the BRDF-CRF stage, not a copy
    from iris_amd import train_brdf_crf
    assert train_emitter.DEFAULT_OPTIONS is train_brdf_crf.DEFAULT_OPTIONS and train_emitter.multistep_lr is train_brdf_crf.multistep_lr
    assert train_emitter.make_optimizer is train_brdf_crf.make_optimizer


def test_refusals_come_before_the_device(tmp_path, capsys, monkeypatch):
    from iris_amd import initialize, train_emitter
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a refused command opened the device"))
    torch.save({}, tmp_path / "vslf.npz")
    torch.save({}, tmp_path / "emitter.pth")
    files = ["--voxel_path", str(tmp_path / "vslf.npz"), "--emitter_path", str(tmp_path / "emitter.pth")]
    common = ["--experiment_name", "x", "--checkpoint_path", str(tmp_path / "c"), "--log_path", str(tmp_path / "l")]
    for mod in (train_emitter, initialize):
        ckpt = ["--ckpt_path", str(tmp_path / "in.ckpt")] if mod is train_emitter else []
        full = common + files + ckpt + ["--ldr_img_dir", "ldr"]
        assert mod.cli(common + files + ckpt + ["--ldr_img_dir", "ldr", "--dataset", "scannetpp", str(tmp_path), "--scene", "room"]) == 2
        assert "scannetpp" in capsys.readouterr().err
        assert mod.cli(full + ["--dataset", "real", str(tmp_path), "--res_scale", "0.5"]) == 2
        assert "res_scale" in capsys.readouterr().err
        assert mod.cli(common + files + ckpt + ["--dataset", "real", str(tmp_path)]) == 2
        assert "ldr_img_dir" in capsys.readouterr().err
        assert mod.cli(full + ["--dataset", "real", str(tmp_path), "--optimizer", "Ranger"]) == 2
        assert "Ranger" in capsys.readouterr().err
        assert mod.cli(common + ckpt + ["--ldr_img_dir", "ldr", "--dataset", "real", str(tmp_path), "--voxel_path", str(tmp_path / "vslf.npz")]) == 2
        assert "emitter_path" in capsys.readouterr().err
        assert mod.cli(common + ckpt + ["--ldr_img_dir", "ldr", "--dataset", "real", str(tmp_path), "--emitter_path", str(tmp_path / "emitter.pth")]) == 2
        assert "voxel_path" in capsys.readouterr().err
        assert mod.cli(full + ["--dataset", "real", str(tmp_path), "--SPP", "4", "--spp", "8"]) == 2
        assert "SPP" in capsys.readouterr().err
    assert train_emitter.cli(common + files + ["--ldr_img_dir", "ldr", "--dataset", "real", str(tmp_path)]) == 2
    assert "ckpt_path" in capsys.readouterr().err
    assert not (tmp_path / "c").exists() and not (tmp_path / "l").exists()


def test_trainer_refuses_a_bad_mode_and_zero_calls():
    from iris_amd.train_emitter import RadianceTrainer, default_hparams
    with pytest.raises(L.IrisError, match="mode"):
        RadianceTrainer(None, None, None, None, None, default_hparams(), "brdf")
    with pytest.raises(L.IrisError, match="SPP"):
        RadianceTrainer(None, None, None, None, None, default_hparams(SPP=4, spp=8), "emitter")
    with pytest.raises(KeyError):
        default_hparams(cache_dir="x")
