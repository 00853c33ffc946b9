"""The trainers' validation on the GPU (iris_amd/csrc/iris_validate.h, iris_amd/utils/validation.py): both kernels against their numpy restatement
(tests/validation_ref.py), the validation set, the two trainers with validate='all', and the three command lines.

Fixtures: the open box of tests/test_train_brdf_crf.py with the emitter file of tests/test_train_emitter.py, here with one radiance row that sums to zero
(that ceiling triangle stays a surface), and a fourth camera that looks at the ceiling."""
import json
import os

import numpy as np
import pytest
import torch

import validation_ref as R
from test_train_brdf_crf import BATCH, BOX_F, BOX_V, H, N, V, VMAX, VMIN, W, cameras, emor_arrays, look_at, stores, write_real_scene
from test_train_emitter import cli_scene, run_module, write_emitter_files

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HALF_DARK = np.array([[6.0, 5.0, 4.0], [0.0, 0.0, 0.0]], np.float32)          # the second ceiling triangle's row sums to zero


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


# ---- iris_val_kd_loss
def loss_inputs(N_, hw, synthetic, seed=0):
    g = np.random.default_rng(seed + 31 * N_ + hw[0] * hw[1] + 2 * synthetic)
    n = N_ * hw[0] * hw[1]
    d = dict(albedo=g.random((n, 3), np.float32), metallic=g.random(n, np.float32), valid=g.random(n) >= 0.2)
    if synthetic:
        emit = np.where(g.random((n, 1)) < 0.25, g.random((n, 3), np.float32) * np.float32(4.0), np.float32(0.0)).astype(np.float32)
        d.update(gt=g.random((n, 3), np.float32), emit=emit)
    else:
        codes = g.integers(0, 256, (n, 3)).astype(np.uint8)
        if codes.size >= 256:
            codes.reshape(-1)[:256] = g.permutation(256).astype(np.uint8)      # every code is there
        d.update(codes=codes)
    return d


def on_device(d):
    return {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}


def device_loss(d, hw, rows=slice(None)):
    from iris_amd.utils.validation import kd_validation_loss
    t = on_device(d)
    hw_n = hw[0] * hw[1]
    cut = lambda a: a.reshape(-1, hw_n, *a.shape[1:])[rows].contiguous()
    truth = {k: cut(t[k]) for k in ("gt", "emit", "codes") if k in t}
    return kd_validation_loss(cut(t["albedo"]), cut(t["metallic"]), cut(t["valid"]), img_hw=hw, **truth)


@pytest.mark.parametrize("synthetic", [True, False], ids=["synthetic", "ldr"])
@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (7, 73), (16, 32), (19, 27), (12, 16)], ids=["1", "511", "512", "513", "192"])
def test_kd_loss_against_the_restatement(hw, n_views, synthetic):
    """|dS| <= S 3HW 2^-53: two float64 sums of the same 3HW float32 squares in different orders"""
    from iris_amd.utils.validation import gamma_table
    d = loss_inputs(n_views, hw, synthetic)
    if not synthetic and d["codes"].size >= 256:
        assert len(np.unique(d["codes"])) == 256
    truth = dict(gt=d["gt"], emit=d["emit"]) if synthetic else dict(codes=d["codes"], lut=gamma_table())
    want = R.kd_loss_sums(d["albedo"], d["metallic"], d["valid"], hw, **truth)
    out = device_loss(d, hw)
    S = out["S"].cpu().numpy()
    n3 = 3 * hw[0] * hw[1]
    print(f"N {n_views}, {hw[0]} x {hw[1]}, {'synthetic' if synthetic else 'ldr'}: S {S.tolist()}, restatement {want.tolist()}, "
          f"|dS| / (S 3HW 2^-53) {(np.abs(S - want) / np.maximum(want * n3 * 2.0 ** -53, 1e-300)).max():.3g}")
    assert S.shape == (n_views,) and out["S"].dtype == torch.float64 and (want.sum() > 0 if hw == (1, 1) else (want > 0).all())
    assert (np.abs(S - want) <= want * n3 * 2.0 ** -53).all()
    loss, psnr = R.loss_and_psnr(S, hw)
    assert np.array_equal(out["loss"].cpu().numpy(), loss)                                 # one correctly rounded float64 division
    assert np.allclose(out["psnr"].cpu().numpy(), psnr, rtol=0, atol=1e-10)
    assert torch.equal(bits(device_loss(d, hw)["S"]), bits(out["S"]))                      # two calls: the same bits
    for n in range(n_views):                                                               # a view alone is its row of the stack
        assert torch.equal(bits(device_loss(d, hw, slice(n, n + 1))["S"]), bits(out["S"][n:n + 1]))


@pytest.mark.parametrize("hw", [(1, 1), (19, 27)])
def test_kd_loss_is_exactly_zero_where_nothing_counts(hw):
    d = loss_inputs(2, hw, True)
    d["emit"][:] = 1.0                                                                     # all masked: every pixel is emissive
    assert device_loss(d, hw)["S"].tolist() == [0.0, 0.0]
    d = loss_inputs(2, hw, False)
    d["valid"][:] = False                                                                  # all invalid, against a black photograph
    d["codes"][:] = 0
    d["albedo"][:] = np.nan                                                                # what the network returns there is never used
    out = device_loss(d, hw)
    assert out["S"].tolist() == [0.0, 0.0] and out["loss"].tolist() == [0.0, 0.0] and out["psnr"].tolist() == pytest.approx([50.0, 50.0], abs=1e-9)      # the clamp at 1e-5
    d = loss_inputs(2, hw, True)
    d["valid"][:] = False
    d["gt"][:] = 0.0
    assert device_loss(d, hw)["S"].tolist() == [0.0, 0.0]


def test_kd_loss_refuses_on_the_device():
    from iris_amd import _lib as L
    from iris_amd.utils.validation import kd_validation_loss
    t = on_device(loss_inputs(1, (2, 3), False))
    with pytest.raises(L.IrisError, match="dtype"):
        kd_validation_loss(t["albedo"].double(), t["metallic"], t["valid"], codes=t["codes"], img_hw=(2, 3))
    with pytest.raises(L.IrisError, match="dtype"):
        kd_validation_loss(t["albedo"], t["metallic"], t["valid"], codes=t["codes"].float(), img_hw=(2, 3))
    with pytest.raises(L.IrisError, match="values expected"):
        kd_validation_loss(t["albedo"][:5], t["metallic"], t["valid"], codes=t["codes"], img_hw=(2, 3))
    with pytest.raises(L.IrisError, match="HIP device"):
        kd_validation_loss(t["albedo"].cpu(), t["metallic"], t["valid"], codes=t["codes"], img_hw=(2, 3))


# ---- iris_val_intrinsics
@pytest.fixture(scope="module")
def box(tmp_path_factory):
    """(scene, emitter with a zero-sum row, material, the 4 x 192 rays with their differentials)"""
    from iris_amd.model.brdf import NGPBRDF
    from iris_amd.model.emitter import SLFEmitter
    from iris_amd.utils.cameras import view_rays
    from iris_amd.utils.path_tracing import Scene
    root = tmp_path_factory.mktemp("box")
    ep, sp = write_emitter_files(root, HALF_DARK)
    scene = Scene(BOX_V, BOX_F, device=DEV)
    emitter = SLFEmitter(ep, sp).to(DEV)
    material = NGPBRDF(VMIN, VMAX).init_parameters(seed=5).to(DEV)
    for p in material.parameters():
        p.requires_grad_(False)
    up = dict(kind="real", K=np.array([[6.0, 0, 8.0], [0, 6.0, 6.0], [0, 0, 1]], np.float32), c2w=look_at((0.0, 0.0, 0.0), (0.1, 1.0, 0.05), up=(0.0, 0.0, 1.0)))
    rays = [view_rays(v, (H, W), DEV, ray_diff=True) for v in cameras() + [up]]
    rays = [torch.cat([r[k] for r in rays]) for k in range(4)]
    rays[1] = torch.nn.functional.normalize(rays[1], dim=-1)
    return scene, emitter, material, rays


def pick(rays, B):
    """B rays spread over the four views"""
    idx = torch.linspace(0, rays[0].shape[0] - 1, B, device=DEV).round().long()
    return [r[idx].contiguous() for r in rays]


@pytest.mark.parametrize("spp", [1, 3, 8])
@pytest.mark.parametrize("B", [67, 192])
def test_val_intrinsics_against_the_restatement_bit_for_bit(box, B, spp):
    from iris_amd.utils.validation import MAPS, validation_intrinsics
    scene, emitter, material, rays = box
    ro, rd, dxdu, dydv = pick(rays, B)
    g = torch.Generator().manual_seed(100 * B + spp)
    draws = [torch.rand(2, B, spp, 1, generator=g).to(DEV)]
    debug = {}
    out = validation_intrinsics(scene, emitter, material, ro, rd, dxdu, dydv, spp, uniforms=draws, debug=debug)
    host = {k: v.cpu().numpy() for k, v in debug.items()}
    radiance = emitter.radiance_on(DEV).cpu().numpy()
    e0, vn = host["e0"], host["valid_next"]
    lit, dark, miss = int((e0 == 0).sum()), int((e0 == 1).sum()), int(((e0 < 0) & ~vn.astype(bool)).sum())
    print(f"B {B}, spp {spp}: {lit} samples on the lit ceiling triangle, {dark} on the zero-sum one, {miss} through the opening, {e0.size - lit - dark - miss} on the walls")
    assert np.array_equal(radiance, HALF_DARK) and (B * spp < 192 or min(lit, dark, miss, e0.size - lit - dark - miss) > 0)
    want = R.val_intrinsics(radiance, e0, vn, host["albedo"], host["roughness"], host["metallic"], spp)
    for k, c in MAPS:
        assert out[k].shape == (B, c) and np.array_equal(out[k].cpu().numpy().view(np.int32), want[k].view(np.int32)), k
    assert float(out["albedo"].abs().max()) > 0 and float(out["emission"].max()) > 0
    # chunked equals unchunked; a second round adds to the first
    chunked = validation_intrinsics(scene, emitter, material, ro, rd, dxdu, dydv, spp, uniforms=draws, chunk=50)
    again = validation_intrinsics(scene, emitter, material, ro, rd, dxdu, dydv, spp, uniforms=draws, out={k: v.clone() for k, v in out.items()})
    twice = R.val_intrinsics(radiance, e0, vn, host["albedo"], host["roughness"], host["metallic"], spp, maps=want)
    for k, _ in MAPS:
        assert torch.equal(chunked[k], out[k]), k
        assert np.array_equal(again[k].cpu().numpy().view(np.int32), twice[k].view(np.int32)), k


def test_val_intrinsics_masks_by_selection(box):
    """a masked sample counts as 0 whatever the network returns there: the reference's product with 0 would make it NaN"""
    from iris_amd.utils.validation import validation_intrinsics
    scene, emitter, material, rays = box
    ro, rd, dxdu, dydv = pick(rays, 192)
    draws = [torch.rand(2, 192, 2, 1, generator=torch.Generator().manual_seed(3)).to(DEV)]

    def poisoned(pos):
        out = {k: v.clone() for k, v in material(pos).items()}
        out["albedo"][(pos == 0).all(-1)] = float("inf")                   # the position the intersector gives a miss
        return out
    debug = {}
    plain = validation_intrinsics(scene, emitter, material, ro, rd, dxdu, dydv, 2, uniforms=draws, debug=debug)
    bad = validation_intrinsics(scene, emitter, poisoned, ro, rd, dxdu, dydv, 2, uniforms=draws)
    assert int(((debug["e0"] < 0) & ~debug["valid_next"]).sum()) > 0
    assert torch.equal(plain["albedo"], bad["albedo"]) and bool(torch.isfinite(bad["albedo"]).all())


# ---- the validation set
def validation_set(scene, emitter=None, synthetic=False, stack=None):
    from iris_amd.utils.validation import ValidationSet
    g = np.random.default_rng(17)
    codes = g.integers(0, 256, (V, H, W, 3)).astype(np.uint8)
    codes[0, :2, :2] = 255
    more = dict(diffcol=g.random((V, H, W, 3), np.float32), emit=np.where(g.random((V, H, W, 1)) < 0.2, np.float32(2.0), np.float32(0.0)) * np.ones(3, np.float32)) if synthetic else {}
    return ValidationSet(cameras(), (H, W), codes, np.array([0.7, 1.0, 1.3], np.float32), scene, emitter=emitter, device=DEV, stack=stack, **more), codes


@pytest.mark.parametrize("synthetic", [False, True], ids=["ldr", "synthetic"])
def test_validation_set_scores_every_view_and_logs_their_mean(box, synthetic):
    from iris_amd.utils.path_tracing import ray_intersect
    from iris_amd.utils.validation import gamma_table
    scene, emitter, material, _ = box
    vs, codes = validation_set(scene, synthetic=synthetic)
    assert len(vs) == V and vs.positions.shape == (V, H * W, 3) and 0 < int(vs.valid[0].sum()) < H * W            # view 0 looks out of the opening
    per = vs.per_view(material)
    with torch.no_grad():
        mat = material(vs.positions.reshape(-1, 3))
    truth = dict(gt=vs.diffcol.cpu().numpy(), emit=vs.emit.cpu().numpy()) if synthetic else dict(codes=codes, lut=gamma_table())
    want = R.kd_loss_sums(mat["albedo"].cpu().numpy(), mat["metallic"].cpu().numpy(), vs.valid.cpu().numpy(), (H, W), **truth)
    S = per["S"].cpu().numpy()
    assert (np.abs(S - want) <= want * 3 * H * W * 2.0 ** -53).all() and (want > 0).all()
    one, _ = validation_set(scene, synthetic=synthetic, stack=1)                    # a view per launch: the same bits as the stack of three
    assert one.stack == 1 and vs.stack >= V and torch.equal(bits(one.per_view(material)["S"]), bits(per["S"]))
    out = vs.evaluate(None, material)
    loss, psnr = R.loss_and_psnr(S, (H, W))
    assert abs(float(out["val/loss"]) - float(loss.mean())) <= float(loss.mean()) * V * 2.0 ** -53 and float(out["val/psnr"]) == pytest.approx(float(psnr.mean()), abs=1e-10)
    assert out["val/loss"].dtype == torch.float64 and out["val/loss"].is_cuda
    again = vs.evaluate(scene, material)
    assert float(again["val/loss"]) == float(out["val/loss"]) and float(again["val/psnr"]) == float(out["val/psnr"])


# ---- the trainers
def png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


def check_images(folder, steps, codes):
    from iris_amd.utils.validation import IMAGE_NAMES
    assert sorted(os.listdir(folder)) == sorted("{:05d}_{}.png".format(s, n) for s in steps for n in IMAGE_NAMES)
    for s in steps:
        images = {n: png(os.path.join(folder, "{:05d}_{}.png".format(s, n))) for n in IMAGE_NAMES}
        assert all(a.shape == (H, W, 3) for a in images.values())
        assert np.array_equal(images["L_gt"], codes)
        assert set(np.unique(images["mask"])) <= {0, 255}
        assert images["mat_albedo"].max() > 0 and images["L_full"].max() > 0


def check_run(tr, tmp_path, steps_per_epoch, epochs):
    from iris_amd.model.brdf import load_ngpbrdf
    val = [e for e in tr.history if "val/loss" in e]
    assert [(e["epoch"], e["step"]) for e in val] == [(k + 1, (k + 1) * steps_per_epoch) for k in range(epochs)]
    assert all(set(e) == {"step", "epoch", "val/loss", "val/psnr"} and np.isfinite(e["val/loss"]) and np.isfinite(e["val/psnr"]) for e in val)
    print("val/loss", [e["val/loss"] for e in val], "val/psnr", [e["val/psnr"] for e in val])
    lines = [json.loads(l) for l in open(tmp_path / "logs" / "exp" / "metrics.jsonl")]
    assert lines == tr.history and len([e for e in lines if tr.prefix + "/loss" in e]) == epochs * steps_per_epoch
    again = tr.validation.evaluate(None, tr.material)                     # the same parameters: the same bits
    assert float(again["val/loss"]) == val[-1]["val/loss"] and float(again["val/psnr"]) == val[-1]["val/psnr"]
    folder = tmp_path / "checkpoints" / "exp"
    assert sorted(os.listdir(folder)) == ["best.ckpt", "best.json", "last.ckpt"]
    best = json.load(open(folder / "best.json"))
    k = int(np.argmin([e["val/loss"] for e in val]))
    assert best == {"val/loss": val[k]["val/loss"], "epoch": val[k]["epoch"], "step": val[k]["step"]}
    state = torch.load(folder / "best.ckpt", map_location="cpu", weights_only=False)
    assert list(state) == ["state_dict", "optimizer_states", "epoch", "global_step", "hyper_parameters"] and state["epoch"] == best["epoch"]
    assert list(torch.load(folder / "last.ckpt", map_location="cpu", weights_only=False)) == list(state)
    loaded = load_ngpbrdf(VMIN, VMAX, str(folder / "best.ckpt")).to(DEV)
    assert float(tr.validation.evaluate(None, loaded)["val/loss"]) == best["val/loss"]


def test_brdf_crf_trainer_validates(box, tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    from iris_amd.model.brdf import NGPBRDF
    from iris_amd.model.crf import EmorCRF
    from iris_amd.train_brdf_crf import BRDFCRFTrainer, default_hparams
    from iris_amd.utils.dataset import PixelSet
    from iris_amd.utils.shading_cache import ShadingCache
    scene, emitter, _, _ = box
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    st = stores()
    ps = PixelSet(cameras(), (H, W), st["rgb"], segmentation=st["segmentation"], int_albedo=st["int_albedo"], exposure=st["exposure"], batch_size=BATCH, device=DEV)
    cache = ShadingCache(N, 6, DEV)
    cache.rows.copy_(torch.rand(cache.rows.shape, generator=torch.Generator().manual_seed(8)).to(DEV))
    ps.attach_cache(cache)
    ps.restrict_to_hits(scene, store_positions=True)
    material = NGPBRDF(VMIN, VMAX).init_parameters(seed=5).to(DEV)
    crf = EmorCRF.from_arrays(*emor_arrays()).to(DEV)
    vs, codes = validation_set(scene, emitter=emitter)
    hp = default_hparams(batch_size=BATCH, experiment_name="exp", checkpoint_path=str(tmp_path / "checkpoints"), log_path=str(tmp_path / "logs"), has_part=0, la=0.01,
                         learning_rate=1e-2, log_every=1, validate="all", val_step=2, val_frame=1, dir_val="val_1", SPP=8, spp=4)
    tr = BRDFCRFTrainer(material, crf, ps, hp, validation=vs)
    steps = len(ps)
    tr.fit(2)
    check_run(tr, tmp_path, steps, 2)
    check_images(tmp_path / "outputs" / "exp" / "val_1", range(0, 2 * steps, 2), codes[1])


def test_radiance_trainer_validates(box, tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    import test_train_emitter as E
    scene = box[0]
    monkeypatch.chdir(tmp_path)
    plain = E.make_trainer(tmp_path, "emitter", SPP=8, spp=4)
    vs, codes = validation_set(plain.scene)
    from iris_amd.train_emitter import RadianceTrainer
    hp = dict(plain.hparams, validate="all", val_step=2, val_frame=0, dir_val="val_0")
    tr = RadianceTrainer(plain.scene, plain.emitter, plain.material, plain.model_crf, plain.ps, hp, "emitter", validation=vs)
    steps = len(tr.ps)
    tr.fit(2)
    check_run(tr, tmp_path, steps, 2)
    val = [e["val/loss"] for e in tr.history if "val/loss" in e]
    assert val[0] == val[1] and json.load(open(tmp_path / "checkpoints" / "exp" / "best.json"))["epoch"] == 1       # the material is frozen: equal losses, the first stays
    check_images(tmp_path / "outputs" / "exp" / "val_0", range(0, 2 * steps, 2), codes[0])
    assert scene is not None


# ---- the command lines
def validated_scene(tmp_path):
    """cli_scene's files and the photograph of view 0, the real layout's validation split here"""
    from iris_amd.utils.texture import write_png
    scene, ep, sp, common = cli_scene(tmp_path)
    codes = np.random.default_rng(5).integers(0, 256, (H, W, 3)).astype(np.uint8)
    write_png(scene / "ldr" / "000_0001.png", codes)
    return scene, ep, sp, common, codes


def stage_args(stage, tmp_path, ep, sp, common):
    if stage == "train_brdf_crf":
        return ["--experiment_name", "cli", "--cache_dir", str(tmp_path / "shading"), "--la", "0.01"] + common
    if stage == "train_emitter":
        from iris_amd.model.brdf import NGPBRDF
        from iris_amd.model.crf import EmorCRF
        from iris_amd.utils.stage import write_checkpoint
        write_checkpoint(tmp_path / "in.ckpt", NGPBRDF(VMIN, VMAX).init_parameters(seed=9).state_dict(), EmorCRF(dim=3, emor_path=tmp_path / "crf" / "emor.txt").state_dict(),
                         {}, epoch=1, global_step=5, hyper_parameters={})
        return ["--experiment_name", "cli", "--ckpt_path", str(tmp_path / "in.ckpt")] + common
    return ["--experiment_name", "cli"] + common


def files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("stage", ["train_brdf_crf", "train_emitter", "initialize"])
def test_cli_validates(tmp_path, stage):
    from iris_amd.utils.validation import IMAGE_NAMES
    scene, ep, sp, common, codes = validated_scene(tmp_path)
    before = files_under(tmp_path)
    p = run_module("iris_amd." + stage, stage_args(stage, tmp_path, ep, sp, common) + ["--validate", "all", "--val_step", "2"], tmp_path)
    assert p.returncode == 0
    assert "accepted and ignored (no in-training validation images" not in p.stdout and "--validate all" in p.stdout and "best val/loss" in p.stdout
    ck = torch.load(tmp_path / "checkpoints" / "cli" / "last.ckpt", map_location="cpu", weights_only=False)
    steps = ck["global_step"]
    lines = [json.loads(l) for l in open(tmp_path / "logs" / "cli" / "metrics.jsonl")]
    val = [e for e in lines if "val/loss" in e]
    assert val == [lines[-1]] and val[0]["epoch"] == 1 and val[0]["step"] == steps and np.isfinite(val[0]["val/loss"]) and len(lines) == steps + 1
    assert json.load(open(tmp_path / "checkpoints" / "cli" / "best.json")) == {"val/loss": val[0]["val/loss"], "epoch": 1, "step": steps}
    new = sorted(set(files_under(tmp_path)) - set(before) - {"in.ckpt"})
    images = [os.path.join("outputs", "cli", "val_0", "{:05d}_{}.png".format(s, n)) for s in range(0, steps, 2) for n in IMAGE_NAMES]
    assert new == sorted([os.path.join("checkpoints", "cli", f) for f in ("best.ckpt", "best.json", "last.ckpt")] + [os.path.join("logs", "cli", "metrics.jsonl")] + images)
    assert np.array_equal(png(tmp_path / images[2]), codes)                       # (L_gt of step 0)


@pytest.mark.parametrize("stage", ["train_brdf_crf", "train_emitter", "initialize"])
def test_cli_without_the_option_writes_what_it_wrote(tmp_path, stage):
    scene, ep, sp, common, _ = validated_scene(tmp_path)
    before = files_under(tmp_path)
    p = run_module("iris_amd." + stage, stage_args(stage, tmp_path, ep, sp, common), tmp_path)
    assert p.returncode == 0
    assert "accepted and ignored (no in-training validation images" in p.stdout and "val/loss" not in p.stdout
    new = sorted(set(files_under(tmp_path)) - set(before) - {"in.ckpt"})
    assert new == [os.path.join("checkpoints", "cli", "last.ckpt"), os.path.join("logs", "cli", "metrics.jsonl")]
    assert all("val/loss" not in json.loads(l) for l in open(tmp_path / "logs" / "cli" / "metrics.jsonl"))
