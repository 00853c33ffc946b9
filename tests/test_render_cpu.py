"""The render stage's fixture and command line without a GPU: tests/golden/render_intrinsics.npz (tools/make_render_golden.py: the reference's render.py:178-220
through its own functions, float32 and float64) and `python -m iris_amd.render`'s argument parser."""
import numpy as np
import torch

from render_formula import MAPS, U, fixture, pixel_means, sample_terms


def _rounds(f):
    return range(int(f["rounds"]))


def test_fixture_loads_and_is_small():
    import os
    from conftest import GOLDEN
    f = fixture()
    B, spp = int(f["H"]) * int(f["W"]), int(f["spp"])
    assert (B, spp, int(f["rounds"])) == (24 * 16, 5, 2)
    assert os.path.getsize(os.path.join(GOLDEN, "render_intrinsics.npz")) < 512 * 1024
    for r in _rounds(f):
        for k, c in (("pos", 3), ("nrm", 3), ("wo", 3), ("albedo", 3), ("u2", 2), ("roughness", 1), ("metallic", 1)):
            assert f[f"{k}_{r}"].shape == (B * spp, c) and f[f"{k}_{r}"].dtype == np.float32, k
        assert f[f"dudv_{r}"].shape == (2, B, spp, 1) and f[f"e0_{r}"].dtype == np.int32 and f[f"valid_next_{r}"].dtype == np.bool_
    for k, c in MAPS:
        assert f[f"map32_{k}"].shape == (B, c) and f[f"map32_{k}"].dtype == np.float32 and f[f"map64_{k}"].dtype == np.float64


def test_fixture_holds_the_five_sample_classes():
    """misses, kept surfaces, real emitters, zero-sum emitters (both rows) and empty voxels under a hit: at least 1 % of the samples each; the material reaches
    roughness 0.02 and 1.0 and metallic 0 and 1"""
    f = fixture()
    e0 = np.concatenate([f[f"e0_{r}"] for r in _rounds(f)]); vn = np.concatenate([f[f"valid_next_{r}"] for r in _rounds(f)])
    keep = np.concatenate([f[f"keep_{r}"] for r in _rounds(f)]); vox = np.concatenate([f[f"voxel_{r}"] for r in _rounds(f)])
    rad = f["emitter_radiance"]
    assert rad[2].tolist() == [0, 0, 0] and rad[3].tolist() == [1, -1, 0] and rad[0].sum() > 0
    hit = vn | (e0 >= 0)
    shares = {"miss": (~hit).mean(), "kept surface": (keep & (e0 < 0)).mean(), "real emitter": ((e0 >= 0) & (e0 < 2)).mean(), "zero-sum emitter (0,0,0)": (e0 == 2).mean(),
              "zero-sum emitter (1,-1,0)": (e0 == 3).mean(), "empty voxel under a hit": (hit & (vox < 0)).mean()}
    print(shares)
    for k, s in shares.items():
        assert s >= 0.01, (k, s)
    assert keep[e0 >= 2].all() and not keep[(e0 >= 0) & (e0 < 2)].any() and not keep[~hit].any()
    rg = np.concatenate([f[f"roughness_{r}"] for r in _rounds(f)]); mt = np.concatenate([f[f"metallic_{r}"] for r in _rounds(f)])
    assert rg.min() == np.float32(0.02) and rg.max() == 1.0 and mt.min() == 0.0 and mt.max() == 1.0


def test_float32_and_float64_maps_agree_and_the_formula_restates_the_reference():
    """d32 per map (the reference's float32 run against its float64 run) is rounding-sized except where the GGX terms are ill-conditioned (a_prime at roughness
    0.02), and the documented formula (tests/render_formula.py) in float64 reproduces the reference's float64 maps: the kernel's contract IS render.py:189-220"""
    f = fixture()
    spp = int(f["spp"])
    acc = {k: 0 for k, _ in MAPS}
    for r in _rounds(f):
        x, keep = sample_terms(torch.float64, *(f[f"{k}_{r}"] for k in ("pos", "nrm", "wo", "e0", "valid_next", "albedo", "roughness", "metallic", "u2")),
                               f["emitter_radiance"], f["slf_inds"], f["slf_radiance"], float(f["voxel_min"]), float(f["voxel_max"]))
        assert np.array_equal(keep.numpy(), f[f"keep_{r}"])
        for k, _ in MAPS:
            acc[k] = acc[k] + pixel_means(x[k], spp)
    for k, _ in MAPS:
        d32 = float(np.abs(f[f"map32_{k}"].astype(np.float64) - f[f"map64_{k}"]).max())
        restated = float((acc[k] - torch.from_numpy(f[f"map64_{k}"])).abs().max())
        print(f"{k}: d32 {d32:.3g}, formula (float64) against the reference's float64 run {restated:.3g}, max |map| {float(np.abs(f[f'map64_{k}']).max()):.3g}")
        assert d32 <= (1e-3 if k == "a_prime" else 64 * U * max(1.0, float(np.abs(f[f"map64_{k}"]).max())))
        assert restated <= 1e-9
    assert np.isfinite(np.concatenate([f[f"map32_{k}"].ravel() for k, _ in MAPS])).all()


def test_parser_accepts_the_reference_argument_lists():
    """scripts/fipt/kitchen/render.sh and scripts/scannetpp/room2/render.sh, argument for argument"""
    from iris_amd.render import build_parser
    a = build_parser().parse_args("--experiment_name fipt_syn_kitchen --device 0 --ckpt last_1.ckpt --dataset synthetic /data/kitchen --emitter_path checkpoints/e/bake "
                                  "--output_path outputs/e/output --split val --ldr_img_dir Image --SPP 256 --spp 16 --crf_basis 3".split())
    assert a.dataset == ["synthetic", "/data/kitchen"] and (a.SPP, a.spp, a.crf_basis, a.indir_depth, a.light_type) == (256, 16, 3, 5, "slf")
    b = build_parser().parse_args("--experiment_name scannetpp_room2 --device 0 --ckpt last_1.ckpt --dataset scannetpp /data/scannetpp/ --scene 7e09430da7 --res_scale 0.5 "
                                  "--emitter_path checkpoints/e/bake --output_path outputs/e/output --split test --SPP 256 --spp 16 --crf_basis 3".split())
    assert b.scene == "7e09430da7" and b.res_scale == 0.5 and b.split == "test" and b.checkpoint_path == "./checkpoints"


def test_psnr_closed_form():
    from iris_amd.render import psnr
    a = np.zeros((4, 4, 3)); b = np.full((4, 4, 3), 0.1)
    assert abs(psnr(a, b) - 20.0) < 1e-9 and psnr(a, a) == float("inf")
