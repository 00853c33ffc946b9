"""The render stage's SSIM column (iris_amd/render.py --metrics psnr,ssim): the reference's three-column rgb/metrics.txt, its SSIM the device metric of
(gt, rgb_ldr), checked against the float64 restatement of the contract (tests/ssim_ref64.py) at the file's print precision."""
import json

import numpy as np
import pytest
import torch

from ssim_ref64 import ssim_ref64
from test_render import DEV, setup, write_emitter_files

pytestmark = pytest.mark.gpu


def test_cli_writes_the_ssim_column(tmp_path, capsys):
    """python -m iris_amd.render --metrics psnr,ssim on tests/test_render.py's room at 24 x 16, SPP 4, spp 2, indir_depth 2, stub material, a non-constant
    photograph: header, view row and mean row of the reference's file; the SSIM written equals ssim_ref64(gt, rgb_ldr) of the same view through render_view with
    the CLI's seed to 1e-5 (the file's precision; the kernel's own bound is tests/test_metrics.py's); without "ssim" render_view returns None for it"""
    from iris_amd import render as R
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils.cameras import view_rays
    from iris_amd.utils.exr import write_exr
    from iris_amd.utils.stage import read_image
    from stub_material import StubMaterial
    f, scene, em = setup()
    H, W = int(f["H"]), int(f["W"])
    data, bake, ckpt_dir, outp = tmp_path / "data", tmp_path / "bake", tmp_path / "ckpt" / "exp", tmp_path / "out"
    for d in (data, bake, ckpt_dir):
        d.mkdir(parents=True)
    with open(data / "scene.obj", "w") as fh:
        fh.writelines("v {:.9g} {:.9g} {:.9g}\n".format(*v) for v in f["verts"].tolist())
        fh.writelines("f {} {} {}\n".format(*(i + 1 for i in t)) for t in f["faces"].tolist())
    write_emitter_files(f, str(bake), "vslf_0.npz")
    write_emitter_files(f, str(bake), "vslf.npz")
    s = torch.linspace(0, 1, 1024)
    crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (k + 1)) * 0.05 for k in range(3)]))
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
    torch.save({"state_dict": {"model_crf." + k: v for k, v in crf.state_dict().items()}}, ckpt_dir / "last.ckpt")
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.clip(0.5 + 0.3 * np.sin(0.4 * xx + 0.2 * yy)[..., None] * np.array([1.0, 0.7, -0.5]) + 0.05 * np.random.default_rng(5).standard_normal((H, W, 3)), 0, 1).astype(np.float32)
    write_exr(str(data / "gt.exr"), gt, "none")
    with open(data / "cameras.json", "w") as fh:
        json.dump({"img_hw": [H, W], "views": [{"K": f["K"].tolist(), "c2w": f["c2w"].tolist(), "image": "gt.exr", "exposure": 1.2}]}, fh)
    argv = ["--experiment_name", "exp", "--checkpoint_path", str(tmp_path / "ckpt"), "--ckpt", "last.ckpt", "--dataset", "generic", str(data), "--cameras", str(data / "cameras.json"),
            "--emitter_path", str(bake), "--output_path", str(outp), "--split", "val", "--SPP", "4", "--spp", "2", "--indir_depth", "2", "--crf_basis", "3",
            "--material", "stub_material:material", "--seed", "3", "--metrics", "psnr,ssim"]
    R.main(argv)
    assert "Mean SSIM: " in capsys.readouterr().out
    lines = open(outp / "val" / "rgb" / "metrics.txt").read().splitlines()
    assert lines[0] == "Name, PSNR, SSIM" and len(lines) == 3
    row, mean = lines[1].split(", "), lines[2].split(", ")
    assert row[0] == "00000" and mean[0] == "mean " and len(row) == 3 and len(mean) == 3
    assert row[1:] == mean[1:] and all(len(v.split(".")[1]) == 5 for v in row[1:])
    # the same view through render_view with the CLI's seed
    gt_read = read_image(str(data / "gt.exr"), (H, W))
    rays = view_rays({"kind": "real", "K": f["K"], "c2w": f["c2w"]}, (H, W), torch.device(DEV), ray_diff=True)
    torch.manual_seed(3 * 1000003); torch.cuda.manual_seed(3 * 1000003)
    out = R.render_view(scene, em, StubMaterial(), crf.to(DEV), rays, (H, W), 4, 2, 2, exposure=1.2, gt=gt_read, metrics=("psnr", "ssim"))
    _, m64 = ssim_ref64(gt_read, out["rgb_ldr"].cpu().numpy(), 1.0)
    print(f"metrics.txt SSIM {row[2]}, render_view {out['ssim']:.9f}, ssim_ref64 {m64[0]:.9f}")
    assert isinstance(out["ssim"], float) and -1.0 <= out["ssim"] < 1.0
    assert abs(float(row[2]) - m64[0]) <= 1e-5
    assert abs(out["ssim"] - m64[0]) <= 1e-5 and abs(out["psnr"] - float(row[1])) < 1e-4
    torch.manual_seed(3 * 1000003); torch.cuda.manual_seed(3 * 1000003)
    plain = R.render_view(scene, em, StubMaterial(), crf.to(DEV), rays, (H, W), 4, 2, 2, exposure=1.2, gt=gt_read)
    assert plain["ssim"] is None and plain["psnr"] == out["psnr"]
    with pytest.raises(R.L.IrisError):
        R.render_view(scene, em, StubMaterial(), crf.to(DEV), rays, (H, W), 4, 2, 2, gt=gt_read, metrics=("lpips",))
