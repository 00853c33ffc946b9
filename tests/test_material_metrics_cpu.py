"""The material metrics without a GPU: the contract's exact restatement (tests/material_metrics_ref.py (a)) against the reference's float32 formulas taken
literally ((b)), hand-worked cases, the host side of iris_amd/utils/material_metrics.py (summarize, the table, the file readers) and the parsers and error
paths of python -m iris_amd.utils.metric_brdf / metric_crf and of render --material_metrics."""
import json
import os

import numpy as np
import pytest
import torch

import material_metrics_ref as R

SHAPES = ((1, 1, 1), (3, 5, 7), (2, 16, 67), (2, 64, 129))
U = 2.0 ** -24
# (a) against (b), measured on the CPU over the inputs of test_exact_contract_is_the_references_float32_formulas (4 shapes x 6 seeds):
#   the MSEs: worst |b - a| / (a 2^-24) = 3.30 (float32 rounding of x / 255, of the squares and of numpy's pairwise mean)  -> tolerance 4 x 3.30 = 13.2
#   the emission log-MSE: worst |b - a| / log_mse_f32_scale = 0.188                                                        -> tolerance 4 x 0.188 = 0.754
MSE_TOL_ULPS = 13.2
LOG_TOL_SCALE = 0.754


def _view(d, n):
    return {k: v[n] for k, v in d.items()}


def test_exact_contract_is_the_references_float32_formulas():
    """51 / 255 and 255 / 255 ARE float32 0.2 and 1 (what makes the reference's clamps and its == 1 integer tests), then (a) against (b) view by view."""
    assert np.float32(51) / np.float32(255) == np.float32(0.2) and np.float32(255) / np.float32(255) == np.float32(1)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    assert ((k >= np.float32(0.2)) == (np.arange(256) >= 51)).all() and ((k == 1) == (np.arange(256) == 255)).all()
    worst_mse = worst_log = 0.0
    views = emitters = 0
    for si, (N, H, W) in enumerate(SHAPES):
        for rep in range(6):
            gt, u8, _ = R.make_inputs(N, H, W, 100 * rep + si, colour_nan=False)
            ex = R.exact(gt, u8)
            pv = R.per_view(ex["sums"], ex["s_emit"], H, W)
            for n in range(N):
                lit = R.literal(_view(gt, n), _view(u8, n))
                views += 1
                for key in ("mse_albedo", "mse_kd", "mse_roughness"):
                    a, b = pv[key][n], float(lit[key])
                    if a == 0.0:
                        assert b == 0.0
                        continue
                    worst_mse = max(worst_mse, abs(b - a) / (a * U))
                if lit["emit_iou"] is None:
                    assert ex["sums"][n, 3] == 0 and np.isnan(pv["emit_iou"][n]) and np.isnan(pv["emit_log_mse"][n])
                    continue
                emitters += 1
                assert lit["emit_iou"] == pv["emit_iou"][n]
                worst_log = max(worst_log, abs(float(lit["emit_log_mse"]) - pv["emit_log_mse"][n]) / R.log_mse_f32_scale(gt["emit"][n], u8["emit"][n]))
    print(f"(a) against (b) over {views} views ({emitters} with an emitter): MSE worst {worst_mse:.3g} x 2^-24 relative, log-MSE worst {worst_log:.3g} x scale")
    assert views == 48 and emitters >= 30
    assert worst_mse <= MSE_TOL_ULPS and worst_log <= LOG_TOL_SCALE


def _one_pixel():
    gt = {"emit": np.zeros((1, 1, 3), np.float32), "albedo": np.array([[[0.5, 0.2, 1.0]]], np.float32), "kd": np.array([[[0.1, 2.0, -1.0]]], np.float32),
          "rough": np.array([[1.0]], np.float32)}
    est = {"emit": np.array([[[0.0, 0.0, np.e - 1.0]]], np.float32), "albedo": np.array([[[130, 50, 250]]], np.uint8), "kd": np.array([[[20, 250, 3]]], np.uint8),
           "rough": np.array([[40]], np.uint8)}
    return gt, est


def test_one_pixel_view_by_hand():
    gt, est = _one_pixel()
    ex = R.exact(gt, est)
    # albedo codes 127, 51, 255 against 130, 50, 250; roughness 255 (diffuse) against clamp(40) = 51; kd codes 25, 255, 0 against 20, 250, 3
    assert ex["sums"].tolist() == [[9 + 1 + 25, 25 + 25 + 9, (255 - 51) ** 2, 0, 1, 0, 1]]
    assert abs(ex["s_emit"][0] - 1.0) < 1e-6                            # log(e) - log(1), once
    pv = R.per_view(ex["sums"], ex["s_emit"], 1, 1)
    assert pv["mse_albedo"][0] == 35 / (65025 * 3) and pv["mse_roughness"][0] == 204 ** 2 / 65025 and np.isnan(pv["emit_iou"][0]) and np.isnan(pv["emit_log_mse"][0])
    gt["rough"][0, 0] = np.nextafter(np.float32(1), np.float32(0))      # code 254: not diffuse, kd drops out
    assert R.exact(gt, est)["sums"][0, :3].tolist() == [35, 0, (254 - 51) ** 2]


def test_views_without_an_emitter_and_all_emitter_views():
    gt, u8, f32 = R.make_inputs(3, 6, 8, 7, emitter_views=(True, False, True))
    gt["emit"][2] = np.float32(0.5)                                     # view 2: every pixel an emitter
    for est in (u8, f32):
        ex = R.exact(gt, est)
        pv = R.per_view(ex["sums"], ex["s_emit"], 6, 8)
        assert ex["sums"][1, 3] == 0 and ex["sums"][1, 5] == 0 and np.isnan(pv["emit_iou"][1]) and np.isnan(pv["emit_log_mse"][1])
        assert ex["sums"][2, 3] == 48 and ex["sums"][2, :3].tolist() == [0, 0, 0]
        assert ex["sums"][0, 3] > 0 and ex["sums"][0, 0] > 0 and ex["sums"][0, 1] > 0 and ex["sums"][0, 2] > 0
        s = R.summary(pv)
        assert s["emit_iou"] == np.mean([pv["emit_iou"][0], pv["emit_iou"][2]]) and s["emit_log_mse"] == np.mean([pv["emit_log_mse"][0], pv["emit_log_mse"][2]])
        assert s["albedo"] == np.mean([-10 * np.log10(pv["mse_albedo"][0]), -10 * np.log10(pv["mse_albedo"][1]), 100.0])


def test_summarize_by_hand_and_the_table():
    from iris_amd.utils import material_metrics as M
    nan = float("nan")
    s = M.summarize({"mse_kd": [1e-2, 1e-4, 0.0], "mse_albedo": torch.tensor([1e-1, 1e-3, 1e-5], dtype=torch.float64), "mse_roughness": np.array([1.0, 1e-12, 1e-2]),
                     "emit_iou": [0.5, nan, 1.0], "emit_log_mse": [2.0, nan, 4.0]})
    want = {"kd": (20 + 40 + 100) / 3, "albedo": (10 + 30 + 50) / 3, "roughness": (0 + 100 + 20) / 3, "emit_iou": 0.75, "emit_log_mse": 3.0}
    assert set(s) == set(want) and all(abs(s[k] - want[k]) < 1e-12 for k in want), s
    none = M.summarize({"mse_kd": [1.0], "mse_albedo": [1.0], "mse_roughness": [1.0], "emit_iou": [nan], "emit_log_mse": [nan]})
    assert none["kd"] == 0.0 and np.isnan(none["emit_iou"]) and np.isnan(none["emit_log_mse"])
    assert M.format_summary(want).splitlines() == ["kd:           " + str(want["kd"]), "albedo:       30.0", "roughness:    40.0", "emit_iou:     0.75", "emit_log_mse: 3.0"]
    # the table: batches of raw sums (as material_metrics returns them: int64, S_emit's bits in word 7) -> the contract's per-view values and summary
    gt, u8, _ = R.make_inputs(3, 6, 8, 11, emitter_views=(True, False, True))
    ex = R.exact(gt, u8)
    raw = np.concatenate([ex["sums"], ex["s_emit"].view(np.int64)[:, None]], 1)
    table = M.Table((6, 8))
    table.add({"sums": torch.from_numpy(raw[:2])})
    table.add({"sums": torch.from_numpy(raw[2:])})
    summary, doc = table.finish()
    pv = R.per_view(ex["sums"], ex["s_emit"], 6, 8)
    assert summary == R.summary(pv)
    assert doc["views"] == 3 and doc["img_hw"] == [6, 8] and [row[:7] for row in doc["sums"]] == ex["sums"].tolist() and [row[7] for row in doc["sums"]] == ex["s_emit"].tolist()
    assert doc["per_view"]["emit_iou"][1] is None and doc["per_view"]["mse_kd"] == pv["mse_kd"].tolist()
    assert json.loads(json.dumps(doc)) == doc and doc["summary"] == summary


def test_cpu_tensors_and_bad_inputs_raise():
    from iris_amd import _lib as L
    from iris_amd.utils.material_metrics import material_metrics
    gt, u8, _ = R.make_inputs(1, 4, 5, 3)
    with pytest.raises(L.IrisError, match="HIP device"):
        material_metrics({k: torch.from_numpy(v) for k, v in gt.items()}, {k: torch.from_numpy(v) for k, v in u8.items()})
    with pytest.raises(L.IrisError, match="no 'rough'"):
        material_metrics({k: torch.from_numpy(v) for k, v in gt.items() if k != "rough"}, {})
    with pytest.raises(L.IrisError, match="dict"):
        material_metrics(None, None)


# ---- the files and the command lines
def test_readers_return_the_files_values(tmp_path):
    pytest.importorskip("PIL")
    from iris_amd import _lib as L
    from iris_amd.utils import material_metrics as M
    gt, u8, _ = R.make_inputs(2, 4, 6, 5)
    R.write_gt_tree(str(tmp_path / "gt"), gt)
    R.write_method_tree(str(tmp_path / "m"), u8)
    assert M.count_views(str(tmp_path / "gt")) == 2
    for i in range(2):
        g, e = M.load_gt_view(str(tmp_path / "gt"), i), M.load_method_view(str(tmp_path / "m"), i)
        for k in R.KEYS:                                                 # bit for bit (NaN included), the B channel for both roughness files
            assert g[k].dtype == np.float32 and g[k].tobytes() == gt[k][i].tobytes(), k
            assert e[k].dtype == u8[k].dtype and e[k].tobytes() == u8[k][i].tobytes(), k
    up = M.upload([M.load_method_view(str(tmp_path / "m"), i) for i in range(2)], "cpu")
    assert up["albedo"].dtype == torch.uint8 and tuple(up["albedo"].shape) == (2, 4, 6, 3) and tuple(up["rough"].shape) == (2, 4, 6)
    with pytest.raises(L.IrisError, match="002_0001.exr"):
        M.load_gt_view(str(tmp_path / "gt"), 2)
    # a compression read_exr does not decode is refused by name
    p = tmp_path / "gt" / "Emit" / "000_0001.exr"
    raw = p.read_bytes()
    key = b"compression\0compression\0\x01\0\0\0"
    at = raw.index(key) + len(key)
    p.write_bytes(raw[:at] + b"\x04" + raw[at + 1:])                    # PIZ
    with pytest.raises(L.IrisError, match="Emit.000_0001.exr.*compression 4"):
        M.load_gt_view(str(tmp_path / "gt"), 0)


def _status(cli, argv, capsys):
    capsys.readouterr()
    rc = cli(argv)
    return rc, capsys.readouterr().err


def test_metric_brdf_parser_and_error_paths(tmp_path, capsys):
    pytest.importorskip("PIL")
    from iris_amd.utils import metric_brdf as B
    args = B.build_parser().parse_args(["--gt", "g", "--method", "m"])
    assert (args.gt, args.method, args.device, args.max_views, args.batch, args.json) == ("g", "m", 0, None, 8, None)
    args = B.build_parser().parse_args(["--gt", "g", "--method", "m", "--batch", "2", "--max_views", "3", "--json", "o.json", "--device", "1"])
    assert (args.device, args.max_views, args.batch, args.json) == (1, 3, 2, "o.json")
    with pytest.raises(SystemExit):
        B.build_parser().parse_args(["--gt", "g"])
    gt, u8, _ = R.make_inputs(2, 4, 6, 5)
    g, m = str(tmp_path / "gt"), str(tmp_path / "m")
    rc, err = _status(B.cli, ["--gt", g, "--method", m], capsys)
    assert rc == 2 and err.startswith("metric_brdf: ") and "Image" in err and len(err.splitlines()) == 1
    R.write_gt_tree(g, gt, n_images=0)
    rc, err = _status(B.cli, ["--gt", g, "--method", m], capsys)
    assert rc == 2 and "no view" in err                                  # a view count of 0
    R.write_gt_tree(g, gt)
    rc, err = _status(B.cli, ["--gt", g, "--method", m, "--max_views", "0"], capsys)
    assert rc == 2 and "no view" in err
    rc, err = _status(B.cli, ["--gt", g, "--method", m], capsys)
    assert rc == 2 and m in err                                          # no method folder
    R.write_method_tree(m, u8)
    os.remove(os.path.join(m, "diffuse", "00000_kd.png"))
    rc, err = _status(B.cli, ["--gt", g, "--method", m], capsys)
    assert rc == 2 and "00000_kd.png" in err and len(err.splitlines()) == 1
    R.write_method_tree(m, {k: np.ascontiguousarray(v[:, :, :5]) for k, v in u8.items()})            # 4 x 5 against 4 x 6
    rc, err = _status(B.cli, ["--gt", g, "--method", m], capsys)
    assert rc == 2 and "view 0" in err and "4 x 5" in err and "4 x 6" in err
    rc, err = _status(B.cli, ["--gt", g, "--method", m, "--batch", "0"], capsys)
    assert rc == 2 and "--batch" in err


def test_metric_crf_parser_and_error_paths(tmp_path, capsys):
    from iris_amd import _lib as L
    from iris_amd.utils import metric_crf as Cm
    from iris_amd.utils import stage
    args = Cm.build_parser().parse_args(["--crf_gt", "c.npy", "--ckpt", "k.ckpt"])
    assert (args.crf_gt, args.ckpt, args.crf_basis, args.emor_path, args.dir_save, args.device) == ("c.npy", "k.ckpt", 3, None, None, 0)
    with pytest.raises(SystemExit):
        Cm.build_parser().parse_args(["--ckpt", "k.ckpt"])
    a = np.linspace(0, 1, 3 * 1024).reshape(3, 1024)
    assert abs(Cm.crf_l2(a, a + 0.01) - 0.01 * np.sqrt(3072)) < 1e-12
    with pytest.raises(L.IrisError):
        Cm.crf_l2(a, a[:, :512])
    crf, ckpt = str(tmp_path / "crf.npy"), str(tmp_path / "last_1.ckpt")
    rc, err = _status(Cm.cli, ["--crf_gt", crf, "--ckpt", ckpt], capsys)
    assert rc == 2 and err.startswith("metric_crf: ") and "crf.npy" in err
    np.save(crf, a)
    rc, err = _status(Cm.cli, ["--crf_gt", crf, "--ckpt", ckpt], capsys)
    assert rc == 2 and "last_1.ckpt" in err
    stage.write_checkpoint(ckpt, {}, {}, {}, epoch=1, global_step=1, hyper_parameters={})
    rc, err = _status(Cm.cli, ["--crf_gt", crf, "--ckpt", ckpt], capsys)
    assert rc == 2 and "model_crf" in err


def test_render_option_is_in_the_cli_parser_only(tmp_path, capsys):
    from iris_amd import render as Rn
    from iris_amd.utils import stage
    base = ["--experiment_name", "e", "--emitter_path", "p"]
    assert Rn.build_cli_parser().parse_args(base).material_metrics is None
    assert Rn.build_cli_parser().parse_args(base + ["--material_metrics", "gt/train"]).material_metrics == "gt/train"
    with pytest.raises(SystemExit):
        Rn.build_parser().parse_args(base + ["--material_metrics", "gt/train"])
    capsys.readouterr()
    rc = stage.exit_status("render", Rn.main, base + ["--material_metrics", str(tmp_path / "nowhere")])
    assert rc == 2 and "nowhere" in capsys.readouterr().err
