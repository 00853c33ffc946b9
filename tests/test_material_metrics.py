"""The material metrics on the GPU (iris_amd/csrc/iris_matmetrics.h, iris_amd/utils/material_metrics.py, python -m iris_amd.utils.metric_brdf / metric_crf,
render --material_metrics) against the contract's exact restatement, tests/material_metrics_ref.py (a): the seven integer sums bit for bit, S_emit within a
2-half-ulp logarithm and the summation tree's roundings.

Shapes (N, H, W): (1,1,1); (3,5,7) -- an odd pixel count, so views 1 and 2 of the 3-byte-pixel stacks start at unaligned addresses --; (2,16,67) -- ragged
vector tails --; (2,64,129) -- 17 chunks of 512 pixels per view, the last one partial."""
import json
import math
import os

import numpy as np
import pytest
import torch

import material_metrics_ref as R

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (3, 5, 7), (2, 16, 67), (2, 64, 129))
DEV = "cuda"


def _dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}


def _host(res):
    sums = res["sums"].cpu().numpy()
    return sums[:, :7], np.ascontiguousarray(sums[:, 7]).view(np.float64), sums


@pytest.fixture(scope="module")
def cases():
    """per shape: the inputs and (a) of the uint8, the float32 and a mixed estimate, computed once"""
    out = {}
    for si, (N, H, W) in enumerate(SHAPES):
        gt, u8, f32 = R.make_inputs(N, H, W, 40 + si)
        mix = {"emit": u8["emit"], "albedo": f32["albedo"], "kd": u8["kd"], "rough": f32["rough"]}
        ests = {"u8": u8, "f32": f32, "mix": mix}
        out[(N, H, W)] = (gt, ests, {k: R.exact(gt, e) for k, e in ests.items()})
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_are_exact_and_reproducible(cases, shape):
    from iris_amd.utils.material_metrics import material_metrics
    N, H, W = shape
    gt, ests, refs = cases[shape]
    g = _dev(gt)
    for kind, est in ests.items():
        e = _dev(est)
        res = material_metrics(g, e)
        ints, s_emit, raw = _host(res)
        ref = refs[kind]
        assert res["sums"].dtype == torch.int64 and tuple(res["sums"].shape) == (N, 8)
        assert (ints == ref["sums"]).all(), (kind, ints.tolist(), ref["sums"].tolist())
        assert (material_metrics(g, e)["sums"].cpu().numpy() == raw).all(), kind             # bit for bit, S_emit's word included
        for n in range(N):
            tol = R.s_emit_tolerance(ref, n, H, W, c=2.0)
            err = abs(s_emit[n] - ref["s_emit"][n])
            print(f"{shape} {kind} view {n}: S_emit {s_emit[n]:.17g}, |got - ref| = {err:.3g}, bound {tol:.3g}, ratio {err / tol if tol else 0.0:.3g}")
            assert np.isfinite(s_emit[n]) and err <= tol
            # a view alone gives the view's words of the stack (its maps then start at other alignments)
            one = material_metrics({k: v[n] for k, v in g.items()}, {k: v[n] for k, v in e.items()})["sums"].cpu().numpy()
            assert (one[0] == raw[n]).all(), (kind, n)
        pv = R.per_view(ref["sums"], s_emit, H, W)
        for key in ("mse_albedo", "mse_kd", "mse_roughness", "emit_iou", "emit_log_mse"):
            got = res[key].cpu().numpy()
            assert got.dtype == np.float64 and np.array_equal(got, pv[key], equal_nan=True), key
        assert (res["s_emit"].cpu().numpy() == s_emit).all()


def test_a_non_finite_emission_term_marks_its_view_only(cases):
    from iris_amd.utils.material_metrics import material_metrics
    shape = (3, 5, 7)
    gt, ests, refs = cases[shape]
    clean = _host(material_metrics(_dev(gt), _dev(ests["u8"])))
    for view, value, where in ((1, float("nan"), "est"), (2, -1.0, "est"), (0, float("nan"), "gt")):
        g, e = {k: v.copy() for k, v in gt.items()}, {k: v.copy() for k, v in ests["u8"].items()}
        (e if where == "est" else g)["emit"][view, 2, 3, 1] = value
        ints, s_emit, _ = _host(material_metrics(_dev(g), _dev(e)))
        want = R.exact(g, e)
        assert (ints == want["sums"]).all()                             # (a NaN changes its pixel's mask, nothing else)
        assert not np.isfinite(s_emit[view]), (view, value, s_emit)
        others = [n for n in range(3) if n != view]
        assert (ints[others] == clean[0][others]).all() and (s_emit[others] == clean[1][others]).all()


def _render_maps(N, H, W, seed):
    """float32 maps as render_view returns them, with values outside [0, 1] and on both sides of every code's edge"""
    rng = np.random.default_rng(seed)
    k = (np.arange(256) / 255.0).astype(np.float32)
    edge = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), np.float32([-0.25, 1.5, -0.0, 3.0])])

    def m(*shape):
        a = rng.random(shape).astype(np.float32)
        flat = a.reshape(-1)
        n = min(edge.size, flat.size // 2)
        flat[rng.choice(flat.size, n, replace=False)] = rng.permutation(edge)[:n]
        return a
    emission = np.where(rng.random((N, H, W, 1)) < 0.3, rng.random((N, H, W, 3)) * 4, 0).astype(np.float32)
    return {"emission": emission, "a_prime": m(N, H, W, 3), "kd": m(N, H, W, 3), "roughness": m(N, H, W), "metallic": m(N, H, W), "slf": m(N, H, W, 3),
            "rgb_full": m(N, H, W, 3), "rgb_ldr": None}


def test_files_and_tensors_give_the_same_bits(tmp_path):
    """write_view's PNGs and EXR read back (the uint8 path) against the float32 maps they were written from, and render's material_metrics_view"""
    pytest.importorskip("PIL")
    from iris_amd import render as Rn
    from iris_amd.utils import material_metrics as M
    N, H, W = 2, 5, 7
    gt, _, _ = R.make_inputs(N, H, W, 77)
    maps = _render_maps(N, H, W, 78)
    R.write_gt_tree(str(tmp_path / "gt"), gt)
    on_files, on_tensors = [], []
    for i in range(N):
        out = {k: (None if v is None else torch.from_numpy(v[i]).to(DEV)) for k, v in maps.items()}
        Rn.write_view(str(tmp_path / "out"), "train", i, out, "zip")
        on_tensors.append(Rn.material_metrics_view(str(tmp_path / "gt"), i, out, (H, W))["sums"].cpu().numpy())
        on_files.append(M.load_method_view(str(tmp_path / "out" / "train"), i))
        assert on_files[-1]["albedo"].dtype == np.uint8 and on_files[-1]["rough"].shape == (H, W)
    files = M.material_metrics(_dev(gt), M.upload(on_files, DEV))["sums"].cpu().numpy()
    assert (files == np.concatenate(on_tensors)).all()
    est = {"emit": maps["emission"], "albedo": maps["a_prime"], "kd": maps["kd"], "rough": maps["roughness"]}
    stack = M.material_metrics(_dev(gt), _dev(est))["sums"].cpu().numpy()
    assert (stack == files).all() and (files[:, :7] == R.exact(gt, est)["sums"]).all()


def test_metric_brdf_command_line(tmp_path, capsys):
    pytest.importorskip("PIL")
    from iris_amd.utils import metric_brdf as B
    N, H, W = 3, 6, 8
    gt, u8, _ = R.make_inputs(N, H, W, 91, emitter_views=(True, False, True))
    g, m = str(tmp_path / "gt"), str(tmp_path / "m")
    R.write_gt_tree(g, gt)
    R.write_method_tree(m, u8)
    ref = R.exact(gt, u8)
    docs = {}
    for batch in (2, 8):
        capsys.readouterr()
        assert B.cli(["--gt", g, "--method", m, "--batch", str(batch), "--json", str(tmp_path / f"b{batch}.json")]) == 0
        lines = capsys.readouterr().out.splitlines()
        docs[batch] = json.loads((tmp_path / f"b{batch}.json").read_text())
        assert [l[:13] for l in lines] == ["kd:          ", "albedo:      ", "roughness:   ", "emit_iou:    ", "emit_log_mse:"]
        assert [float(l[14:]) for l in lines] == [docs[batch]["summary"][k] for k in ("kd", "albedo", "roughness", "emit_iou", "emit_log_mse")]
    assert docs[2] == docs[8]
    doc = docs[8]
    assert doc["views"] == N and [row[:7] for row in doc["sums"]] == ref["sums"].tolist()
    s_emit = np.array([row[7] for row in doc["sums"]])
    tol = np.array([R.s_emit_tolerance(ref, n, H, W) for n in range(N)])
    assert (np.abs(s_emit - ref["s_emit"]) <= tol).all()
    want = R.summary(R.per_view(ref["sums"], ref["s_emit"], H, W))
    for k in ("kd", "albedo", "roughness", "emit_iou"):
        assert doc["summary"][k] == want[k], k
    assert abs(doc["summary"]["emit_log_mse"] - want["emit_log_mse"]) <= (tol[0] + tol[2]) / 2 / (3 * H * W) + 1e-16 * want["emit_log_mse"]
    assert doc["per_view"]["emit_iou"][1] is None and doc["per_view"]["emit_log_mse"][1] is None
    capsys.readouterr()
    assert B.cli(["--gt", g, "--method", m, "--max_views", "1"]) == 0
    one = R.summary(R.per_view(ref["sums"][:1], s_emit[:1], H, W))
    assert [float(l[14:]) for l in capsys.readouterr().out.splitlines()] == [one[k] for k in ("kd", "albedo", "roughness", "emit_iou", "emit_log_mse")]


def test_metric_crf_command_line(tmp_path, capsys):
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils import metric_crf as Cm
    from iris_amd.utils import stage
    rng = np.random.default_rng(5)
    x = np.linspace(0, 1, 1024)
    model = EmorCRF.from_arrays(x ** 0.6, np.stack([np.sin(np.pi * (j + 1) * x) * 0.05 for j in range(3)]))
    with torch.no_grad():
        model.weight.copy_(torch.from_numpy(rng.normal(size=(3, 3)).astype(np.float32)))
    pred = model.get_crf().detach().numpy()
    assert pred.shape == (3, 1024)
    crf_gt = pred + np.float32(0.0123) * np.where(np.arange(1024) % 2, -1, 1)[None].astype(np.float32)        # a known shift: L2 = 0.0123 sqrt(3072)
    np.save(tmp_path / "crf.npy", crf_gt)
    stage.write_checkpoint(str(tmp_path / "last_1.ckpt"), {}, model.state_dict(), {}, epoch=1, global_step=1, hyper_parameters={})
    capsys.readouterr()
    assert Cm.cli(["--crf_gt", str(tmp_path / "crf.npy"), "--ckpt", str(tmp_path / "last_1.ckpt"), "--dir_save", str(tmp_path / "save")]) == 0
    out = capsys.readouterr().out.strip()
    saved = np.load(tmp_path / "save" / "crf.npy")                      # the curves the command evaluated on the device
    assert saved.shape == (3, 1024) and np.abs(saved - pred).max() <= 1e-6
    want = float(np.linalg.norm(crf_gt - saved))
    assert abs(want - 0.0123 * math.sqrt(3072)) < 1e-5                   # (float32 rounding of pred + shift: <= 6e-8 per value)
    assert out == "L2: {:.5f}".format(want)


def test_refusals():
    from iris_amd import _lib as L
    from iris_amd.utils.material_metrics import material_metrics
    gt, u8, _ = R.make_inputs(2, 4, 5, 3)
    g, e = _dev(gt), _dev(u8)
    with pytest.raises(L.IrisError, match="HIP device"):
        material_metrics({k: v.cpu() for k, v in g.items()}, e)
    with pytest.raises(L.IrisError, match="HIP device"):
        material_metrics(g, dict(e, kd=e["kd"].cpu()))
    with pytest.raises(L.IrisError):
        material_metrics(g, dict(e, albedo=e["albedo"][:, :, :4]))                       # another width
    with pytest.raises(L.IrisError):
        material_metrics(g, dict(e, rough=e["rough"][:1]))                               # another view count
    with pytest.raises(L.IrisError):
        material_metrics(dict(g, rough=g["rough"][..., None].expand(-1, -1, -1, 3)), e)  # three channels where one is expected
    with pytest.raises(L.IrisError, match="dtype"):
        material_metrics(g, dict(e, emit=e["emit"].double()))
    with pytest.raises(L.IrisError, match="dtype"):
        material_metrics(dict(g, albedo=e["albedo"]), e)                                 # the ground truth is float32 only
    with pytest.raises(L.IrisError, match="requires grad"):
        material_metrics(g, dict(e, emit=e["emit"].clone().requires_grad_()))
    # the size guard, by the workspace query alone: H W <= 2^30 and N ceil(H W / 512) < 2^31
    lib = L.lib()
    q = lib.iris_material_metrics_workspace_bytes
    assert q(2, 64, 129) == 2 * 17 * 8 * 8 and q(1, 1, 1) == 64
    assert q(1, 32768, 32768) == (2 ** 30 // 512) * 64 and q(1, 32768, 32769) == 0 and q(1, 2 ** 31 - 1, 2) == 0
    assert q(1023, 32768, 32768) == 1023 * (2 ** 21) * 64 and q(1024, 32768, 32768) == 0
    assert q(0, 4, 4) == 0 and q(1, 0, 4) == 0 and q(1, 4, -1) == 0
    sums = torch.zeros(2, 8, dtype=torch.int64, device=DEV)
    a = L.MaterialMetricsArgs(emit_gt=L.ptr(g["emit"]), albedo_gt=L.ptr(g["albedo"]), kd_gt=L.ptr(g["kd"]), rough_gt=L.ptr(g["rough"]), emit=L.ptr(e["emit"]),
                              albedo=L.ptr(e["albedo"]), kd=L.ptr(e["kd"]), rough=L.ptr(e["rough"]), sums=L.ptr(sums), workspace=None, workspace_bytes=0,
                              albedo_is_u8=1, kd_is_u8=1, rough_is_u8=1, N=2, H=4, W=5)
    import ctypes as C
    with pytest.raises(L.IrisError, match="workspace"):
        L.check(lib.iris_material_metrics(C.byref(a), L.stream()))
    a.N, a.H, a.W = 1, 32768, 32769
    with pytest.raises(L.IrisError, match="unsupported size"):
        L.check(lib.iris_material_metrics(C.byref(a), L.stream()))


def test_render_scores_what_metric_brdf_reads_from_its_files(tmp_path, capsys):
    """python -m iris_amd.render --material_metrics GT_DIR on tests/test_render.py's room (24 x 16, SPP 4, spp 2, stub material), then
    python -m iris_amd.utils.metric_brdf on the files that run wrote: the same sums, S_emit's bits included, and the same five numbers"""
    pytest.importorskip("PIL")
    from iris_amd import render as Rn
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils import metric_brdf as B
    from test_render import setup, write_emitter_files
    f, _, _ = setup()
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
    torch.save({"state_dict": {"model_crf." + k: v for k, v in crf.state_dict().items()}}, ckpt_dir / "last.ckpt")
    with open(data / "cameras.json", "w") as fh:
        json.dump({"img_hw": [H, W], "views": [{"K": f["K"].tolist(), "c2w": f["c2w"].tolist()}]}, fh)
    gt, _, _ = R.make_inputs(1, H, W, 17)
    R.write_gt_tree(str(tmp_path / "gt"), gt)
    argv = ["--experiment_name", "exp", "--checkpoint_path", str(tmp_path / "ckpt"), "--ckpt", "last.ckpt", "--dataset", "generic", str(data), "--cameras", str(data / "cameras.json"),
            "--emitter_path", str(bake), "--output_path", str(outp), "--split", "train", "--SPP", "4", "--spp", "2", "--indir_depth", "2", "--crf_basis", "3",
            "--material", "stub_material:material", "--seed", "3", "--material_metrics", str(tmp_path / "gt")]
    capsys.readouterr()
    Rn.main(argv)
    printed = [l for l in capsys.readouterr().out.splitlines() if l[:13] in ("kd:          ", "albedo:      ", "roughness:   ", "emit_iou:    ", "emit_log_mse:")]
    assert len(printed) == 5
    live = json.loads((outp / "train" / "material_metrics.json").read_text())
    assert B.cli(["--gt", str(tmp_path / "gt"), "--method", str(outp / "train"), "--json", str(tmp_path / "files.json")]) == 0
    assert capsys.readouterr().out.splitlines() == printed
    files = json.loads((tmp_path / "files.json").read_text())
    assert live["views"] == 1 and live["sums"] == files["sums"] and live["per_view"] == files["per_view"] and live["summary"] == files["summary"]
    assert live["sums"][0][0] > 0 and live["sums"][0][2] > 0            # (the room's maps are not the random ground truth)
