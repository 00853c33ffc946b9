"""The video stage's host parts (iris_amd/utils/png.py, utils/cameras.load_trajectory, utils/stage.ffconcat_text, iris_amd/render_video.build_parser) without a
GPU: the PNG container and the host encoder against PIL, the library's MAGMA table against matplotlib's data, the trajectory views of the three dataset
layouts, the video list, the reference's command line."""
import os
import struct
import zlib

import numpy as np
import pytest

from test_stage_setup_cpu import H, W, _real_scene, _scannetpp_scene, _synthetic_scene


def _images():
    rng = np.random.default_rng(3)
    ramp = (np.add.outer(np.arange(6), np.arange(10) * 7) % 256).astype(np.uint8)
    return {"gray_ramp": ramp, "gray_noise": rng.integers(0, 256, (5, 7), dtype=np.uint8), "gray_1ch": ramp[..., None], "gray_flat": np.full((4, 4), 200, np.uint8),
            "rgb_noise": rng.integers(0, 256, (6, 9, 3), dtype=np.uint8), "rgb_ramp": np.stack([ramp, ramp[::-1], 255 - ramp], -1), "rgb_one": np.array([[[1, 2, 3]]], np.uint8)}


def _chunks(data):
    """[(tag, payload)] of a PNG file; every chunk's CRC-32 is checked"""
    from iris_amd.utils.png import SIGNATURE
    assert data[:8] == SIGNATURE
    out, o = [], 8
    while o < len(data):
        (n,), tag = struct.unpack_from(">I", data, o), data[o + 4:o + 8]
        payload = data[o + 8:o + 8 + n]
        assert struct.unpack_from(">I", data, o + 8 + n)[0] == zlib.crc32(tag + payload) & 0xFFFFFFFF, tag
        out.append((tag, payload))
        o += 12 + n
    assert o == len(data)
    return out


def _decode(data):
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im.mode, np.asarray(im)


@pytest.mark.parametrize("name", sorted(_images()))
def test_container_and_host_encoder_round_trip(name):
    pytest.importorskip("PIL")
    from iris_amd.utils import png
    a = _images()[name]
    h, w, c = a.shape[0], a.shape[1], (1 if a.ndim == 2 else a.shape[2])
    filtered = png.sub_filter(a)
    assert len(filtered) == h * (1 + w * c) and filtered[0] == 1
    for data in (png.png_container(w, h, c, zlib.compress(filtered)), png.encode_png_host(a), png.encode_png_host(a, level=9)):
        chunks = _chunks(data)
        assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 0 if c == 1 else 2, 0, 0, 0) and chunks[2][1] == b""
        assert zlib.decompress(chunks[1][1]) == filtered
        mode, pixels = _decode(data)
        assert mode == ("L" if c == 1 else "RGB")
        np.testing.assert_array_equal(pixels, a.reshape(h, w) if c == 1 else a)


def test_sub_filter_is_the_png_filter_type_1():
    """Recon(x) = Filt(x) + Recon(a) mod 256, a = the byte bpp positions to the left (PNG specification, 9.2), written out"""
    from iris_amd.utils.png import sub_filter
    a = _images()["rgb_noise"]
    rows = np.frombuffer(sub_filter(a), np.uint8).reshape(a.shape[0], -1)
    assert (rows[:, 0] == 1).all()
    recon = np.zeros((a.shape[0], a.shape[1] * 3), np.uint8)
    for x in range(recon.shape[1]):
        recon[:, x] = rows[:, 1 + x] + (recon[:, x - 3] if x >= 3 else 0)
    np.testing.assert_array_equal(recon.reshape(a.shape), a)


def test_container_and_encoder_refuse_what_png_cannot_hold():
    from iris_amd.utils import png
    with pytest.raises(ValueError):
        png.png_container(4, 4, 2, b"")
    with pytest.raises(ValueError):
        png.png_container(0, 4, 3, b"")
    with pytest.raises(ValueError):
        png.encode_png_host(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        png.encode_png_host(np.zeros((4, 4, 4), np.uint8))


def test_magma_table_is_matplotlibs():
    cm = pytest.importorskip("matplotlib._cm_listed")
    from iris_amd.utils.png import magma_table
    t = magma_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    np.testing.assert_array_equal(t, np.rint(np.asarray(cm._magma_data, np.float32) * 255).astype(np.uint8))
    scaled = np.asarray(cm._magma_data, np.float64) * 255
    assert np.abs(scaled - np.floor(scaled) - 0.5).min() > 5e-4          # no entry near a rounding tie: the rounding mode does not matter


def test_quantize_host_is_the_references_save_image():
    from iris_amd._lib import IrisError
    from iris_amd.utils.png import magma_table, quantize_host
    rng = np.random.default_rng(0)
    a = (rng.random((5, 7, 3), dtype=np.float32) * 1.4 - 0.2).astype(np.float32)
    want = (np.clip(a, 0.0, 1.0) * 255).astype(np.uint8)[:4, :6]           # render_video.py:38-44
    np.testing.assert_array_equal(quantize_host(a), want)
    e = a * 12
    np.testing.assert_array_equal(quantize_host(e, 10.0), (np.clip(e / np.float32(10.0), 0.0, 1.0) * 255).astype(np.uint8)[:4, :6])
    g = a[..., 0].copy()
    g[0, 0], g[0, 1], g[1, 0] = np.nan, np.inf, -np.inf
    q = quantize_host(g)
    assert q.shape == (4, 6) and q[0, 0] == 0 and q[0, 1] == 255 and q[1, 0] == 0
    np.testing.assert_array_equal(quantize_host(g, magma=True), magma_table()[q])
    u8 = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    np.testing.assert_array_equal(quantize_host(u8), u8[:2, :4])
    with pytest.raises(IrisError):
        quantize_host(a, magma=True)
    with pytest.raises(IrisError):
        quantize_host(np.zeros((1, 7, 3), np.float32))


# ---- trajectory
def _traj(n, rows=3):
    t = np.zeros((n, rows, 4), np.float64)
    for k in range(n):
        a = 0.2 * k
        t[k, :3] = [[np.cos(a), 0, np.sin(a), 0.1 * k + 1 / 3], [0, 1, 0, 0.2], [-np.sin(a), 0, np.cos(a), 0.3]]
        if rows == 4:
            t[k, 3] = [0, 0, 0, 1]
    return t


@pytest.mark.parametrize("res_scale", [1.0, 0.5])
@pytest.mark.parametrize("rows", [3, 4])
def test_load_trajectory_on_the_three_layouts(tmp_path, res_scale, rows):
    from iris_amd.utils import cameras, stage
    syn, real, spp = (str(tmp_path / n) for n in ("syn", "real", "spp"))
    meta = _synthetic_scene(syn)
    _real_scene(real)
    _scannetpp_scene(spp)
    traj = _traj(5, rows)
    np.save(os.path.join(syn, "render_traj.npy"), traj)                     # the scene's folder, not the split's
    np.save(os.path.join(real, "render_traj.npy"), traj)
    np.save(os.path.join(spp, "data", "sc0", "psdf", "render_traj.npy"), traj)
    hw = (int(H * res_scale), int(W * res_scale))
    want_c2w = traj[:, :3].astype(np.float32)

    def check(got, kind, size=hw):
        assert got[0] == size and len(got[1]) == 5
        for v, c in zip(got[1], want_c2w):
            assert v["kind"] == kind and v["c2w"].dtype == np.float32 and v["c2w"].shape == (3, 4) and np.array_equal(v["c2w"], c)

    for split in ("train", "val"):
        got = cameras.load_trajectory("synthetic", syn, "", res_scale, split=split)
        check(got, "synthetic")
        focal = float(0.5 * hw[1] / np.tan(0.5 * meta[split]["camera_angle_x"]))
        assert all(v["focal"] == focal for v in got[1])
        assert got[0] == stage.load_views("synthetic", syn, "", res_scale, split=split)[0]
        got = cameras.load_trajectory("real", real, "", res_scale, split=split)
        check(got, "real")
        first = cameras.load_real(real, res_scale, split=split)[1][0]["K"]
        # (the first TRAIN view of the layout is capture 1, the first validation view capture 0: K_list.txt's focal 6 and 5, scaled)
        assert first[0, 0] == np.float32((6 if split == "train" else 5) * res_scale) and first[2, 2] == 1
        assert all(np.array_equal(v["K"], first) for v in got[1])
    for split in ("train", "test"):
        got = cameras.load_trajectory("scannetpp", spp, "sc0", res_scale, split=split)
        img_hw, views = cameras.load_scannetpp(spp, "sc0", res_scale, split=split)
        check(got, "real", img_hw)
        assert all(np.array_equal(v["K"], views[0]["K"]) for v in got[1])
    full, half = (cameras.load_trajectory("scannetpp", spp, "sc0", s, split="train") for s in (1.0, 0.5))
    assert half[0] == (int(full[0][0] * 0.5), int(full[0][1] * 0.5)) and np.array_equal(half[1][0]["K"][:2], (full[1][0]["K"][:2].astype(np.float64) * 0.5).astype(np.float32))
    # stage.load_trajectory is the same call; the views are what view_rays takes
    a, b = stage.load_trajectory("real", real, "", res_scale, split="val"), cameras.load_trajectory("real", real, "", res_scale, split="val")
    assert a[0] == b[0] and all(np.array_equal(x["c2w"], y["c2w"]) and np.array_equal(x["K"], y["K"]) for x, y in zip(a[1], b[1]))
    assert set(a[1][0]) == {"kind", "K", "c2w"} and set(cameras.load_trajectory("synthetic", syn, "", res_scale)[1][0]) == {"kind", "focal", "c2w"}


def test_a_missing_or_malformed_trajectory_is_refused_with_its_path(tmp_path, monkeypatch):
    import torch
    from iris_amd import render_relight, render_video
    from iris_amd._lib import IrisError
    from iris_amd.utils import cameras, stage
    syn, real, spp = (str(tmp_path / n) for n in ("syn", "real", "spp"))
    _synthetic_scene(syn)
    _real_scene(real)
    _scannetpp_scene(spp)
    for dataset, root, scene, path in (("synthetic", syn, "", os.path.join(syn, "render_traj.npy")), ("real", real, "", os.path.join(real, "render_traj.npy")),
                                       ("scannetpp", spp, "sc0", os.path.join(spp, "data", "sc0", "psdf", "render_traj.npy"))):
        assert cameras.trajectory_path(dataset, root, scene) == path
        with pytest.raises(IrisError) as err:
            cameras.load_trajectory(dataset, root, scene, 1.0)
        assert path in str(err.value)
    np.save(os.path.join(real, "render_traj.npy"), np.zeros((4, 2, 4)))
    with pytest.raises(IrisError, match=r"\(N,3,4\) or \(N,4,4\)"):
        cameras.load_trajectory("real", real, "", 1.0)
    with pytest.raises(IrisError):
        cameras.load_trajectory("generic", real, "", 1.0)
    # both stages meet the missing file before they open a device
    def no_device(*a, **k):
        raise AssertionError("the device was opened before the trajectory was looked for")
    monkeypatch.setattr(stage, "open_device", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    common = ["--experiment_name", "e", "--dataset", "synthetic", syn, "--emitter_path", str(tmp_path), "--output_path", str(tmp_path / "out")]
    with pytest.raises(IrisError, match="render trajectory not found"):
        render_video.main(common)
    with pytest.raises(IrisError, match="render trajectory not found"):
        render_relight.main(common + ["--mode", "traj", "--light_cfg", "none.yaml"])


# ---- the video list
def test_ffconcat_lists_the_frames_forward_then_reversed(tmp_path):
    from iris_amd import render_video
    from iris_amd.utils import stage
    frames = ["rgb/%05d_rgb_full.png" % i for i in range(4)]
    text = stage.ffconcat_text(frames, 30)
    lines = text.splitlines()
    assert lines[0] == "ffconcat version 1.0" and text.endswith("\n")
    files = [l for l in lines[1:] if l.startswith("file ")]
    durations = [l for l in lines[1:] if l.startswith("duration ")]
    assert len(files) == len(durations) == 8 and len(lines) == 17
    assert files == ["file '%s'" % f for f in frames + frames[::-1]]
    assert all(abs(float(d.split()[1]) - 1 / 30) < 1e-8 for d in durations)
    assert lines[1::2] == files and lines[2::2] == durations
    # the stage's eight lists name the stage's own frame files, relative to the list
    out = tmp_path / "video"
    lists = render_video.write_lists(str(out), 3)
    assert [os.path.basename(p) for p in lists] == [n + ".ffconcat" for n in ("rgb_full", "kd", "a_prime", "roughness", "roughness_color", "metallic", "metallic_color", "emission")]
    for k, p in enumerate(lists):
        named = [l[6:-1] for l in open(p).read().splitlines() if l.startswith("file ")]
        want = [os.path.relpath(render_video.frame_paths(str(out), i)[k], str(out)) for i in range(3)]
        assert named == want + want[::-1]
    assert render_video.frame_paths("o", 7) == [os.path.join("o", *p) for p in (("rgb", "00007_rgb_full.png"), ("diffuse", "00007_kd.png"), ("a_prime", "00007_a_prime.png"),
                                                                                 ("roughness", "00007_roughness.png"), ("roughness", "00007_roughness_color.png"),
                                                                                 ("metallic", "00007_metallic.png"), ("metallic", "00007_metallic_color.png"),
                                                                                 ("emission", "00007_emission.png"))]


# ---- the parser
def test_parser_accepts_the_references_command_line():
    """scripts/fipt/kitchen/render.sh:30-37 with its variables expanded"""
    from iris_amd.render_video import build_parser
    a = build_parser().parse_args(["--experiment_name", "fipt_syn_kitchen", "--device", "0", "--ckpt", "last_1.ckpt", "--dataset", "synthetic",
                                   "/hdd/datasets/fipt/indoor_synthetic/kitchen", "--emitter_path", "checkpoints/fipt_syn_kitchen/bake", "--output_path",
                                   "outputs/fipt_syn_kitchen/video", "--split", "val", "--ldr_img_dir", "Image", "--SPP", "256", "--spp", "16", "--crf_basis", "3"])
    assert a.dataset == ["synthetic", "/hdd/datasets/fipt/indoor_synthetic/kitchen"] and a.SPP == 256 and a.spp == 16 and a.crf_basis == 3 and a.split == "val"
    assert a.ckpt == "last_1.ckpt" and a.device == 0 and a.light_type == "slf" and a.ldr_img_dir == "Image"
    # the additions default to the reference's behaviour; the encoder's default is the device
    assert a.material is None and a.emor_path is None and a.denoise == "atrous" and a.seed == 0 and a.max_views is None and a.png_encoder == "device"
    b = build_parser().parse_args(["--experiment_name", "e", "--emitter_path", "b", "--png_encoder", "host", "--batch_size", "4", "--has_part", "1", "--val_step", "2"])
    assert b.png_encoder == "host" and b.batch_size == 4
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--experiment_name", "e", "--emitter_path", "b", "--png_encoder", "pil"])
