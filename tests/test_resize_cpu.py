"""The 8-bit resize contract of the scannetpp layout's --res_scale without a GPU: tests/resize_ref.py (the contract in numpy) on hand cases, against exact
bilinear interpolation and against PIL's NEAREST; the library's host tables against it; and the layout's setup on a scannetpp tree written here.
tests/test_resize.py holds the device kernel to resize_ref byte for byte."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

import resize_ref
from test_stage_setup_cpu import _scannetpp_scene

# (source, target): exact 2; general both ways; one axis exactly 2 and the other not (the general path); PIL's accumulated-addition case; upscale; same size;
# a one-pixel source; a one-pixel target; a wide row whose rows start misaligned
SIZES = [((12, 16), (6, 8)), ((13, 17), (6, 8)), ((11, 16), (5, 8)), ((24, 40), (9, 15)), ((7, 5), (14, 10)), ((9, 9), (9, 9)), ((1, 1), (3, 3)), ((2, 3), (1, 1)),
         ((20, 70), (9, 67))]
SIZE_IDS = ["%dx%d-%dx%d" % (*s, *t) for s, t in SIZES]
FULL = [((1168, 1752), (584, 876)), ((1169, 1753), (584, 876))]             # a scannetpp photograph at --res_scale 0.5: the exact-2 and the general path
CONTENTS = ("random", "white", "checker")


@functools.lru_cache(maxsize=None)
def content(name, hw, channels, seed=0):
    """random bytes, an all-255 image, or a 0 / 255 checkerboard of single pixels (the extremes of the intermediate sums); read-only, shared by the tests"""
    H, W = hw
    shape = (H, W) if channels == 1 else (H, W, channels)
    if name == "random":
        a = np.random.default_rng([seed, H, W, channels]).integers(0, 256, shape, dtype=np.uint8)
    elif name == "white":
        a = np.full(shape, 255, np.uint8)
    else:
        y, x = np.mgrid[0:H, 0:W]
        a = (((y + x) % 2) * 255).astype(np.uint8)
        a = a if channels == 1 else np.ascontiguousarray(np.repeat(a[..., None], channels, 2))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def linear_ref(name, src_hw, dst_hw, channels, seed=0):
    out = resize_ref.resize_linear_u8(content(name, src_hw, channels, seed), dst_hw)
    out.setflags(write=False)
    return out


# ---- (a) hand cases
def test_hand_cases():
    g = np.random.default_rng(1)
    a = g.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    assert resize_ref.resize_linear_u8(a, (5, 7)) is a                                          # same size: the source, unchanged
    assert np.array_equal(resize_ref.resize_nearest_u8(a[..., 0], (5, 7)), a[..., 0])
    for block, want in (([[1, 2], [3, 4]], 3), ([[0, 0], [0, 1]], 0), ([[1, 1], [0, 0]], 1), ([[1, 1], [1, 0]], 1), ([[255, 255], [255, 255]], 255),
                        ([[255, 254], [254, 254]], 254), ([[0, 255], [255, 0]], 128)):
        got = resize_ref.resize_linear_u8(np.array(block, np.uint8), (1, 1))                    # (a + b + c + d + 2) >> 2
        assert got.shape == (1, 1) and int(got[0, 0]) == want == (sum(map(sum, block)) + 2) >> 2, block
    for v in (0, 1, 127, 200, 255):                                                             # a one-pixel source: that value everywhere, through the general path
        assert np.array_equal(resize_ref.resize_linear_u8(np.full((1, 1, 3), v, np.uint8), (3, 3)), np.full((3, 3, 3), v, np.uint8))
        assert np.array_equal(resize_ref.resize_nearest_u8(np.full((1, 1), v, np.uint8), (3, 2)), np.full((3, 2), v, np.uint8))
    # the weights of 16 -> 8 (scale exactly 2: f = 0.5 everywhere) and the clamp at both ends of 5 -> 10
    ofs, coef = resize_ref.linear_axis(16, 8)
    assert ofs.tolist() == list(range(0, 16, 2)) and (coef == 1024).all()
    ofs, coef = resize_ref.linear_axis(5, 10)
    assert ofs[0] == 0 and coef[0].tolist() == [2048, 0] and ofs[-1] == 4 and coef[-1].tolist() == [2048, 0]
    assert ofs.dtype == np.int32 and coef.dtype == np.int16 and (coef.sum(1) == 2048).all()


# ---- (b) closeness to exact bilinear interpolation
@pytest.mark.parametrize("sizes", SIZES[:5] + FULL[1:], ids=SIZE_IDS[:5] + ["1169x1753-584x876"])
def test_linear_is_within_one_code_value_of_exact_bilinear(sizes):
    """The bound is a condition, not a measurement: the 11-bit weights are off by at most 2^-12 each (two per pass: 2 * 2^-12 * 255 = 0.12 per pass), the two
    truncations (>> 4 of the 11 fractional bits leaves 7, >> 16 of the product leaves 2) lose under 0.04, and the final (+ 2) >> 2 rounds to half a code
    value: below 1 in all.  Exact 2: the rounded mean, at most 0.5."""
    import torch.nn.functional as F
    src, dst = sizes
    worst = 0.0
    for name in CONTENTS:
        s = content(name, src, 3)
        exact = F.interpolate(torch.from_numpy(np.array(s)).double().permute(2, 0, 1)[None], size=dst, mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
        err = float(np.abs(linear_ref(name, src, dst, 3).astype(np.float64) - exact).max())
        print(src, dst, name, err)
        worst = max(worst, err)
    assert worst < 1.0
    if src == (2 * dst[0], 2 * dst[1]):
        assert worst <= 0.5


# ---- (c) nearest against PIL
def nearest_pil(a, hw):
    from PIL import Image
    return np.array(Image.fromarray(a).resize((hw[1], hw[0]), Image.NEAREST))


def test_nearest_equals_pil():
    g = np.random.default_rng(2)
    pairs = [(tuple(g.integers(1, 91, 2)), tuple(g.integers(1, 91, 2))) for _ in range(300)] + SIZES + [((1168, 1752), (584, 876)), ((1169, 1753), (584, 876))]
    for src, dst in pairs:
        a = g.integers(0, 256, src, dtype=np.uint8)
        assert np.array_equal(resize_ref.resize_nearest_u8(a, dst), nearest_pil(a, dst)), (src, dst)
    # the multiply form is NOT the contract
    a = g.integers(0, 256, (24, 40), dtype=np.uint8)
    ys, xs = (np.floor((np.arange(n) + 0.5) * (m / n)).astype(int) for m, n in ((24, 9), (40, 15)))
    assert not (np.array_equal(ys, resize_ref.nearest_axis(24, 9)) and np.array_equal(xs, resize_ref.nearest_axis(40, 15)))


# ---- the library's host tables
def test_library_tables_equal_the_restatement():
    from iris_amd import _lib as L
    from iris_amd.utils import resize
    axes = sorted({(s[k], t[k]) for s, t in SIZES + FULL + [((12, 16), (6, 8)), ((16, 12), (8, 6))] for k in (0, 1)})
    for ns, nd in axes:
        ofs, coef = resize.axis_tables("linear", ns, nd)
        want_ofs, want_coef = resize_ref.linear_axis(ns, nd)
        assert ofs.dtype == np.int32 and coef.dtype == np.int16 and coef.shape == (nd, 2)
        assert np.array_equal(ofs, want_ofs) and np.array_equal(coef, want_coef), (ns, nd)
        ofs, coef = resize.axis_tables("nearest", ns, nd)
        assert coef is None and np.array_equal(ofs, resize_ref.nearest_axis(ns, nd)), (ns, nd)
    for ns, nd in ((0, 4), (4, 0), (65536, 4), (4, 65536)):
        with pytest.raises(L.IrisError, match="1..65535"):
            resize.axis_tables("linear", ns, nd)
    with pytest.raises(L.IrisError, match="mode"):
        resize.axis_tables("cubic", 4, 4)


def test_resize_refusals_need_no_device(monkeypatch):
    from iris_amd import _lib as L
    from iris_amd.utils.resize import resize_u8
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("a refused call reached the library"))
    for bad in (torch.zeros(4, 4, 3, dtype=torch.uint8), [torch.zeros(4, 4, dtype=torch.uint8)], np.zeros((4, 4, 3), np.uint8)):
        with pytest.raises(L.IrisError):
            resize_u8(bad, (2, 2))
    with pytest.raises(L.IrisError, match="mode"):
        resize_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), (2, 2), "cubic")


# ---- the scannetpp layout at --res_scale 0.5, on a tree written here
def scannetpp_tree(root, scene="sc0", folders=("images",)):
    """the golden camera files (1169 x 1753 views; five of the six train names have a frame), a mesh file's name, and full-size 8-bit files"""
    from PIL import Image
    from iris_amd.utils import cameras
    _scannetpp_scene(str(root), scene)
    os.makedirs(root / "data" / scene / "scans")
    open(root / "data" / scene / "scans" / "scene.ply", "w").close()
    _, views = cameras.load_scannetpp(str(root), scene, 1.0, "train")
    for folder in folders:
        os.makedirs(root / "data" / scene / "psdf" / folder)
        for v in views:
            Image.fromarray(np.zeros((1169, 1753, 3), np.uint8)).save(root / "data" / scene / "psdf" / folder / v["name"], quality=10)
    return views


def prebake_args(root, scene="sc0", res_scale=0.5):
    return argparse.Namespace(dataset="scannetpp", dataset_root=str(root), scene=scene, res_scale=res_scale, ldr_img_dir=None, cameras=None, max_views=None)


def test_scannetpp_photographs_and_prebake_at_half_resolution(tmp_path, monkeypatch):
    from iris_amd import slf_bake
    from iris_amd._lib import IrisError
    from iris_amd.utils import stage
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the host half of a stage opened the device"))
    views = scannetpp_tree(tmp_path)
    img_hw, got, photos = stage.load_photographs("scannetpp", str(tmp_path), "sc0", 0.5)
    assert img_hw == (584, 876) and [v["name"] for v in got] == [v["name"] for v in views] and len(views) == 5
    assert photos == [(str(tmp_path / "data" / "sc0" / "psdf" / "images" / v["name"]), 1.0) for v in views]       # the full-size files' paths
    mesh, hw, got, photos2 = slf_bake.open_prebake(prebake_args(tmp_path), "slf_bake", need_exposure=True)
    assert hw == (584, 876) and photos2 == photos and mesh.endswith("scene.ply")
    assert stage.layout_resizes("scannetpp") and not stage.layout_resizes("scannetpp", "cameras.json") and not stage.layout_resizes("real")
    a = stage.read_photograph(photos[0][0], hw, resize=True)
    assert a.shape == (1169, 1753, 3) and a.dtype == np.uint8                                    # full size: the device resizes it
    with pytest.raises(IrisError, match="resizing"):
        stage.read_photograph(photos[0][0], hw)
    with pytest.raises(IrisError, match="resizing"):                                             # another layout's files are not resized
        stage.check_photograph_size(photos[0][0], hw, stage.layout_resizes("real"))
    os.remove(photos[2][0])
    with pytest.raises(FileNotFoundError, match=views[2]["name"]):
        slf_bake.open_prebake(prebake_args(tmp_path), "slf_bake", need_exposure=True)


def test_an_exr_photograph_of_the_wrong_size_stays_refused(tmp_path):
    from iris_amd._lib import IrisError
    from iris_amd.utils import stage
    from iris_amd.utils.exr import write_exr
    path = str(tmp_path / "a.exr")
    write_exr(path, np.zeros((4, 6, 3), np.float32))
    stage.check_photograph_size(path, (4, 6), resize=True)
    with pytest.raises(IrisError, match="resizing"):
        stage.check_photograph_size(path, (2, 3), resize=True)


def trainer_args(root, scene, **changes):
    return argparse.Namespace(**dict(dict(dataset=["scannetpp", str(root)], scene=scene, res_scale=0.5, ldr_img_dir=None, optimizer="Adam", learning_rate=1e-3,
                                          weight_decay=0.0), **changes))


def test_trainers_refuse_an_incomplete_scannetpp_root_before_the_device(tmp_path, monkeypatch, capsys):
    from iris_amd import train_brdf_crf
    from iris_amd._lib import IrisError
    from iris_amd.utils import stage
    from iris_amd.utils.dataset import files
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a refused command opened the device"))
    empty = tmp_path / "empty"
    os.makedirs(empty)
    with pytest.raises(IrisError, match="scannetpp.*train_test_lists.json"):                     # an IrisError naming the layout and the path
        stage.refuse_unbuilt_training(trainer_args(empty, "room"))
    with pytest.raises(IrisError, match="scannetpp.*train_test_lists.json"):
        files.load_training_files("scannetpp", str(empty), None, res_scale=0.5, scene="room")
    common = ["--experiment_name", "x", "--checkpoint_path", str(tmp_path / "c"), "--log_path", str(tmp_path / "l"), "--cache_dir", str(tmp_path)]
    assert train_brdf_crf.cli(common + ["--dataset", "scannetpp", str(empty), "--scene", "room", "--res_scale", "0.5"]) == 2
    err = capsys.readouterr().err
    assert "scannetpp" in err and "train_test_lists.json" in err and len(err.strip().splitlines()) == 1
    # a complete tree passes; the check opens the first view's three files only, and only their headers
    full = tmp_path / "full"
    os.makedirs(full)
    views = scannetpp_tree(full, folders=("images", "albedo", "seg"))
    from PIL import Image
    opened = []
    real_open = Image.open
    monkeypatch.setattr(Image, "open", lambda path, *a, **k: (opened.append(str(path)), real_open(path, *a, **k))[1])
    monkeypatch.setattr(Image.Image, "load", lambda self: pytest.fail("the check decoded an image"))
    stage.refuse_unbuilt_training(trainer_args(full, "sc0"))
    assert opened == [str(full / "data" / "sc0" / "psdf" / d / views[0]["name"]) for d in ("images", "albedo", "seg")]
    monkeypatch.undo()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a refused command opened the device"))
    os.remove(full / "data" / "sc0" / "psdf" / "seg" / views[0]["name"])
    with pytest.raises(FileNotFoundError, match="seg"):
        stage.refuse_unbuilt_training(trainer_args(full, "sc0"))
    os.remove(full / "data" / "sc0" / "scans" / "scene.ply")
    with pytest.raises(IrisError, match="mesh not found"):
        stage.refuse_unbuilt_training(trainer_args(full, "sc0"))
    # the other layouts still take no scale
    with pytest.raises(IrisError, match="res_scale"):
        stage.refuse_unbuilt_training(trainer_args(full, "", dataset=["real", str(full)], ldr_img_dir="ldr"))
    assert not (tmp_path / "c").exists() and not (tmp_path / "l").exists()
