"""The JPEG frames of the video stage on the GPU (iris_amd/csrc/iris_jpeg.h, iris_amd/utils/jpeg.py): the device encoder against tests/jpeg_ref.py BYTE FOR
BYTE -- the contract is integer arithmetic, so there is no tolerance --, then the frame writer and the two stages with --video mjpeg.  The coded pixels are
test_video.py's ref_pixels; the shapes and contents are test_jpeg_cpu.py's, which shows on the CPU that jpeg_ref's files are sound JPEG."""
import io
import os
import re
import struct

import numpy as np
import pytest
import torch

import jpeg_ref
from conftest import REPO
from test_jpeg_cpu import CONTENTS, SHAPE_IDS, SHAPES, check_structure, coded, content
from test_video import _common, decode as decode_png, ref_pixels, tree  # noqa: F401  (tree: the module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB"
    return np.asarray(im)


def avi_chunks(path):
    """the '00dc' chunks of an .avi file, through its idx1"""
    data = open(path, "rb").read()
    movi = data.index(b"movi")
    at = data.rindex(b"idx1")
    n = struct.unpack_from("<I", data, at + 4)[0] // 16
    assert struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and at + 8 + 16 * n == len(data)
    out = []
    for k in range(n):
        ckid, flags, off, size = struct.unpack_from("<4sIII", data, at + 8 + 16 * k)
        assert ckid == b"00dc" and data[movi + off:movi + off + 4] == b"00dc" and struct.unpack_from("<I", data, movi + off + 4)[0] == size
        out.append(data[movi + off + 8:movi + off + 8 + size])
    return out


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_device_file_is_the_reference_file(k):
    """the six contents of a shape in ONE call (one group of float images, the uint8 image a second group) at the content's quality"""
    from iris_amd.utils import jpeg
    shape, magma = SHAPES[k]
    by_quality = {}
    for name in CONTENTS:
        by_quality.setdefault(content(name, shape)[2], []).append(name)
    for quality, names in by_quality.items():
        images = [content(name, shape) for name in names]
        files = jpeg.encode_frames_device([torch.from_numpy(a).to(DEV) for a, _, _ in images], [d for _, d, _ in images], [magma] * len(names), quality)
        assert len(files) == len(names)
        for name, data in zip(names, files):
            px, want = coded(k, name)
            ecs = check_structure(data, px.shape[1], px.shape[0])
            assert data == want, (name, len(data), len(want), next(i for i, (a, b) in enumerate(zip(data + b"\0", want + b"\0")) if a != b))
            a = decode(data)
            assert a.shape == px.shape[:2] + (3,)
            if px.ndim == 2:
                assert (a[..., 0] == a[..., 1]).all() and (a[..., 1] == a[..., 2]).all()
            if name == "noise" and px.size >= 256:
                assert b"\xff\x00" in ecs
        assert jpeg.encode_frames_device([torch.from_numpy(a).to(DEV) for a, _, _ in images], [d for _, d, _ in images], [magma] * len(names), quality) == files


def test_mixed_list_and_more_images_than_one_launch_takes():
    """one call with different sizes, float and uint8, magma and not, and more equal images than one transform launch takes: the files come in the order of the
    images, each equal to its single-image encoding and to the reference"""
    from iris_amd.utils import jpeg
    group = int(re.search(r"kPngMaxImages = (\d+);", open(os.path.join(REPO, "iris_amd", "csrc", "iris_png.h")).read()).group(1))
    rng = np.random.default_rng(5)
    images = [rng.random((6, 10), dtype=np.float32) * np.float32(0.3 * (j % 4) + 0.2) for j in range(group + 3)]
    flags = [j % 3 == 0 for j in range(group + 3)]
    images[2:2] = [rng.integers(0, 256, (18, 34, 3), dtype=np.uint8), rng.random((7, 9, 3), dtype=np.float32), rng.integers(0, 256, (6, 10), dtype=np.uint8)]
    flags[2:2] = [False, False, True]
    dev = [torch.from_numpy(a).to(DEV) for a in images]
    files = jpeg.encode_frames_device(dev, None, flags, 75)
    assert len(files) == len(images)
    for j, (a, m, data) in enumerate(zip(images, flags, files)):
        assert data == jpeg_ref.encode(ref_pixels(a, 1.0, m), 75), j
    for j in (0, 2, 3, 4, group + 5):
        assert jpeg.encode_frames_device([dev[j]], None, [flags[j]], 75) == [files[j]]
    # a non-contiguous view is taken as the image it shows
    base = torch.from_numpy(rng.random((20, 22, 3), dtype=np.float32)).to(DEV)
    assert jpeg.encode_frames_device([base[1:19, 2:20]]) == [jpeg_ref.encode(ref_pixels(base[1:19, 2:20].cpu().numpy()), 90)]


def test_refusals():
    from iris_amd._lib import IrisError
    from iris_amd.utils import jpeg
    with pytest.raises(IrisError, match="empty"):
        jpeg.encode_frames_device([torch.zeros(1, 7, 3, device=DEV)])
    with pytest.raises(IrisError, match="empty"):
        jpeg.encode_frames_device([torch.zeros(6, 1, device=DEV)])
    with pytest.raises(IrisError, match="magma"):
        jpeg.encode_frames_device([torch.zeros(4, 4, 3, device=DEV)], None, [True])
    with pytest.raises(IrisError):
        jpeg.encode_frames_device([torch.zeros(4, 4, 2, device=DEV)])
    with pytest.raises(IrisError):
        jpeg.encode_frames_device([torch.zeros(4, 4, 3)])                                  # a host tensor: there is no CPU path
    for d in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(IrisError, match="divisor"):
            jpeg.encode_frames_device([torch.zeros(4, 4, 3, device=DEV)], [d])
    for q in (0, 101):
        with pytest.raises(IrisError, match="quality"):
            jpeg.encode_frames_device([torch.zeros(4, 4, 3, device=DEV)], quality=q)
    with pytest.raises(IrisError):
        jpeg.encode_frames_device([])


def test_frame_writer_with_video(tree):  # noqa: F811
    """render_video's frame writer with video="mjpeg" on ONE render_view output (12 x 16, SPP 2, spp 1) submitted as three frames: eight .avi files of six
    chunks -- frames 0 1 2 2 1 0, each the reference's file for that map --, and the PNG files and lists exactly as without the option"""
    from iris_amd import render_video as RV
    from iris_amd.render import render_view
    from iris_amd.utils import cameras
    from stub_material import StubMaterial
    H, W = tree["hw"]
    img_hw, views = cameras.load_trajectory("real", str(tree["data"]), "", 1.0, split="val")
    rays = cameras.view_rays(views[1], img_hw, torch.device(DEV), ray_diff=True)
    torch.manual_seed(5); torch.cuda.manual_seed(5)
    out = render_view(tree["scene"], tree["em"], StubMaterial(), tree["crf"].to(DEV), rays, img_hw, 2, 1, 2, exposure=1.0, gt=None)
    want = [ref_pixels(out[key].cpu().numpy(), d, m) for _, _, key, d, m in RV.FRAME_FILES]
    roots = {}
    for video in ("none", "mjpeg"):
        roots[video] = str(tree["root"] / ("jpeg_frames_" + video))
        writer = RV.FrameWriter(torch.device(DEV), "device", video=video, video_quality=80)
        paths = [writer.submit(roots[video], i, out) for i in range(3)]
        writer.close()
        RV.write_lists(roots[video], 3)
        for ps in paths:
            for p, w in zip(ps, want):
                np.testing.assert_array_equal(decode_png(open(p, "rb").read()), w, err_msg=p)
    listing = {v: sorted(os.path.relpath(os.path.join(d, n), roots[v]) for d, _, names in os.walk(roots[v]) for n in names) for v in roots}
    avis = sorted(name + ".avi" for _, name, _, _, _ in RV.FRAME_FILES)
    assert len(listing["none"]) == 24 + 8 and not [n for n in listing["none"] if n.endswith(".avi")]
    assert sorted(set(listing["mjpeg"]) - set(listing["none"])) == avis and set(listing["none"]) <= set(listing["mjpeg"])
    for n in listing["none"]:
        a, b = open(os.path.join(roots["none"], n), "rb").read(), open(os.path.join(roots["mjpeg"], n), "rb").read()
        assert a == b, n
    for (_, name, _, _, _), px in zip(RV.FRAME_FILES, want):
        chunks = avi_chunks(os.path.join(roots["mjpeg"], name + ".avi"))
        assert len(chunks) == 6
        ref = jpeg_ref.encode(px, 80)
        for c in range(3):
            assert chunks[c] == ref and chunks[5 - c] == chunks[c], (name, c)
        assert decode(chunks[0]).shape == (H, W, 3)
    from iris_amd._lib import IrisError
    with pytest.raises(IrisError, match="'none' or 'mjpeg'"):
        RV.FrameWriter(torch.device(DEV), "device", video="h264")


def test_stages_write_their_videos(tree):  # noqa: F811
    from iris_amd import render_relight as RR
    from iris_amd import render_video as RV
    out = tree["root"] / "jpeg_video"
    RV.main(_common(tree, out) + ["--indir_depth", "2", "--video", "mjpeg", "--max_views", "2"])
    H, W = tree["hw"]
    for _, name, _, _, _ in RV.FRAME_FILES:
        chunks = avi_chunks(str(out / (name + ".avi")))
        assert len(chunks) == 4 and chunks[0] == chunks[3] and chunks[1] == chunks[2]
        assert decode(chunks[1]).shape == (H, W, 3)
        check_structure(chunks[0], W, H)
    # the rgb frames are the JPEG of the pixels of the PNG files beside them
    for i, c in enumerate(avi_chunks(str(out / "rgb_full.avi"))[:2]):
        assert c == jpeg_ref.encode(decode_png(open(RV.frame_paths(str(out), i)[0], "rb").read()), 90)
    assert sorted(n for n in os.listdir(out) if n.endswith(".ffconcat")) == sorted(name + ".ffconcat" for _, name, _, _, _ in RV.FRAME_FILES)
    rel = tree["root"] / "jpeg_relight"
    RR.main(_common(tree, rel) + ["--mode", "traj", "--light_cfg", str(tree["data"] / "relight.json"), "--indir_depth", "1", "--sphere_subdiv", "0", "--video", "mjpeg",
                                  "--video_quality", "75", "--max_views", "2"])
    chunks = avi_chunks(str(rel / "relight.avi"))
    assert len(chunks) == 4 and chunks[0] == chunks[3] and chunks[1] == chunks[2]
    for i in range(2):
        assert chunks[i] == jpeg_ref.encode(decode_png(open(rel / ("%05d_rgb.png" % i), "rb").read()), 75)
    assert os.path.isfile(rel / "relight.ffconcat")


def test_without_the_option_no_video_is_written(tree):  # noqa: F811
    from iris_amd import render_relight as RR
    from iris_amd import render_video as RV
    out = tree["root"] / "jpeg_none"
    RV.main(_common(tree, out) + ["--indir_depth", "2", "--max_views", "1"])
    files = sorted(os.path.relpath(os.path.join(d, n), out) for d, _, names in os.walk(out) for n in names)
    assert files == sorted([os.path.relpath(p, out) for p in RV.frame_paths(str(out), 0)] + [name + ".ffconcat" for _, name, _, _, _ in RV.FRAME_FILES])
    rel = tree["root"] / "jpeg_relight_none"
    RR.main(_common(tree, rel) + ["--mode", "traj", "--light_cfg", str(tree["data"] / "relight.json"), "--indir_depth", "1", "--sphere_subdiv", "0", "--max_views", "1"])
    assert sorted(os.listdir(rel)) == ["00000_rgb.exr", "00000_rgb.png", "relight.ffconcat"]
