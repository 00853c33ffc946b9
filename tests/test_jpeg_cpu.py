"""The JPEG frame contract without a GPU: tests/jpeg_ref.py (the contract in numpy) against Pillow's decoder and encoder, the headers and the size bound of the
library against it, and the two stages' command lines.  tests/test_jpeg.py holds the device encoder to jpeg_ref byte for byte; this file shows that what
jpeg_ref writes is a JPEG file as good as libjpeg's own at the same tables."""
import functools
import io
import sys

import numpy as np
import pytest

import jpeg_ref
from test_video import ref_pixels

# (H, W, C) before the crop, magma: one MCU; smaller than a block; odd both ways; partial MCUs both ways and two intervals; 66 MCUs per row (396 blocks per
# interval: more than a wave has lanes), grey and RGB; ten MCU rows (the RST counter wraps); the colour map
SHAPES = [((16, 16, 3), False), ((2, 2, 1), False), ((3, 5, 3), False), ((18, 34, 3), False), ((8, 1042, 1), False), ((16, 1042, 3), False), ((146, 18, 3), False),
          ((40, 24, 1), True)]
SHAPE_IDS = ["%dx%dx%d%s" % (*s, "_magma" if m else "") for s, m in SHAPES]
CONTENTS = ("noise", "ramp", "flat", "checker", "clipped", "uint8")


def content(name, shape, seed=0):
    """-> (image, divisor, quality).  noise: uniform (its stream holds FF bytes); ramp: smooth in both directions, the channels at different slopes; flat; checker:
    the upper half 8 x 8 squares of 0 and 1 (DC differences of category 11), the lower half single pixels of 0 and 1 (AC category 10), at quality 100; clipped:
    NaN, +-inf, negatives and values above the divisor 10; uint8: noise that skips the quantiser"""
    H, W, C = shape
    rng = np.random.default_rng([seed, H, W, C, CONTENTS.index(name)])
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    if name == "noise":
        return rng.random(shape, dtype=np.float32), 1.0, 90
    if name == "ramp":
        return np.stack([(0.1 + 0.8 * (s * x / W + (1 - s) * y / H)).astype(np.float32) for s in (0.25, 0.5, 0.75)][:C], -1), 1.0, 90
    if name == "flat":
        return np.full(shape, 0.4, np.float32), 1.0, 90
    if name == "checker":
        a = np.where(y < H // 2, (y // 8 + x // 8) % 2, (y + x) % 2).astype(np.float32)
        return np.repeat(a[..., None], C, 2), 1.0, 100
    if name == "clipped":
        vals = np.array([np.nan, np.inf, -np.inf, -5.0, 0.0, 2.5, 5.0, 7.5, 10.0, 15.0, 3000.0], np.float32)
        return np.repeat(rng.choice(vals, (H * W * C + 4) // 5), 5)[:H * W * C].reshape(shape), 10.0, 90
    return rng.integers(0, 256, shape, dtype=np.uint8), 1.0, 90


@functools.lru_cache(maxsize=None)
def coded(k, name, quality=None, seed=0):
    """-> (the pixels that get coded, jpeg_ref's file) for SHAPES[k] and the content `name`; computed once, shared by the tests (test_jpeg.py's too)"""
    shape, magma = SHAPES[k]
    image, divisor, q = content(name, shape, seed)
    px = np.ascontiguousarray(ref_pixels(image, divisor, magma))
    data = jpeg_ref.encode(px, quality or q)
    px.setflags(write=False)
    return px, data


def decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return 100.0 if mse == 0 else min(100.0, 10 * np.log10(255.0 ** 2 / mse))


def rgb(px):
    return px if px.ndim == 3 else np.repeat(px[..., None], 3, 2)


def walk(data):
    """-> (segments in front of the entropy-coded data as (marker, payload), the entropy-coded data, what follows it)"""
    assert data[:2] == b"\xff\xd8"
    segs, o = [(0xD8, b"")], 2
    while True:
        assert data[o] == 0xFF, o
        marker, n = data[o + 1], int.from_bytes(data[o + 2:o + 4], "big")
        segs.append((marker, data[o + 4:o + 2 + n]))
        o += 2 + n
        if marker == 0xDA:
            break
    end = len(data) - 2
    return segs, data[o:end], data[end:]


def check_structure(data, width, height):
    """the marker structure the contract states; returns the entropy-coded data"""
    segs, ecs, tail = walk(data)
    markers = [m for m, _ in segs]
    assert markers == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA] and tail == b"\xff\xd9"
    assert segs[1][1] == b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
    sof = segs[4][1]
    assert sof[0] == 8 and int.from_bytes(sof[1:3], "big") == height and int.from_bytes(sof[3:5], "big") == width and sof[5:] == bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    mcus, rows = (width + 15) // 16, (height + 15) // 16
    assert int.from_bytes(segs[9][1], "big") == mcus
    rst, o = [], 0
    while True:
        o = ecs.find(b"\xff", o)
        if o < 0:
            break
        assert o + 1 < len(ecs) and (ecs[o + 1] == 0 or 0xD0 <= ecs[o + 1] <= 0xD7), (o, ecs[o + 1:o + 2])
        if ecs[o + 1]:
            rst.append(ecs[o + 1] - 0xD0)
        o += 2
    assert rst == [m % 8 for m in range(rows - 1)]
    return ecs


def test_tables_are_the_ones_libjpeg_writes():
    """Annex K as typed into jpeg_ref.py and as the library holds it == the DHT and (at quality 50, where the scaling is the identity) DQT segments of a file
    written by Pillow's libjpeg"""
    from PIL import Image
    from iris_amd.utils import jpeg
    out = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(out, "JPEG", quality=50, subsampling=2, optimize=False)
    segs, _, _ = walk(out.getvalue())
    theirs = {p[0]: p[1:] for m, p in segs if m == 0xC4}
    assert len(theirs) == 4
    for ident, (bits, vals) in ((0x00, jpeg_ref.DC_LUMA), (0x10, jpeg_ref.AC_LUMA), (0x01, jpeg_ref.DC_CHROMA), (0x11, jpeg_ref.AC_CHROMA)):
        assert theirs[ident] == bytes(bits) + bytes(vals)
    dqt = {p[0]: p[1:] for m, p in segs if m == 0xDB}
    zz = jpeg_ref.zigzag()
    assert dqt[0] == bytes(jpeg_ref.QUANT_LUMA[zz].tolist()) and dqt[1] == bytes(jpeg_ref.QUANT_CHROMA[zz].tolist())
    t = jpeg.tables()
    assert [(i, bytes(b), bytes(v)) for i, b, v in t["dht"]] == [(i, bytes(b), bytes(v)) for i, (b, v) in ((0x00, jpeg_ref.DC_LUMA), (0x10, jpeg_ref.AC_LUMA),
                                                                                                         (0x01, jpeg_ref.DC_CHROMA), (0x11, jpeg_ref.AC_CHROMA))]
    assert np.array_equal(t["zigzag"], zz) and np.array_equal(t["quant"], np.stack([jpeg_ref.QUANT_LUMA, jpeg_ref.QUANT_CHROMA]))
    for q in (1, 10, 49, 50, 75, 90, 100):
        assert np.array_equal(np.asarray(jpeg.quant_tables(q)), jpeg_ref.quant_tables(q))
        for w, h in ((2, 2), (34, 18), (1920, 1080)):
            assert jpeg.jpeg_headers(w, h, q) == jpeg_ref.headers(w, h, q)


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_decodes_in_pil_with_the_stated_structure(k):
    (H, W, C), magma = SHAPES[k]
    for name in CONTENTS:
        px, data = coded(k, name)
        assert px.shape[:2] == (H - H % 2, W - W % 2)
        ecs = check_structure(data, px.shape[1], px.shape[0])
        im = decode(data)
        assert im.mode == "RGB" and im.size == (px.shape[1], px.shape[0])
        a = np.asarray(im)
        if px.ndim == 2:
            assert (a[..., 0] == a[..., 1]).all() and (a[..., 1] == a[..., 2]).all()
        if name == "noise" and px.size >= 256:
            assert b"\xff\x00" in ecs
        if name == "flat":
            assert np.abs(a.astype(int) - rgb(px)).max() <= 1


def test_checkerboard_reaches_the_largest_categories():
    px, _ = coded(0, "checker")
    Y, _, _ = jpeg_ref.planes(px)
    c = jpeg_ref.coefficients(Y, jpeg_ref.quant_tables(100)[0])
    assert abs(int(c[0, 1, 0]) - int(c[0, 0, 0])) >= 1024 and 512 <= np.abs(c[..., 1:]).max() <= 1023


def test_fidelity_against_libjpeg():
    """PSNR against the coded pixels: ours >= Pillow's own encoder (the same tables, 4:2:0, standard Huffman tables) - jpeg_ref.MARGIN_DB; the deficits are
    printed (pytest -s) and recorded in jpeg_ref.MEASURED_DEFICITS"""
    from PIL import Image
    worst = {}
    for q in (50, 90, 100):
        qt = jpeg_ref.quant_tables(q)
        for k in range(len(SHAPES)):
            for name in CONTENTS:
                px, data = coded(k, name, q)
                out = io.BytesIO()
                Image.fromarray(rgb(px)).save(out, "JPEG", qtables=[qt[0].tolist(), qt[1].tolist()], subsampling=2, optimize=False)
                ours, theirs = psnr(np.asarray(decode(data)), rgb(px)), psnr(np.asarray(decode(out.getvalue())), rgb(px))
                print("q %3d %-16s %-8s ours %6.2f dB  libjpeg %6.2f dB  deficit %+.3f" % (q, SHAPE_IDS[k], name, ours, theirs, theirs - ours))
                if theirs - ours > worst.get(q, (-1e9,))[0]:
                    worst[q] = (theirs - ours, SHAPE_IDS[k], name)
    print("largest deficits", worst)
    for q, (deficit, shape, name) in worst.items():
        assert deficit <= jpeg_ref.MARGIN_DB[q], (q, shape, name, deficit)
        assert jpeg_ref.MARGIN_DB[q] == np.ceil(jpeg_ref.MEASURED_DEFICITS[q] * 4) / 4 + 0.25


@pytest.mark.parametrize("quality", [90, 100])
def test_flat_grey_is_exact(quality):
    """the DC step is at most 3 at quality >= 90: the error of the DC is at most 1.5 / 8 of a level and every AC coefficient is zero"""
    assert jpeg_ref.quant_tables(quality)[0][0] <= 3
    for v in range(256):
        a = np.asarray(decode(jpeg_ref.encode(np.full((16, 16), v, np.uint8), quality)))
        assert (a == v).all(), v


def test_stream_bound_holds_on_the_checkerboard():
    """single pixels of 0 and 255 at quality 100: the content built to approach the bound"""
    from iris_amd import _lib as L
    for H, W in ((16, 16), (18, 34), (2, 2), (32, 1042)):
        y, x = np.mgrid[0:H, 0:W]
        data = jpeg_ref.entropy_data((((y + x) % 2) * 255).astype(np.uint8), 100)
        bound = int(L.lib().iris_jpeg_stream_bound(H, W))
        assert bound == ((H + 15) // 16) * (2 * (((W + 15) // 16 * 6 * 1660 + 7) // 8) + 2)
        assert len(data) <= bound
    assert int(L.lib().iris_jpeg_stream_bound(1, 8)) == 0 and int(L.lib().iris_jpeg_stream_bound(8, 65538)) == 0


def test_host_refusals_need_no_device():
    from iris_amd._lib import IrisError
    from iris_amd.utils import jpeg
    for q in (0, 101, 90.5, None):
        with pytest.raises(IrisError, match="quality"):
            jpeg.quant_tables(q)
    with pytest.raises(IrisError):
        jpeg.jpeg_headers(0, 4, 90)


# the parser main() parses with: render_relight keeps build_parser() as the pinned table of its earlier options and adds the two in build_video_parser()
PARSER = {"render_video": "build_parser", "render_relight": "build_video_parser"}


def _base(module):
    return ["--experiment_name", "e", "--emitter_path", "b"] + (["--light_cfg", "l.json"] if module == "render_relight" else [])


@pytest.mark.parametrize("module", ["render_video", "render_relight"])
def test_command_line(module, capsys):
    import importlib
    stage = importlib.import_module("iris_amd." + module)
    args = getattr(stage, PARSER[module])().parse_args(_base(module) + ["--video", "mjpeg", "--video_quality", "75"])
    assert (args.video, args.video_quality) == ("mjpeg", 75)
    args = getattr(stage, PARSER[module])().parse_args(_base(module))
    assert (args.video, args.video_quality) == ("none", 90)
    for bad in (["--video_quality", "0"], ["--video_quality", "101"], ["--video", "h264"]):
        with pytest.raises(SystemExit) as e:                     # argparse's exit, from main(): before the data is read and the device opened
            stage.main(_base(module) + ["--video", "mjpeg"] + bad)
        assert e.value.code == 2 and bad[0] in capsys.readouterr().err


def test_parsers_do_not_import_the_video_modules():
    """in a fresh interpreter: after the stage's parser is built and a parse with --video none neither utils.jpeg nor utils.avi is loaded"""
    import os
    import subprocess
    from conftest import REPO
    code = "import sys\n" + "".join("from iris_amd import {m} as S; S.{p}().parse_args({a!r})\n".format(m=m, p=PARSER[m], a=_base(m)) for m in PARSER)
    code += "sys.exit(3 if 'iris_amd.utils.jpeg' in sys.modules or 'iris_amd.utils.avi' in sys.modules else 0)"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
