"""The video stage on the GPU: PNG files encoded on the device (iris_amd/csrc/iris_png.h, iris_amd/utils/png.py), render_video's frame writer and CLI, and
render_relight --mode traj from the scene's own trajectory.

The reference for pixels is the numpy statement of the reference's save_image written here (`ref_pixels`), never the code under test; the MAGMA table it uses is
matplotlib's published data.  Every comparison is exact: the files are lossless and the quantiser is specified bit for bit.

Size bound.  iris_deflate.h cuts an image's scanline bytes into segments of kZipSeg = 16384 bytes; a segment is stored (5 bytes of block header + its bytes)
whenever the Huffman-coded block with its 4-byte sync marker would not be smaller, so a segment never exceeds its bytes + 5; the stream adds the 2-byte zlib header
and the 4-byte Adler-32:  len(IDAT) <= raw + 5 * ceil(raw / 16384) + 6.  (The bound asked of this encoder was raw + 9 per segment + 6 -- stored header 5 + sync
marker 4; a stored block is byte-aligned by itself and carries no marker, so the exact constant is 5 and the test holds the encoder to it.)"""
import io
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEG = 16384


# ---- the reference, in numpy
def magma_rgb():
    try:
        from matplotlib._cm_listed import _magma_data
        return np.rint(np.asarray(_magma_data, np.float32) * 255).astype(np.uint8)
    except ImportError:                                                    # (tests/test_video_cpu.py ties the library's table to matplotlib's where it is installed)
        from iris_amd.utils.png import magma_table
        return magma_table()


def ref_pixels(x, divisor=1.0, magma=False):
    """render_video.py:35-46 save_image: clip to [0,1], * 255, astype(uint8), the colour map, the even crop; NaN -> 0; the divisor applied first in float32"""
    x = x[..., 0] if x.ndim == 3 and x.shape[2] == 1 else x
    if x.dtype == np.uint8:
        q = x
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            v = x.astype(np.float32) / np.float32(divisor)
        v[np.isnan(v)] = 0.0
        q = (np.clip(v, 0.0, 1.0) * 255).astype(np.uint8)
    if magma:
        q = magma_rgb()[q]
    h, w = q.shape[:2]
    return q[:h - h % 2, :w - w % 2]


def ref_filtered(px):
    """PNG filter type 1 on every row: the type byte, then each byte minus the byte one pixel to its left (mod 256)"""
    a = px[..., None] if px.ndim == 2 else px
    d = a.astype(np.int32)
    d[:, 1:] -= a[:, :-1].astype(np.int32)
    rows = np.concatenate([np.ones((a.shape[0], 1), np.uint8), (d % 256).astype(np.uint8).reshape(a.shape[0], -1)], 1)
    return rows.tobytes()


def parse(data):
    """-> (width, height, colour type, IDAT payload); signature, chunk order and every CRC-32 checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    chunks, o = [], 8
    while o < len(data):
        (n,), tag = struct.unpack_from(">I", data, o), data[o + 4:o + 8]
        payload = data[o + 8:o + 8 + n]
        assert struct.unpack_from(">I", data, o + 8 + n)[0] == zlib.crc32(tag + payload) & 0xFFFFFFFF, tag
        chunks.append((tag, payload))
        o += 12 + n
    assert o == len(data) and [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    return w, h, ctype, chunks[1][1]


def decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def check_file(data, px):
    """the file decodes (PIL) to exactly px, its IDAT inflates to the filtered rows of px, and it respects the size bound; returns len(IDAT)"""
    w, h, ctype, idat = parse(data)
    assert (h, w) == px.shape[:2] and ctype == (0 if px.ndim == 2 else 2)
    raw = ref_filtered(px)
    assert zlib.decompress(idat) == raw
    np.testing.assert_array_equal(decode(data), px)
    assert len(idat) <= len(raw) + 5 * ((len(raw) + SEG - 1) // SEG) + 6 <= len(raw) + 9 * ((len(raw) + SEG - 1) // SEG) + 6
    return len(idat)


# ---- contents
def contents(H, W, C, seed):
    """six images (H, W, C) float32 with their divisors: constant, uniform noise, a ramp, piecewise constant with NaN / +-inf / negatives / values above 1,
    emission on the quantisation boundaries k / 25.5 -+ 1 ulp under divisor 10, and low-amplitude noise on a ramp"""
    rng = np.random.default_rng(seed)
    n = H * W * C
    const = np.full((H, W, C), 0.7312, np.float32)
    noise = rng.random((H, W, C), dtype=np.float32)
    ramp = ((np.arange(n, dtype=np.float32) % 1021) / np.float32(1020)).reshape(H, W, C)
    piece = np.repeat(rng.choice(np.array([np.nan, np.inf, -np.inf, -0.5, -0.0, 0.0, 0.25, 0.5, 1.0, 1.5, 300.0, 1e-45], np.float32), (n + 6) // 7), 7)[:n].reshape(H, W, C)
    k = rng.integers(0, 257, n)
    edge = (k / 25.5).astype(np.float32)                                   # edge / 10 * 255 lands on, just below or just above the integer k
    step = rng.integers(-1, 2, n)
    edge = np.where(step < 0, np.nextafter(edge, np.float32(-1)), np.where(step > 0, np.nextafter(edge, np.float32(100)), edge)).astype(np.float32).reshape(H, W, C)
    soft = (ramp * np.float32(0.5) + rng.random((H, W, C), dtype=np.float32) * np.float32(0.004)).astype(np.float32)
    return [const, noise, ramp, piece, edge, soft], [1.0, 1.0, 1.0, 1.0, 10.0, 1.0]


# (64,85,3) and (64,86,3) were chosen as "exactly one segment, 64 * 256 B" and "one byte-row past it"; that count leaves out the crop to even width: they
# filter to 64 * 253 = 16192 and 64 * 259 = 16576 bytes, one segment and two.  With even height and width the filtered size H2 * (1 + W2 * channels) is an
# even number times an odd one and can never be 16384; (2,8190,1) and (2,8192,1) come as close as it gets: 16382 and 16386 bytes.
SHAPES = [((2, 2, 1), False), ((2, 2, 3), False), ((3, 5, 3), False), ((64, 85, 3), False), ((64, 86, 3), False), ((130, 200, 3), False), ((130, 200, 1), True),
          ((2, 8190, 1), False), ((2, 8192, 1), False)]


@pytest.mark.parametrize("shape,magma", SHAPES, ids=["%dx%dx%d%s" % (*s, "_magma" if m else "") for s, m in SHAPES])
def test_round_trip_is_exact(shape, magma):
    """M = 6 images of different content in ONE call; (64,85,3) filters to one segment, (64,86,3) to two, (2,8190,1) and (2,8192,1) to two bytes less and two
    bytes more than a segment, (130,200,3) to five segments with a partial last one; (3,5,3) crops to (2,4)"""
    from iris_amd.utils import png
    H, W, C = shape
    images, divisors = contents(H, W, C, seed=H * 1000 + W * 10 + C)
    dev = [torch.from_numpy(a).to(DEV) for a in images]
    files = png.encode_frames_device(dev, divisors, [magma] * 6)
    assert len(files) == 6
    sizes = []
    for a, d, data in zip(images, divisors, files):
        px = ref_pixels(a, d, magma)
        assert px.shape[:2] == (H - H % 2, W - W % 2) and (px.ndim == 3) == (C == 3 or magma)
        sizes.append(check_file(data, px))
    raw = (H - H % 2) * (1 + (W - W % 2) * (3 if magma else C))
    assert raw == {(64, 85, 3): 16192, (64, 86, 3): 16576, (2, 8190, 1): SEG - 2, (2, 8192, 1): SEG + 2, (130, 200, 3): 4 * SEG + 12594}.get(shape, raw)
    if raw >= SEG:
        assert sizes[0] < raw // 50                                         # a constant: runs of zeros after the filter, matches of 258
        if not magma:                                                       # (through the colour map a pixel's three bytes carry 8 bits: that does compress)
            assert raw < sizes[1] <= raw + 5 * ((raw + SEG - 1) // SEG) + 6  # uniform noise: stored blocks
    # determinism: a second call gives the same bytes
    assert png.encode_frames_device(dev, divisors, [magma] * 6) == files
    # the host arm decodes to the same pixels
    for a, d, data in zip(images, divisors, files):
        host = png.encode_png_host(png.quantize_host(a, d, magma))
        np.testing.assert_array_equal(decode(host), decode(data))


def test_uint8_input_mixed_sizes_and_more_images_than_one_launch_takes():
    """uint8 maps skip the quantiser; one call may mix sizes, channel counts and magma flags (a launch per group); 19 equal images need two launches of 16"""
    from iris_amd.utils import png
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((7, 9, 3), (7, 9), (7, 9, 1), (40, 33, 3), (7, 9, 3))]
    flags = [False, True, False, False, False]
    floats = [rng.random((7, 9, 3), dtype=np.float32), rng.random((7, 9), dtype=np.float32)]
    files = png.encode_frames_device([torch.from_numpy(a).to(DEV) for a in imgs + floats], None, flags + [False, True])
    for a, m, data in zip(imgs + floats, flags + [False, True], files):
        check_file(data, ref_pixels(a, 1.0, m))
    many = [rng.random((4, 6), dtype=np.float32) * np.float32(k % 3 + 0.5) for k in range(19)]
    files = png.encode_frames_device([torch.from_numpy(a).to(DEV) for a in many])
    for a, data in zip(many, files):
        check_file(data, ref_pixels(a))
    # a non-contiguous view is taken as the image it shows
    base = torch.from_numpy(rng.random((10, 12, 3), dtype=np.float32)).to(DEV)
    (data,) = png.encode_frames_device([base[1:9, 2:10]])
    check_file(data, ref_pixels(base[1:9, 2:10].cpu().numpy()))


def test_refusals():
    from iris_amd._lib import IrisError
    from iris_amd.utils import png
    with pytest.raises(IrisError, match="empty"):
        png.encode_frames_device([torch.zeros(1, 7, 3, device=DEV)])                       # cropped height 0
    with pytest.raises(IrisError, match="empty"):
        png.encode_frames_device([torch.zeros(6, 1, device=DEV)])
    with pytest.raises(IrisError, match="magma"):
        png.encode_frames_device([torch.zeros(4, 4, 3, device=DEV)], None, [True])
    with pytest.raises(IrisError):
        png.encode_frames_device([torch.zeros(4, 4, 2, device=DEV)])
    with pytest.raises(IrisError):
        png.encode_frames_device([torch.zeros(4, 4, 3)])                                   # a host tensor: there is no CPU path
    with pytest.raises(IrisError):
        png.encode_frames_device([torch.zeros(4, 4, 3, device=DEV)], [0.0])
    with pytest.raises(IrisError):
        png.encode_frames_device([torch.zeros(4, 4, 3, device=DEV, dtype=torch.float64)])


# ---- the stage
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """A scene in the `real` layout around the render fixture's room at 12 x 16: mesh, one (validation) camera, a three-frame trajectory, the emitter files, a
    checkpoint holding the response model, a light file for the relighting stage."""
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils.exr import write_exr
    from test_render import setup, write_emitter_files
    f, scene, em = setup()
    H, W = 12, 16
    root = tmp_path_factory.mktemp("video")
    data, bake, ckpt_dir = root / "data", root / "bake", root / "ckpt" / "exp"
    for d in (data / "Image", bake, ckpt_dir):
        d.mkdir(parents=True)
    with open(data / "scene.obj", "w") as fh:
        fh.writelines("v {:.9g} {:.9g} {:.9g}\n".format(*v) for v in f["verts"].tolist())
        fh.writelines("f {} {} {}\n".format(*(i + 1 for i in t)) for t in f["faces"].tolist())
    write_exr(str(data / "Image" / "000_0001.exr"), np.zeros((H, W, 3), np.float32))
    c2w = np.asarray(f["c2w"], np.float64).reshape(-1)[:12].reshape(3, 4)
    origin, right, down, fwd = c2w[:, 3], c2w[:, 0], c2w[:, 1], c2w[:, 2]
    row = lambda v: " ".join(repr(float(x)) for x in v)     # noqa: E731
    with open(data / "cam.txt", "w") as fh:
        fh.write("\n".join(["1", row(origin), row(origin + fwd), row(-down)]))
    s = W / float(f["W"])
    K = np.array([[float(f["K"][0, 0]) * s, 0, W / 2], [0, float(f["K"][1, 1]) * s, H / 2], [0, 0, 1]])
    with open(data / "K_list.txt", "w") as fh:
        fh.write("\n".join(["1"] + [row(r) for r in K]))
    traj = np.stack([np.concatenate([c2w[:, :3], (origin + 0.05 * k * right)[:, None]], 1) for k in range(3)])
    np.save(data / "render_traj.npy", traj)
    write_emitter_files(f, str(bake), "vslf_0.npz")
    write_emitter_files(f, str(bake), "vslf.npz")
    t = torch.linspace(0, 1, 1024)
    crf = EmorCRF.from_arrays(t ** 0.45, torch.stack([torch.sin(3.14159 * t * (k + 1)) * 0.05 for k in range(3)]))
    torch.save({"state_dict": {"model_crf." + k: v for k, v in crf.state_dict().items()}}, ckpt_dir / "last.ckpt")
    p = origin + 0.8 * fwd
    with open(data / "relight.json", "w") as fh:
        json.dump({"type": "scene", "panel": {"type": "rectangle", "to_world": [{"type": "translate", "value": p.tolist()}, {"type": "scale", "value": [0.2, 0.2, 0.2]}],
                                              "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [6, 6, 6]}}}}, fh)
    return {"root": root, "data": data, "bake": bake, "hw": (H, W), "traj": traj.astype(np.float32), "K": K.astype(np.float32), "crf": crf, "scene": scene, "em": em}


def _common(tree, out):
    return ["--experiment_name", "exp", "--checkpoint_path", str(tree["root"] / "ckpt"), "--ckpt", "last.ckpt", "--dataset", "real", str(tree["data"]), "--emitter_path",
            str(tree["bake"]), "--output_path", str(out), "--split", "val", "--SPP", "2", "--spp", "1", "--crf_basis", "3", "--material", "stub_material:material", "--seed", "3"]


def test_frame_writer_host_and_device_arms_on_one_render(tree):
    """render_video's frame writer on ONE render_view output (12 x 16 px, SPP 2, spp 1) as three frames: 24 files and 8 lists, even sizes, the host and the
    device encoder decode to the same pixels -- the reference's save_image of the maps in `out`"""
    from iris_amd import render_video as RV
    from iris_amd.render import render_view
    from iris_amd.utils import cameras
    from stub_material import StubMaterial
    H, W = tree["hw"]
    img_hw, views = cameras.load_trajectory("real", str(tree["data"]), "", 1.0, split="val")
    assert img_hw == (H, W) and len(views) == 3 and np.array_equal(views[0]["K"], tree["K"]) and np.array_equal(views[2]["c2w"], tree["traj"][2])
    rays = cameras.view_rays(views[1], img_hw, torch.device(DEV), ray_diff=True)
    torch.manual_seed(5); torch.cuda.manual_seed(5)
    out = render_view(tree["scene"], tree["em"], StubMaterial(), tree["crf"].to(DEV), rays, img_hw, 2, 1, 2, exposure=1.0, gt=None)
    want = [ref_pixels(out[key].cpu().numpy(), d, m) for _, _, key, d, m in RV.FRAME_FILES]
    assert any(w.max() > 0 for w in want)
    roots = {}
    for enc in ("device", "host"):
        roots[enc] = tree["root"] / ("frames_" + enc)
        writer = RV.FrameWriter(torch.device(DEV), enc)
        paths = [writer.submit(str(roots[enc]), i, out) for i in range(3)]
        writer.close()
        lists = RV.write_lists(str(roots[enc]), 3)
        assert len({p for ps in paths for p in ps}) == 24 and all(os.path.isfile(p) for ps in paths for p in ps) and len(lists) == 8 and all(os.path.isfile(p) for p in lists)
        assert not [n for _, _, names in os.walk(roots[enc]) for n in names if n.endswith(".part")]
        for ps in paths:
            for p, w in zip(ps, want):
                px = decode(open(p, "rb").read())
                assert px.shape[0] % 2 == 0 and px.shape[1] % 2 == 0
                np.testing.assert_array_equal(px, w, err_msg=p)
        text = open(lists[4]).read().splitlines()
        assert [l for l in text if l.startswith("file ")] == ["file 'roughness/%05d_roughness_color.png'" % i for i in (0, 1, 2, 2, 1, 0)]
    from iris_amd._lib import IrisError
    with pytest.raises(IrisError, match="'host' or 'device'"):
        RV.FrameWriter(torch.device(DEV), "pil")


def test_render_video_cli(tree):
    """python -m iris_amd.render_video on the tree: the reference's eight files per trajectory frame and the eight lists; frame 1 is render_view under the CLI's seed"""
    from iris_amd import render_video as RV
    from iris_amd._lib import IrisError
    from iris_amd.render import render_view
    from iris_amd.utils import cameras
    from stub_material import StubMaterial
    out = tree["root"] / "video"
    RV.main(_common(tree, out) + ["--indir_depth", "2", "--ldr_img_dir", "Image", "--batch_size", "8"])
    for i in range(3):
        assert all(os.path.isfile(p) for p in RV.frame_paths(str(out), i))
    assert sorted(n for n in os.listdir(out) if n.endswith(".ffconcat")) == sorted(name + ".ffconcat" for _, name, _, _, _ in RV.FRAME_FILES)
    H, W = tree["hw"]
    _, views = cameras.load_trajectory("real", str(tree["data"]), "", 1.0, split="val")
    rays = cameras.view_rays(views[1], (H, W), torch.device(DEV), ray_diff=True)
    torch.manual_seed(3 * 1000003 + 1); torch.cuda.manual_seed(3 * 1000003 + 1)
    from iris_amd.utils import stage
    ref = render_view(tree["scene"], tree["em"], StubMaterial(), tree["crf"].to(DEV), rays, (H, W), 2, 1, 2, exposure=1.0, gt=None, denoiser=stage.make_denoiser("atrous", (H, W), torch.device(DEV)))
    for p, (_, _, key, d, m) in zip(RV.frame_paths(str(out), 1), RV.FRAME_FILES):
        np.testing.assert_array_equal(decode(open(p, "rb").read()), ref_pixels(ref[key].cpu().numpy(), d, m), err_msg=p)
    with pytest.raises(IrisError, match="area"):
        RV.main(_common(tree, out) + ["--light_type", "area"])
    RV.main(_common(tree, tree["root"] / "video_host") + ["--indir_depth", "2", "--png_encoder", "host", "--max_views", "1"])
    for a, b in zip(RV.frame_paths(str(out), 0), RV.frame_paths(str(tree["root"] / "video_host"), 0)):
        np.testing.assert_array_equal(decode(open(a, "rb").read()), decode(open(b, "rb").read()))
    assert not os.path.exists(RV.frame_paths(str(tree["root"] / "video_host"), 1)[0])


def test_render_relight_takes_the_trajectory(tree):
    """render_relight --mode traj without --cameras: one frame per trajectory frame and relight.ffconcat"""
    from iris_amd import render_relight as RR
    out = tree["root"] / "relight"
    RR.main(_common(tree, out) + ["--mode", "traj", "--light_cfg", str(tree["data"] / "relight.json"), "--indir_depth", "1", "--sphere_subdiv", "0"])
    H, W = tree["hw"]
    for i in range(3):
        assert os.path.isfile(out / ("%05d_rgb.exr" % i))
        px = decode(open(out / ("%05d_rgb.png" % i), "rb").read())
        assert px.shape == (H, W, 3) and px.dtype == np.uint8
    text = open(out / "relight.ffconcat").read().splitlines()
    assert text[0] == "ffconcat version 1.0"
    assert [l for l in text if l.startswith("file ")] == ["file '%05d_rgb.png'" % i for i in (0, 1, 2, 2, 1, 0)]
    assert len([l for l in text if l.startswith("duration ")]) == 6
