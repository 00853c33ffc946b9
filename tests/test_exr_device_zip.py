"""Device-side deflate of the EXR writer (utils/exr.zip_encode_torch, csrc/iris_deflate.h): every chunk is a zlib stream of its predicted block or
the raw block, as OpenEXR's ZIP rule wants; the files decode bit for bit; sizes against host zlib's Z_RLE parse; the CLIs with --exr_encoder device
write the same pixels as with the host encoder."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from test_exr_conformance import parse_exr


def _maps(H, W, seed=0):
    """(M, H, W, 3) float32: Gaussian noise at several scales, a constant, zeros, half-masked rows, special bit patterns"""
    rng = np.random.default_rng(seed)
    noise = lambda s: np.abs(rng.standard_normal((H, W, 3))).astype(np.float32) * np.float32(s)      # noqa: E731
    masked = noise(1.0)
    masked[:, : (W + 1) // 2] = 0.0
    masked[1::3] = 0.0
    special = noise(2.0).view(np.uint32)
    pats = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x00400000, 0x80000000], np.uint32)
    sel = rng.random((H, W, 3)) < 0.3
    special[sel] = pats[rng.integers(0, len(pats), int(sel.sum()))]
    maps = [noise(1e-3), noise(1.0), noise(1e3), np.full((H, W, 3), 0.5, np.float32), np.zeros((H, W, 3), np.float32), masked, special.view(np.float32)]
    return np.stack(maps)


def _encode(maps, comp):
    from iris_amd.utils import exr
    dev = torch.device("cuda:0")
    full, tail = exr.scanline_blocks_torch(torch.from_numpy(maps).to(dev), comp)
    rec, offs = exr.zip_encode_torch(full, tail, comp)
    torch.cuda.synchronize()
    return full.cpu().numpy(), tail.cpu().numpy(), rec.cpu().numpy(), offs.cpu().numpy()


def _records(buf):
    """back-to-back (y, size, data) records -> [(y, data)]"""
    out, o, buf = [], 0, bytes(buf)
    while o < len(buf):
        y, size = struct.unpack_from("<ii", buf, o)
        out.append((y, buf[o + 8:o + 8 + size]))
        o += 8 + size
    assert o == len(buf)
    return out


def _zrle(pred):
    c = zlib.compressobj(4, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(pred) + c.flush()


def _blocks(full, tail, m):
    return [full[m, i].tobytes() for i in range(full.shape[1])] + ([tail[m].tobytes()] if tail.shape[1] else [])


@pytest.mark.gpu
@pytest.mark.parametrize("comp", ["zip", "zips"])
@pytest.mark.parametrize("hw", [(37, 1), (37, 7), (37, 1920)])
def test_every_chunk_is_a_zlib_stream_of_its_predicted_block_or_the_raw_block(comp, hw):
    from iris_amd.utils import exr
    H, W = hw
    maps = _maps(H, W, seed=W)
    full, tail, rec, offs = _encode(maps, comp)
    lines = 16 if comp == "zip" else 1
    assert offs[0] == 0 and offs[-1] <= rec.shape[0] and np.all(np.diff(offs) > 0)
    n_raw = n_z = 0
    for m in range(maps.shape[0]):
        chunks = _records(rec[offs[m]:offs[m + 1]])
        preds = _blocks(full, tail, m)
        assert [y for y, _ in chunks] == [i * lines for i in range(len(preds))]
        for (y, data), pred in zip(chunks, preds):
            if len(data) == len(pred):
                n_raw += 1
                assert data == exr._unpredict(pred)                     # the raw block bytes
                assert len(_zrle(pred)) >= 0.95 * len(pred) - 64, (m, y)  # raw only where a distance-1 deflate would not shrink it much either
            else:
                n_z += 1
                assert len(data) < len(pred)
                d = zlib.decompressobj()
                assert d.decompress(data) == pred and d.eof and d.unused_data == b"", (m, y)
    assert n_z > 0 or full.shape[-1] <= 12                                # (a 12-byte ZIPS block of W = 1 never shrinks)
    assert n_raw > 0 or W > 7


@pytest.mark.gpu
@pytest.mark.parametrize("comp", ["zip", "zips"])
def test_device_written_files_decode_bit_for_bit(tmp_path, comp):
    from iris_amd.utils import exr
    for H, W in ((37, 7), (21, 53), (19, 1920)):
        maps = _maps(H, W, seed=H + W)
        _, _, rec, offs = _encode(maps, comp)
        for m in range(maps.shape[0]):
            p = str(tmp_path / f"m{m}_{W}.exr")
            exr.write_exr_records(p, H, W, comp, rec[offs[m]:offs[m + 1]])
            np.testing.assert_array_equal(exr.read_exr(p).view(np.uint32), maps[m].view(np.uint32))
            if W <= 53:                                               # (parse_exr un-predicts in Python, byte by byte)
                f = parse_exr(open(p, "rb").read())
                assert f["compression"] == {"zip": 3, "zips": 2}[comp] and (f["height"], f["width"]) == (H, W)
                for ci, ch in enumerate("RGB"):
                    np.testing.assert_array_equal(f["channels"][ch].view(np.uint32), maps[m][..., ci].view(np.uint32))


@pytest.mark.gpu
def test_random_bit_patterns_are_stored_raw_as_the_host_writer_stores_them(tmp_path):
    from iris_amd.utils import exr
    H, W = 37, 1920
    rng = np.random.default_rng(5)
    maps = rng.integers(0, 2 ** 32, (2, H, W, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    for comp in ("zip", "zips"):
        full, tail, rec, offs = _encode(maps, comp)
        for m in range(2):
            for (_, data), pred in zip(_records(rec[offs[m]:offs[m + 1]]), _blocks(full, tail, m)):
                assert len(data) == len(pred)
            a, b = str(tmp_path / "dev.exr"), str(tmp_path / "host.exr")
            exr.write_exr_records(a, H, W, comp, rec[offs[m]:offs[m + 1]])
            exr.write_exr(b, maps[m], comp)
            assert open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("comp", ["zip", "zips"])
def test_size_against_host_zlib_rle(comp):
    H, W = 64, 1920
    rng = np.random.default_rng(11)
    maps = [np.abs(rng.standard_normal((H, W, 3))).astype(np.float32) * s for s in (1e-2, 1.0, 30.0)]
    masked = maps[1].copy()
    masked[:, 700:1500] = 0.0                                            # pixels without a primary hit are zero in the baked maps
    maps = np.stack(maps + [masked, np.full((H, W, 3), 1.0, np.float32)])
    full, tail, rec, offs = _encode(maps, comp)
    for m in range(maps.shape[0]):
        preds = _blocks(full, tail, m)
        ours = sum(len(d) for _, d in _records(rec[offs[m]:offs[m + 1]]))
        host = sum(min(len(_zrle(p)), len(p)) for p in preds)
        assert ours <= 1.02 * host, (m, ours, host)
        if m >= 3:
            assert ours < 0.7 * sum(len(p) for p in preds), m


@pytest.mark.gpu
def test_constant_and_zero_1080p_maps_shrink_50x():
    H, W = 1080, 1920
    uniform = np.full((H, W, 3), np.uint32(0x40404040), np.uint32).view(np.float32)    # a constant whose four bytes are equal: a run after prediction
    maps = np.stack([np.zeros((H, W, 3), np.float32), uniform])
    for comp in ("zip", "zips"):
        full, tail, rec, offs = _encode(maps, comp)
        for m in range(2):
            raw = sum(len(p) for p in _blocks(full, tail, m))
            assert (offs[m + 1] - offs[m]) * 50 <= raw, (comp, m, int(offs[m + 1] - offs[m]), raw)


@pytest.mark.gpu
def test_two_encodes_are_identical():
    from iris_amd.utils import exr
    maps = torch.from_numpy(_maps(45, 1920, seed=3)).cuda()
    for comp in ("zip", "zips"):
        full, tail = exr.scanline_blocks_torch(maps, comp)
        r1, o1 = exr.zip_encode_torch(full, tail, comp)
        r2, o2 = exr.zip_encode_torch(full, tail, comp)
        n = int(o1[-1])
        assert torch.equal(o1, o2) and torch.equal(r1[:n], r2[:n])


def test_write_exr_records_equals_write_exr_blocks(tmp_path):
    """CPU: records deflated by host zlib through write_exr_records -> the same file write_exr_blocks writes."""
    from iris_amd.utils import exr
    rng = np.random.default_rng(2)
    for comp, (H, W) in (("zip", (37, 53)), ("zips", (5, 7)), ("zip", (16, 3))):
        img = (rng.random((H, W, 3)) * 5).astype(np.float32)
        img[:, : W // 2] = 0.0
        full, tail = exr.scanline_blocks_torch(torch.from_numpy(img[None]), comp)
        full, tail = full[0].numpy(), tail[0].numpy()
        lines = 16 if comp == "zip" else 1
        parts = [full[i].tobytes() for i in range(full.shape[0])] + ([tail.tobytes()] if tail.shape[0] else [])
        recs = b""
        for i, p in enumerate(parts):
            data = exr._deflate_predicted(p)
            recs += struct.pack("<ii", i * lines, len(data)) + data
        a, b = str(tmp_path / "rec.exr"), str(tmp_path / "blk.exr")
        exr.write_exr_records(a, H, W, comp, np.frombuffer(recs, np.uint8))
        exr.write_exr_blocks(b, H, W, comp, full, tail)
        assert open(a, "rb").read() == open(b, "rb").read()
        np.testing.assert_array_equal(exr.read_exr(a), img)
    with pytest.raises(ValueError):
        exr.write_exr_records(str(tmp_path / "bad.exr"), 37, 53, "zip", np.frombuffer(recs[:-1], np.uint8))


def _tiny_scene(tmp_path):
    from iris_amd.model.slf import VoxelSLF
    from conftest import golden
    g = golden("bake_box.npz")
    p = golden("pt_single.npz")
    scene_dir = tmp_path / "scene"; scene_dir.mkdir()
    with open(scene_dir / "scene.obj", "w") as fh:
        for v in g["verts"]:
            fh.write("v {} {} {}\n".format(*v))
        for f in g["faces"]:
            fh.write("f {} {} {}\n".format(*(f + 1)))
    H, W = 20, 28
    K = np.array([[0.8 * W, 0, W / 2.0], [0, 0.8 * W, H / 2.0], [0, 0, 1]], np.float32)
    import json
    json.dump({"img_hw": [H, W], "views": [{"K": K.tolist(), "c2w": g["c2w"].tolist()}] * 2}, open(tmp_path / "cams.json", "w"))
    slf = VoxelSLF(torch.from_numpy(g["slf_mask"]), float(g["voxel_min"]), float(g["voxel_max"]))
    slf.radiance[:] = torch.from_numpy(g["slf_radiance"])
    ep, sp = str(tmp_path / "emitter.pth"), str(tmp_path / "vslf.npz")
    torch.save({"is_emitter": torch.from_numpy(g["is_emitter"]), "emitter_vertices": torch.from_numpy(p["emitter_vertices"]),
                "emitter_area": torch.from_numpy(g["emitter_area"]), "emitter_normal": torch.zeros(int(g["is_emitter"].sum()), 3),
                "emitter_radiance": torch.from_numpy(g["emitter_radiance"])}, ep)
    torch.save({"mask": torch.from_numpy(g["slf_mask"]), "voxel_min": float(g["voxel_min"]), "voxel_max": float(g["voxel_max"]), "weight": slf.state_dict()}, sp)
    return ["--scene", str(scene_dir), "--slf_path", sp, "--emitter_path", ep, "--dataset", "generic", "--cameras", str(tmp_path / "cams.json")]


@pytest.mark.gpu
def test_cli_device_encoder_writes_the_host_encoders_pixels(tmp_path):
    from iris_amd import bake_shading as bs, refine_shading as rs
    from iris_amd.utils import exr
    common = _tiny_scene(tmp_path)
    bake = ["--spp_diffuse", "8", "--spps_specular", "4", "4", "4", "4", "4", "4", "--seed", "4"]
    for comp in ("zip", "zips"):
        outs = {}
        for enc in ("host", "device"):
            outs[enc] = str(tmp_path / f"bake_{comp}_{enc}")
            bs.main(common + bake + ["--output", outs[enc], "--compression", comp, "--exr_encoder", enc])
        for im_id in (0, 1):
            for fh, fd in zip(bs.output_files(outs["host"], im_id), bs.output_files(outs["device"], im_id)):
                assert exr.read_exr_header(fd)["compression"] == {"zip": 3, "zips": 2}[comp]
                np.testing.assert_array_equal(exr.read_exr(fd).view(np.uint32), exr.read_exr(fh).view(np.uint32))
    refine = ["--material", "stub_material:material", "--spp_diffuse", "4", "--spp_specular", "4", "--indir_depth", "2", "--seed", "2"]
    outs = {}
    for enc in ("host", "device"):
        outs[enc] = str(tmp_path / f"refine_{enc}")
        rs.main(common + refine + ["--output", outs[enc], "--exr_encoder", enc])
    for fh, fd in zip(bs.output_files(outs["host"], 0), bs.output_files(outs["device"], 0)):
        assert os.path.exists(fd)
        np.testing.assert_array_equal(exr.read_exr(fd).view(np.uint32), exr.read_exr(fh).view(np.uint32))
