"""iris_amd/utils/avi.py: the Motion-JPEG AVI container, checked by a RIFF walker written here.  The frames are JPEG files made by Pillow, so that nothing here
depends on the project's own encoder."""
import io
import os
import struct

import numpy as np
import pytest

W, H, FPS = 20, 12, 30


def pil_jpeg(seed, quality):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)).save(out, "JPEG", quality=quality)
    return out.getvalue()


def frames(n):
    """n different JPEG files, at least one of odd and one of even length"""
    fs = [pil_jpeg(k, 60 + k) for k in range(n)]
    k = n
    while len({len(f) % 2 for f in fs}) < 2 and n > 1:
        fs[-1] = pil_jpeg(k, 50)
        k += 1
    if n == 1 and len(fs[0]) % 2 == 0:
        fs[0] += b"\0"                                      # (bytes after EOI are ignored by decoders: an odd-length frame)
    return fs


def chunks(data, start, end):
    """the chunks between start and end as (fourcc, list type or None, offset of the chunk, offset of its data, size); a chunk is padded to even length"""
    out, o = [], start
    while o < end:
        fourcc, size = data[o:o + 4], struct.unpack_from("<I", data, o + 4)[0]
        assert o + 8 + size <= end, (fourcc, o, size, end)
        out.append((fourcc, data[o + 8:o + 12] if fourcc in (b"RIFF", b"LIST") else None, o, o + 8, size))
        o += 8 + size + size % 2
    assert o == end or o == end + 1
    return out


def walk(data):
    """-> dict of the file's parts; every size field is held to the bytes it spans"""
    (riff,) = chunks(data, 0, len(data))
    assert riff[0] == b"RIFF" and riff[1] == b"AVI " and riff[4] == len(data) - 8
    top = chunks(data, 12, len(data))
    assert [(c[0], c[1]) for c in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl, movi, idx1 = top
    inner = chunks(data, hdrl[3] + 4, hdrl[3] + hdrl[4])
    assert [(c[0], c[1]) for c in inner] == [(b"avih", None), (b"LIST", b"strl")] and inner[0][4] == 56
    strl = chunks(data, inner[1][3] + 4, inner[1][3] + inner[1][4])
    assert [c[0] for c in strl] == [b"strh", b"strf"] and (strl[0][4], strl[1][4]) == (56, 40)
    frames_ = chunks(data, movi[3] + 4, movi[3] + movi[4])
    assert all(c[0] == b"00dc" for c in frames_)
    assert idx1[4] == 16 * len(frames_) and idx1[3] + idx1[4] == len(data)
    index = [struct.unpack_from("<4sIII", data, idx1[3] + 16 * k) for k in range(len(frames_))]
    return dict(avih=struct.unpack_from("<14I", data, inner[0][3]), strh=struct.unpack_from("<4s4sIHHIIIIIIiI4H", data, strl[0][3]),
                strf=struct.unpack_from("<IiiHH4sIiiII", data, strl[1][3]), movi=movi[3], frames=frames_, index=index)


@pytest.mark.parametrize("n", [1, 3])
def test_container(n, tmp_path):
    from PIL import Image
    from iris_amd.utils.avi import AviWriter
    fs = frames(n)
    assert any(len(f) % 2 for f in fs)
    path = str(tmp_path / "v.avi")
    w = AviWriter(path, W, H, FPS)
    for f in fs:
        w.add_frame(f)
    assert os.path.exists(path + ".part") and not os.path.exists(path)
    w.close(reverse=True)
    assert os.listdir(tmp_path) == ["v.avi"]
    data = open(path, "rb").read()
    p = walk(data)
    want = fs + fs[::-1]
    assert len(p["frames"]) == 2 * n
    for (fourcc, _, at, start, size), f, (ckid, flags, off, length) in zip(p["frames"], want, p["index"]):
        assert data[start:start + size] == f
        assert at % 2 == 0 and (size % 2 == 0 or data[start + size] == 0)               # padded to even length, with a zero
        assert (ckid, flags, length) == (b"00dc", 0x10, size) and p["movi"] + off == at   # key frame; offset from the 'movi' fourcc to the chunk's header
        im = Image.open(io.BytesIO(data[start:start + size]))
        im.load()
        assert im.size == (W, H)
    usec, _, _, flags, total, _, streams, buf, width, height = p["avih"][:10]
    assert (usec, flags & 0x10, total, streams, width, height) == (1000000 // FPS, 0x10, 2 * n, 1, W, H) and buf >= max(len(f) for f in fs)
    strh = p["strh"]
    assert strh[:2] == (b"vids", b"MJPG") and strh[6:8] == (1, FPS) and strh[9] == 2 * n and strh[-4:] == (0, 0, W, H)
    size, width, height, planes, bits, comp = p["strf"][:6]
    assert (size, width, height, planes, bits, comp) == (40, W, H, 1, 24, b"MJPG")
    # forward only
    w = AviWriter(path, W, H, FPS)
    for f in fs:
        w.add_frame(f)
    w.close(reverse=False)
    p = walk(open(path, "rb").read())
    assert len(p["frames"]) == n and p["avih"][4] == n and os.listdir(tmp_path) == ["v.avi"]


def test_a_file_past_two_gigabytes_is_refused(tmp_path):
    """the size accounting is fed lengths; nothing of that size is written"""
    from iris_amd._lib import IrisError
    from iris_amd.utils.avi import AviWriter
    w = AviWriter(str(tmp_path / "a.avi"), W, H, FPS)
    w._reserve(2 ** 30)
    with pytest.raises(IrisError, match="OpenDML"):
        w._reserve(2 ** 30)                                  # forward: 2 GiB and the headers
    w.fh.close()
    w = AviWriter(str(tmp_path / "b.avi"), W, H, FPS)
    w.add_frame(pil_jpeg(0, 80))
    w._reserve(2 ** 30 + 2 ** 20)                            # fits forward, not twice
    with pytest.raises(IrisError, match="OpenDML"):
        w.close(reverse=True)
    assert not os.path.exists(str(tmp_path / "b.avi")) and not os.path.exists(str(tmp_path / "b.avi.part"))
    w = AviWriter(str(tmp_path / "c.avi"), W, H, FPS)
    for length in (2 ** 31 - 1 - 224 - 8 - 16 - 8, ):        # the largest single even-length frame that fits: headers 224, idx1 8 + 16, chunk header 8
        w._reserve(length - length % 2)
    with pytest.raises(IrisError):
        w._reserve(2)
    w.fh.close()
    with pytest.raises(IrisError):
        AviWriter(str(tmp_path / "d.avi"), 0, H, FPS)
