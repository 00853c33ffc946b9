"""Baseline JPEG files for the video stage's Motion-JPEG .avi files (render_video --video mjpeg): the headers on the host, the entropy-coded data on the device.

    device  enqueue_frames_device: iris_jpeg_encode per group of equal-size images (iris_amd/csrc/iris_jpeg.h: the PNG path's quantiser, MAGMA table and even
            crop, integer Y Cb Cr 4:2:0, integer DCT, the Annex K tables, one restart interval per MCU row).  The streams lie dense at the start of a buffer
            sized for the worst case, which is many times the raw image: the host copies the offsets (a few bytes), then exactly the used bytes.
    host    jpeg_headers(width, height, quality): SOI, APP0 JFIF 1.01, two DQT, SOF0, four DHT, DRI, SOS -- a function of its three arguments alone

The contract of a frame is DESIGN.md 5c-14; tests/jpeg_ref.py restates it in numpy.  The tables come from the library (iris_jpeg_tables), so the headers
cannot disagree with the kernels about them.
"""
import ctypes as C

import numpy as np

EOI = b"\xff\xd9"
_tables = None


def _check_quality(quality):
    from .. import _lib as L
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise L.IrisError(f"jpeg: the quality {quality!r} is not an integer in 1..100")
    return int(quality)


def tables():
    """-> dict: quant (2, 64) the Annex K tables in natural order, zigzag (64,) the natural index of each zigzag position, dht: four (class << 4 | id, BITS,
    HUFFVAL) in the order the headers write them"""
    global _tables
    if _tables is None:
        from .. import _lib as L
        buf = (C.c_uint8 * 604)()
        L.lib().iris_jpeg_tables(buf)
        raw = bytes(buf)
        dht, o = [], 192
        for ident, n in ((0x00, 12), (0x10, 162), (0x01, 12), (0x11, 162)):
            dht.append((ident, raw[o:o + 16], raw[o + 16:o + 16 + n]))
            o += 16 + n
        _tables = dict(quant=np.frombuffer(raw[:128], np.uint8).reshape(2, 64).astype(np.int64), zigzag=np.frombuffer(raw[128:192], np.uint8).astype(np.int64), dht=dht)
    return _tables


def quant_tables(quality):
    """the luma and the chroma table at `quality`, natural (row-major) order, as two lists of 64: Annex K scaled by the IJG rule -- s = 5000 / q below 50,
    200 - 2 q from 50; entry (base * s + 50) / 100 clamped to 1..255"""
    q = _check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return [[int(v) for v in row] for row in np.clip((tables()["quant"] * s + 50) // 100, 1, 255)]


def _segment(marker, payload):
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def jpeg_headers(width, height, quality):
    """everything in front of the entropy-coded data of a (height, width) frame"""
    from .. import _lib as L
    if not (0 < width <= 65535 and 0 < height <= 65535):
        raise L.IrisError(f"jpeg_headers: {width} x {height}: a side is 1..65535")
    t, qt = tables(), np.asarray(quant_tables(quality))
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")                      # 1.01, no units, aspect 1:1, no thumbnail
    for k in (0, 1):
        out += _segment(0xDB, bytes((k,)) + bytes(qt[k][t["zigzag"]].tolist()))
    # 8 bit; Y: 2 x 2, table 0; Cb, Cr: 1 x 1, table 1
    out += _segment(0xC0, bytes((8,)) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes((3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for ident, bits, vals in t["dht"]:
        out += _segment(0xC4, bytes((ident,)) + bits + vals)
    out += _segment(0xDD, ((width + 15) // 16).to_bytes(2, "big"))                                               # one restart interval per MCU row
    return out + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def enqueue_frames_device(images, divisors=None, magma=None, quality=90):
    """The device part of encode_frames_device, enqueued on the current stream: -> (buf, layout).  buf: ONE device uint8 tensor holding, first, every group's
    stream offsets (int64; layout["head"] bytes) and then every group's streams, dense from the group's position, in room for the worst case.  layout["groups"]:
    per group (indices of its images, width, height, position of its offsets in int64 units, position of its streams in bytes) for streams_from_host."""
    import torch
    from .. import _lib as L
    n = len(images)
    quality = _check_quality(quality)
    divisors = [1.0] * n if divisors is None else [float(d) for d in divisors]
    magma = [False] * n if magma is None else [bool(m) for m in magma]
    if n == 0 or len(divisors) != n or len(magma) != n:
        raise L.IrisError("encode_frames_device: one divisor and one magma flag per image, at least one image")
    lib, groups, tensors = L.lib(), {}, []
    for i, t in enumerate(images):
        if not torch.is_tensor(t) or t.dtype not in (torch.float32, torch.uint8):
            raise L.IrisError(f"encode_frames_device: image {i}: expected a float32 or uint8 tensor on a HIP device")
        t = L.require_gpu(t, t.dtype, f"image {i}")
        t = t[..., None] if t.dim() == 2 else t
        if t.dim() != 3 or t.shape[2] not in (1, 3):
            raise L.IrisError(f"encode_frames_device: image {i}: expected (H, W), (H, W, 1) or (H, W, 3), got {tuple(t.shape)}")
        if magma[i] and t.shape[2] != 1:
            raise L.IrisError(f"encode_frames_device: image {i}: a magma image has one channel, this one has {t.shape[2]}")
        if not (divisors[i] > 0.0 and divisors[i] < float("inf")):
            raise L.IrisError(f"encode_frames_device: image {i}: the divisor {divisors[i]} is not positive and finite")
        H, W, ch = (int(s) for s in t.shape)
        if H - H % 2 == 0 or W - W % 2 == 0:
            raise L.IrisError(f"encode_frames_device: image {i}: a {H} x {W} image cropped to even height and width is empty")
        if int(lib.iris_jpeg_stream_bound(H, W)) == 0:
            raise L.IrisError(f"encode_frames_device: image {i}: unsupported size {H} x {W}")
        tensors.append(t)
        groups.setdefault((H, W, ch, t.dtype), []).append(i)
    dev = tensors[0].device
    if any(t.device != dev for t in tensors):
        raise L.IrisError("encode_frames_device: the images lie on different devices")
    layout, n_off, n_bytes = [], 0, 0
    for (H, W, ch, dtype), idx in groups.items():
        layout.append(dict(indices=idx, width=W - W % 2, height=H - H % 2, off=n_off, pos=n_bytes, shape=(H, W, ch), u8=dtype == torch.uint8))
        n_off += len(idx) + 1
        n_bytes += (len(idx) * int(lib.iris_jpeg_stream_bound(H, W)) + 255) // 256 * 256
    head = (8 * n_off + 255) // 256 * 256
    buf = torch.empty(head + n_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for g in layout:
            M, (H, W, ch) = len(g["indices"]), g["shape"]
            g["pos"] += head
            ws_bytes = int(lib.iris_jpeg_workspace_bytes(M, H, W))
            if ws_bytes == 0:
                raise L.IrisError(f"encode_frames_device: unsupported size ({M} images of {H} x {W})")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            ptrs = (C.c_void_p * M)(*[tensors[i].data_ptr() for i in g["indices"]])
            divs = (C.c_float * M)(*[divisors[i] for i in g["indices"]])
            flags = (C.c_uint8 * M)(*[int(magma[i]) for i in g["indices"]])
            L.mark()
            L.check(lib.iris_jpeg_encode(ptrs, divs, flags, M, H, W, ch, int(g["u8"]), quality, C.c_void_p(buf.data_ptr() + g["pos"]),
                                         C.c_void_p(buf.data_ptr() + 8 * g["off"]), L.ptr(ws), ws_bytes, L.stream()))
            L.mark("jpeg encode")
    return buf, dict(head=head, quality=quality, groups=[{k: g[k] for k in ("indices", "width", "height", "off", "pos")} for g in layout])


def group_sizes(head, layout):
    """head: the first layout["head"] bytes of buf on the host (a uint8 numpy array) -> per group the bytes its streams occupy from its position"""
    from .. import _lib as L
    sizes = []
    for g in layout["groups"]:
        M = len(g["indices"])
        offs = np.asarray(head, np.uint8)[8 * g["off"]:8 * (g["off"] + M + 1)].view(np.int64)
        if offs[0] != 0 or (np.diff(offs) <= 0).any():
            raise L.IrisError("jpeg: the stream offsets are not what iris_jpeg_encode writes (was the copy complete?)")
        sizes.append(int(offs[M]))
    return sizes


def streams_from_host(head, data, layout, n):
    """head as for group_sizes; data: per group the group_sizes() bytes from its position, on the host -> per image, in the order of the images,
    (width, height, entropy-coded data)"""
    streams = [None] * n
    for g, d in zip(layout["groups"], data):
        M = len(g["indices"])
        offs = np.asarray(head, np.uint8)[8 * g["off"]:8 * (g["off"] + M + 1)].view(np.int64)
        for j, i in enumerate(g["indices"]):
            streams[i] = (g["width"], g["height"], np.asarray(d, np.uint8)[offs[j]:offs[j + 1]])
    return streams


def files_from_host(head, data, layout, n):
    """-> the n JPEG files' bytes: jpeg_headers, the stream, EOI"""
    return [jpeg_headers(w, h, layout["quality"]) + s.tobytes() + EOI for w, h, s in streams_from_host(head, data, layout, n)]


def encode_frames_device(images, divisors=None, magma=None, quality=90):
    """images: device tensors, float32 or uint8, (H, W), (H, W, 1) or (H, W, 3), of any mix of sizes; divisors: per image (default 1); magma: per image
    (default False; one channel only); quality 1..100 -> list of the JPEG files' bytes.  Two device-to-host copies: the offsets, then the used bytes."""
    buf, layout = enqueue_frames_device(images, divisors, magma, quality)
    head = buf[:layout["head"]].cpu().numpy()
    data = [buf[g["pos"]:g["pos"] + size].cpu().numpy() for g, size in zip(layout["groups"], group_sizes(head, layout))]
    return files_from_host(head, data, layout, len(images))
