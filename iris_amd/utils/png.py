"""8-bit PNG files (grey or RGB, no interlace) for the video stage: the container on the host, the pixels' way into it on the device or on the host.

    device arm  encode_frames_device: iris_png_rows (quantiser, MAGMA colour map, even crop, Sub filter: one launch per group of equal-size images), iris_png_encode
                (the EXR writer's deflate kernels in zlib-stream mode), ONE device-to-host copy, then png_container around each stream
    host arm    quantize_host (the reference's save_image in numpy) + encode_png_host (the same Sub filter, zlib.compress); also the oracle of the container

The quantiser is (np.clip(image, 0, 1) * 255).astype(np.uint8) with NaN -> 0 after an IEEE division by the image's divisor; the colour map is OpenCV's
COLORMAP_MAGMA as R,G,B (the table lives in the library: iris_png_magma_table).  Both arms crop to even height and width, as the reference's save_image does.
"""
import ctypes as C
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_magma = None


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + bytes(data) + struct.pack(">I", zlib.crc32(data, zlib.crc32(tag)) & 0xFFFFFFFF)


def png_container(width, height, channels, zlib_stream):
    """signature, IHDR (8 bit, colour type 0 for one channel or 2 for three, deflate, adaptive filtering, no interlace), ONE IDAT holding zlib_stream -- the
    zlib stream of the filtered scanlines --, IEND"""
    if channels not in (1, 3) or width <= 0 or height <= 0:
        raise ValueError(f"png_container: {width} x {height} x {channels}: one or three channels and a positive size")
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 0 if channels == 1 else 2, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib_stream) + _chunk(b"IEND", b"")


def sub_filter(a):
    """(H, W) or (H, W, C) uint8 -> the filtered scanlines: per row the filter type 1 (Sub) and every byte minus the byte one pixel to its left (mod 256)"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a = a[..., None] if a.ndim == 2 else a
    d = a.copy()
    d[:, 1:] -= a[:, :-1]
    rows = np.empty((a.shape[0], 1 + a.shape[1] * a.shape[2]), np.uint8)
    rows[:, 0] = 1
    rows[:, 1:] = d.reshape(a.shape[0], -1)
    return rows.tobytes()


def encode_png_host(u8_array, level=1):
    """(H, W), (H, W, 1) or (H, W, 3) uint8 -> the PNG file's bytes: Sub filter, zlib.compress(level), png_container"""
    a = np.asarray(u8_array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError(f"encode_png_host: expected a non-empty (H, W), (H, W, 1) or (H, W, 3) uint8 array, got {a.dtype} {a.shape}")
    return png_container(a.shape[1], a.shape[0], 1 if a.ndim == 2 else a.shape[2], zlib.compress(sub_filter(a), level))


def magma_table():
    """(256, 3) uint8, R,G,B: the table the device kernel uses (matplotlib's _magma_data * 255 rounded to nearest, which is OpenCV's COLORMAP_MAGMA)"""
    global _magma
    if _magma is None:
        from .. import _lib as L
        buf = (C.c_uint8 * 768)()
        L.lib().iris_png_magma_table(buf)
        _magma = np.frombuffer(bytes(buf), np.uint8).reshape(256, 3).copy()
    return _magma


def quantize_host(image, divisor=1.0, magma=False):
    """The reference's save_image up to the file, in numpy: float32 (H, W) / (H, W, C) -> uint8, image / divisor, NaN -> 0, clip to [0,1], * 255, truncated;
    magma (one channel): through the colour map, as R,G,B; the trailing odd row / column dropped.  uint8 input skips the quantiser."""
    from .. import _lib as L
    a = np.asarray(image)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[..., 0]
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise L.IrisError(f"quantize_host: expected (H, W), (H, W, 1) or (H, W, 3), got {a.shape}")
    if magma and a.ndim == 3:
        raise L.IrisError("quantize_host: a magma image has one channel")
    if a.dtype != np.uint8:
        with np.errstate(invalid="ignore", divide="ignore"):
            v = a.astype(np.float32) / np.float32(divisor)
            v = np.where(np.isnan(v), np.float32(0), v)
            a = (np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    if magma:
        a = magma_table()[a]
    h, w = a.shape[:2]
    if h - h % 2 == 0 or w - w % 2 == 0:
        raise L.IrisError(f"quantize_host: a {h} x {w} image cropped to even height and width is empty")
    return np.ascontiguousarray(a[:h - h % 2, :w - w % 2])


def enqueue_frames_device(images, divisors=None, magma=None):
    """The device part of encode_frames_device, enqueued on the current stream: -> (buf, layout).  buf: ONE device uint8 tensor holding, first, every group's
    stream offsets (int64) and then every group's streams at their worst-case size (known in advance: nothing is read back here).  layout: per group
    (indices of its images, width, height, channels, position of its offsets in int64 units, position of its streams in bytes) for files_from_host."""
    import torch
    from .. import _lib as L
    n = len(images)
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
        if int(lib.iris_png_row_bytes(H, W, ch, int(magma[i]))) == 0:
            raise L.IrisError(f"encode_frames_device: image {i}: a {H} x {W} image cropped to even height and width is empty")
        tensors.append(t)
        groups.setdefault((H, W, ch, t.dtype, magma[i], t.device), []).append(i)
    dev = tensors[0].device
    if any(t.device != dev for t in tensors):
        raise L.IrisError("encode_frames_device: the images lie on different devices")
    layout, n_off, n_bytes = [], 0, 0
    for (H, W, ch, dtype, mg, _), idx in groups.items():
        block = int(lib.iris_png_row_bytes(H, W, ch, int(mg)))
        cap = int(lib.iris_png_stream_bound(block))
        layout.append(dict(indices=idx, width=W - W % 2, height=H - H % 2, channels=3 if mg else ch, off=n_off, pos=n_bytes, block=block, cap=cap,
                           shape=(H, W, ch), u8=dtype == torch.uint8, magma=mg))
        n_off += len(idx) + 1
        n_bytes += (len(idx) * cap + 255) // 256 * 256
    head = (8 * n_off + 255) // 256 * 256
    buf = torch.empty(head + n_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for g in layout:
            M, (H, W, ch) = len(g["indices"]), g["shape"]
            g["pos"] += head
            ws_bytes = int(lib.iris_png_workspace_bytes(M, g["block"]))
            if ws_bytes == 0:
                raise L.IrisError(f"encode_frames_device: unsupported size ({M} images of {g['block']} scanline bytes)")
            rows = torch.empty(M * g["block"], dtype=torch.uint8, device=dev)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            ptrs = (C.c_void_p * M)(*[tensors[i].data_ptr() for i in g["indices"]])
            divs = (C.c_float * M)(*[divisors[i] for i in g["indices"]])
            flags = (C.c_uint8 * M)(*[int(g["magma"])] * M)
            L.mark()
            L.check(lib.iris_png_rows(ptrs, divs, flags, M, H, W, ch, int(g["u8"]), L.ptr(rows), L.stream()))
            L.mark("png rows")
            L.check(lib.iris_png_encode(L.ptr(rows), M, g["block"], C.c_void_p(buf.data_ptr() + g["pos"]), C.c_void_p(buf.data_ptr() + 8 * g["off"]),
                                        L.ptr(ws), ws_bytes, L.stream()))
            L.mark("png deflate")
    return buf, [{k: g[k] for k in ("indices", "width", "height", "channels", "off", "pos", "cap")} for g in layout]


def streams_from_host(host, layout, n):
    """host: enqueue_frames_device's buf on the host (a uint8 numpy array) -> per image, in the order of the images, (width, height, channels, zlib stream)"""
    host = np.asarray(host, np.uint8)
    streams = [None] * n
    for g in layout:
        M = len(g["indices"])
        offs = host[8 * g["off"]:8 * (g["off"] + M + 1)].view(np.int64)
        if offs[0] != 0 or (np.diff(offs) <= 0).any() or offs[M] > M * g["cap"]:
            from .. import _lib as L
            raise L.IrisError("streams_from_host: the stream offsets are not what iris_png_encode writes (was the copy complete?)")
        for j, i in enumerate(g["indices"]):
            streams[i] = (g["width"], g["height"], g["channels"], host[g["pos"] + offs[j]:g["pos"] + offs[j + 1]])
    return streams


def files_from_host(host, layout, n):
    """-> the n PNG files' bytes: png_container around each of streams_from_host's streams"""
    return [png_container(*s) for s in streams_from_host(host, layout, n)]


def encode_frames_device(images, divisors=None, magma=None):
    """images: device tensors, float32 or uint8, (H, W), (H, W, 1) or (H, W, 3), of any mix of sizes; divisors: per image (default 1); magma: per image
    (default False; one channel only) -> list of the PNG files' bytes.  Step (a) and step (b) per group of equal-size images, one device-to-host copy."""
    buf, layout = enqueue_frames_device(images, divisors, magma)
    return files_from_host(buf.cpu().numpy(), layout, len(images))
