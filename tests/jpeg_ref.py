"""The video stage's JPEG frame contract restated in numpy: uint8 pixels -> a complete baseline JPEG file.  It shares no code with
iris_amd/utils/jpeg.py or iris_amd/csrc/iris_jpeg.h; the tables are typed in from ITU-T T.81 Annex K (tests/test_jpeg_cpu.py holds them against the tables
libjpeg writes into its own files).

    pixels      (H2, W2) or (H2, W2, 3) uint8, even sizes; a grey image is R = G = B
    padding     to multiples of 16 by repeating the last column, then the last row
    colour      Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
                Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16          (8388608 = 128 << 16)
                Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16          grey: Y = v, Cb = Cr = 128 exactly
    chroma      2 x 2 mean (a + b + c + d + 2) >> 2; every sample minus 128
    DCT         M[k][n] = +-C[j], C = (-, 32138, 30274, 27246, 23170, 18205, 12540, 6393) = round(32768 cos(j pi / 16)), row 0 = 23170: with
                a = (2 n + 1) k mod 32, a > 16 -> 32 - a, then a > 8 -> the sign flips and a -> 16 - a.  Rows: t = (x M^T + 256) >> 9 (128 times the 1-D
                transform; the sums stay below 2^26, t below 2^17); columns: c8 = (M t + 524288) >> 20 (sums below 2^35: 64-bit); >> is the arithmetic
                shift.  c8 is eight times the DCT coefficient.  On the 0 / 255 checkerboard it differs from the DCT in float64 only
                at coefficients within 0.06 of a tie (13-bit constants and three fractional bits between the passes: within 0.15).
    quantise    table entry e (quant_tables): q = sign(c8) * ((|c8| + 4 e) // (8 e)): c8 / (8 e) rounded half away from zero
    entropy     Annex K tables; per MCU Y00 Y01 Y10 Y11 Cb Cr; DC difference against the previous block of the component, 0 at the start of an interval
    intervals   one per MCU row: padded with 1-bits to a byte, FF -> FF 00, then RSTm (m = row mod 8) except after the last
    file        SOI, APP0 JFIF 1.01 (no units, 1:1), DQT luma, DQT chroma, SOF0, DHT x 4 (DC0, AC0, DC1, AC1), DRI, SOS, data, EOI

Fidelity against libjpeg (Pillow 12, libjpeg-turbo: qtables=quant_tables(q), subsampling=2, optimize=False), PSNR of the decoded file against the coded
pixels, ours minus libjpeg's, over the contents of tests/test_jpeg_cpu.py (noise, ramp, flat, checkerboard, clipped float, uint8; grey, RGB and magma):
MEASURED_DEFICITS and MARGIN_DB below."""
import numpy as np

QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
            0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
            0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
            0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
              0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
              0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
              0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])

# measured on the CPU (tests/test_jpeg_cpu.py::test_fidelity_against_libjpeg prints them): the largest deficit in dB per quality, and where
#   50: 0.712  3x5x3 uint8 noise (eight pixels)      90: 0.510  146x18x3 ramp      100: 24.002  18x34x3 checkerboard
# The 24 dB are not a loss of that size: at quality 100 libjpeg reproduces the 0 / 255 checkerboard exactly (PSNR capped at 100 dB) and this encoder gets 3 of
# 1836 values wrong by one level (76.0 dB) -- the checkerboard's coefficients include exact ties (123.5, 127.5), which the two transforms break differently.
# Without the checkerboard the largest deficit at quality 100 is 0.962 dB (18x34x3 ramp).  The rule -- the largest deficit rounded up to the next 0.25 dB plus
# 0.25 dB -- gives 24.5 dB over all three qualities; the test applies it per quality, which is never wider: 1.0, 1.0 and 24.5 dB.
MEASURED_DEFICITS = {50: 0.712, 90: 0.510, 100: 24.002}
MARGIN_DB = {50: 1.0, 90: 1.0, 100: 24.5}


def zigzag():
    """natural (row-major) index of the k-th coefficient in zigzag order"""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8))
    return np.array(order)


def quant_tables(quality):
    """the two Annex K tables scaled by the IJG rule, natural order, (2, 64)"""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.stack([QUANT_LUMA, QUANT_CHROMA]) * s + 50) // 100, 1, 255)


def dct_matrix():
    C = [0, 32138, 30274, 27246, 23170, 18205, 12540, 6393, 0]
    M = np.zeros((8, 8), np.int64)
    for k in range(8):
        for n in range(8):
            a, sign = (2 * n + 1) * k % 32, 1
            if a > 16:
                a = 32 - a
            if a > 8:
                a, sign = 16 - a, -1
            M[k, n] = 23170 if k == 0 else sign * C[a]
    return M


def huff_codes(bits, vals):
    """symbol -> (code, length): codes of each length are consecutive, the first of a length is twice the one after the last of the length before"""
    table, code, i = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[i]] = (code, length)
            code += 1
            i += 1
        code <<= 1
    return table


def planes(px):
    """-> Y (Hp, Wp), Cb and Cr (Hp / 2, Wp / 2), int64, before the level shift"""
    px = np.asarray(px)
    assert px.dtype == np.uint8 and px.shape[0] % 2 == 0 and px.shape[1] % 2 == 0 and px.shape[0] > 0 and px.shape[1] > 0
    rgb = (np.repeat(px[..., None], 3, 2) if px.ndim == 2 else px).astype(np.int64)
    H, W = rgb.shape[:2]
    rgb = np.pad(rgb, ((0, -H % 16), (0, -W % 16), (0, 0)), mode="edge")
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16
    half = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2      # noqa: E731
    return Y, half(Cb), half(Cr)


def coefficients(plane, table):
    """(h, w) samples, h and w multiples of 8 -> (h / 8, w / 8, 64) quantised coefficients in zigzag order"""
    h, w = plane.shape
    x = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    M = dct_matrix()
    t = (x @ M.T + 256) >> 9
    c8 = (M @ t + 524288) >> 20
    assert np.abs(x @ M.T).max() < 2 ** 26 and np.abs(t).max() < 2 ** 17 and np.abs(M @ t).max() < 2 ** 35
    e = table.reshape(8, 8)
    q = np.sign(c8) * ((np.abs(c8) + 4 * e) // (8 * e))
    return q.reshape(h // 8, w // 8, 64)[..., zigzag()]


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def interval(self):
        """the bits so far, padded with ones to a byte, FF -> FF 00"""
        pad = -self.n % 8
        raw = ((self.acc << pad) | ((1 << pad) - 1)).to_bytes((self.n + pad) // 8, "big")
        return raw.replace(b"\xff", b"\xff\x00")


def _magnitude(v):
    """-> (category, the category's low bits: v, or v - 1 for a negative v)"""
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def _block(w, zz, pred, dc, ac):
    size, low = _magnitude(int(zz[0]) - pred)
    w.put(*dc[size])
    w.put(low, size)
    run = 0
    for v in zz[1:]:
        v = int(v)
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*ac[0xF0])
            run -= 16
        size, low = _magnitude(v)
        w.put(*ac[run << 4 | size])
        w.put(low, size)
        run = 0
    if run:
        w.put(*ac[0x00])
    return int(zz[0])


def entropy_data(px, quality):
    """the bytes between the SOS header and EOI"""
    qt = quant_tables(quality)
    Y, Cb, Cr = planes(px)
    cy, cb, cr = coefficients(Y, qt[0]), coefficients(Cb, qt[1]), coefficients(Cr, qt[1])
    dc = (huff_codes(*DC_LUMA), huff_codes(*DC_CHROMA))
    ac = (huff_codes(*AC_LUMA), huff_codes(*AC_CHROMA))
    rows, cols = cb.shape[:2]
    out = b""
    for my in range(rows):
        w, pred = _Bits(), [0, 0, 0]
        for mx in range(cols):
            for by, bx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                pred[0] = _block(w, cy[2 * my + by, 2 * mx + bx], pred[0], dc[0], ac[0])
            pred[1] = _block(w, cb[my, mx], pred[1], dc[1], ac[1])
            pred[2] = _block(w, cr[my, mx], pred[2], dc[1], ac[1])
        out += w.interval()
        if my < rows - 1:
            out += bytes([0xFF, 0xD0 + my % 8])
    return out


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def headers(width, height, quality):
    qt = quant_tables(quality)[:, zigzag()]
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _segment(0xDB, bytes([0]) + bytes(qt[0].tolist())) + _segment(0xDB, bytes([1]) + bytes(qt[1].tolist()))
    out += _segment(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, ((width + 15) // 16).to_bytes(2, "big"))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(px, quality=90):
    """(H2, W2) or (H2, W2, 3) uint8 with even sizes -> the JPEG file's bytes"""
    px = np.asarray(px)
    return headers(px.shape[1], px.shape[0], quality) + entropy_data(px, quality) + b"\xff\xd9"
