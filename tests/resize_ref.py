"""The 8-bit resize contract of the scannetpp layout's --res_scale restated in numpy: plain integer arithmetic, no device.  It shares no
code with iris_amd/utils/resize.py or iris_amd/csrc/iris_resize.h.

    resize_linear_u8    what the reference's open_png does to a photograph or an albedo prior: cv2.resize(img, (Wt, Ht)) on the decoded 8-bit image, i.e.
                        OpenCV's default INTER_LINEAR on its 8-bit fixed-point path
        same size       the source, unchanged
        exact 2         H == 2 Ht and W == 2 Wt (BOTH axes): (a + b + c + d + 2) >> 2 over each 2 x 2 block -- OpenCV switches from INTER_LINEAR to its fast
                        area path
        otherwise       per axis of ns source and nd destination samples (linear_axis): scale = 1.0 / (nd / ns) in double (the inverse is formed first: not
                        ns / nd); f = float32((d + 0.5) scale - 0.5), product and difference in double, ONE rounding; s = floor(f); f = float32(f - s);
                        s < 0 -> s = 0, f = 0; s >= ns - 1 -> s = ns - 1, f = 0; int16 weights rint(float32(1 - f) 2048) and rint(f 2048), half to even;
                        the second tap's index is min(s + 1, ns - 1).  Horizontal pass in int32: R = S[s] w0 + S[s + 1] w1.  Vertical pass:
                        dst = (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2.  Upscaling runs the same code.
    resize_nearest_u8   what sample_nearest does to the segment ids: PIL's Image.NEAREST.  Per axis a = ns / nd in double, x = a 0.5, then for every d IN ORDER
                        index = min(floor(x), ns - 1) and x += a: accumulated addition, as PIL's affine scan steps its source coordinate.  (The multiply form
                        floor((d + 0.5) a) differs from PIL, e.g. at 24 x 40 -> 9 x 15.)

What this restatement is and is not:
  * The linear contract restates OpenCV's resize.cpp from its published algorithm.  It has NOT been compared with a cv2 binary: parity with cv2 is unpinned
    (as the closest hit's and tiny-cuda-nn's are).  tests/test_resize_cpu.py holds it within one code value of exact bilinear interpolation and on hand cases.
  * It is OpenCV's own C path: opencv-python does not hand 8-bit linear resizing to IPP unless inexact IPP is enabled.
  * PIL's JPEG decoder may differ from cv2's by a code value before any resize; that was already true at scale 1.
  * The nearest contract IS pinned: tests/test_resize_cpu.py compares it with PIL on a few hundred size pairs.
"""
import numpy as np

COEF_BITS = 11
COEF_ONE = 1 << COEF_BITS


def linear_axis(ns, nd):
    """-> (ofs (nd) int32, coef (nd, 2) int16) of one axis"""
    ofs, coef = np.zeros(nd, np.int32), np.zeros((nd, 2), np.int16)
    scale = 1.0 / (float(nd) / float(ns))
    for d in range(nd):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= ns - 1:
            s, f = ns - 1, np.float32(0)
        ofs[d] = s
        coef[d, 0] = np.int16(np.rint(np.float32(np.float32(1) - f) * np.float32(COEF_ONE)))
        coef[d, 1] = np.int16(np.rint(f * np.float32(COEF_ONE)))
    return ofs, coef


def nearest_axis(ns, nd):
    """-> ofs (nd) int32 of one axis"""
    ofs = np.zeros(nd, np.int32)
    a = float(ns) / float(nd)
    x = a * 0.5
    for d in range(nd):
        ofs[d] = min(int(np.floor(x)), ns - 1)
        x += a
    return ofs


def resize_linear_u8(src, hw):
    """src (H, W, C) or (H, W) uint8 -> (Ht, Wt, C) or (Ht, Wt) uint8"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    H, W = src.shape[:2]
    Ht, Wt = int(hw[0]), int(hw[1])
    if (H, W) == (Ht, Wt):
        return src
    S = src.astype(np.int32)
    if H == 2 * Ht and W == 2 * Wt:
        return ((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    xo, xc = linear_axis(W, Wt)
    yo, yc = linear_axis(H, Ht)
    x1, y1 = np.minimum(xo + 1, W - 1), np.minimum(yo + 1, H - 1)
    tail = (1,) * (src.ndim - 2)
    w0, w1 = xc[:, 0].astype(np.int32).reshape(1, Wt, *tail), xc[:, 1].astype(np.int32).reshape(1, Wt, *tail)
    R = S[:, xo] * w0 + S[:, x1] * w1                                           # (H, Wt, ...) int32
    b0, b1 = yc[:, 0].astype(np.int32).reshape(Ht, 1, *tail), yc[:, 1].astype(np.int32).reshape(Ht, 1, *tail)
    out = (((b0 * (R[yo] >> 4)) >> 16) + ((b1 * (R[y1] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_nearest_u8(src, hw):
    """src (H, W) uint8 (further axes ride along) -> (Ht, Wt) uint8"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim >= 2
    H, W = src.shape[:2]
    Ht, Wt = int(hw[0]), int(hw[1])
    return np.ascontiguousarray(src[nearest_axis(H, Ht)][:, nearest_axis(W, Wt)])
