"""The segmentation fusion's contract in numpy (iris_amd/utils/segmentation.py, csrc/iris_labels.h): a restatement of the reference's
utils/fuse_segmentation.py lines 69-87 (the vote and the per-triangle winner) and 99-100 (the painted view), with the two decisions DESIGN.md 5c-16
takes: votes outside [1, n_labels) are dropped instead of spilling into the neighbouring row, and equal counts go to the lower id."""
import numpy as np


def vote(tri, valid, ids, F, n_labels, hist=None):
    """hist[tri, long(id)] += 1 over the valid pixels whose id, truncated toward zero, lies in [1, n_labels) and whose triangle lies in [0, F).
    ids: float (NaN allowed) or integer, one per pixel.  -> (F, n_labels) int64 (pass `hist` to accumulate over views)."""
    hist = np.zeros((F, n_labels), np.int64) if hist is None else hist
    tri, valid, ids = np.asarray(tri).reshape(-1), np.asarray(valid, bool).reshape(-1), np.asarray(ids).reshape(-1)
    if ids.dtype.kind == "f":
        finite = np.isfinite(ids)
        whole = np.where(finite, np.trunc(np.where(finite, ids, 0)), -1).astype(np.int64)       # .long(); NaN and infinities vote for nothing
    else:
        whole = ids.astype(np.int64)
    keep = valid & (whole >= 1) & (whole < n_labels) & (tri >= 0) & (tri < F)
    np.add.at(hist, (tri[keep].astype(np.int64), whole[keep]), 1)
    return hist


def triangle_labels(hist):
    """1 + argmax(hist[:, 1:], 1) (numpy's argmax: the first of equal maxima, i.e. the lower id), 0 where that maximum is 0"""
    hist = np.asarray(hist)
    if hist.shape[1] < 2:
        return np.zeros(hist.shape[0], np.int64)
    body = hist[:, 1:]
    return np.where(body.max(1) == 0, 0, 1 + body.argmax(1)).astype(np.int64)


def label_view(tri, valid, table, miss=0):
    """table[tri] on a hit, miss otherwise -> int64"""
    tri, valid = np.asarray(tri).reshape(-1), np.asarray(valid, bool).reshape(-1)
    return np.where(valid, np.asarray(table, np.int64)[np.where(valid, tri, 0)], miss).astype(np.int64)


def reference_flat(tri, valid, ids, F, seg_num):
    """A literal transcription of fuse_segmentation.py:69-87: a flat vector of F * seg_num counters, inds = tri * seg_num + long(id) over the valid pixels,
    reshape(-1, seg_num)[:, 1:].max(-1) + 1, zeroed where the maximum is 0.  Raises IndexError where torch's scatter_add_ would (an index out of range).
    Equal maxima resolve as numpy's argmax (torch's CUDA max does not promise which)."""
    labels = np.zeros(F * seg_num, np.int64)
    tri, valid = np.asarray(tri).reshape(-1), np.asarray(valid, bool).reshape(-1)
    inds = tri[valid].astype(np.int64) * int(seg_num) + np.trunc(np.asarray(ids, np.float64).reshape(-1)[valid]).astype(np.int64)
    if len(inds) and (inds.min() < 0 or inds.max() >= labels.size):
        raise IndexError("scatter_add_: index out of range")
    np.add.at(labels, inds, 1)
    body = labels.reshape(-1, seg_num)[:, 1:]
    new_label = body.argmax(-1) + 1
    new_label[body.max(-1) == 0] = 0
    return new_label
