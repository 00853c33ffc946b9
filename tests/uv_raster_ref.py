"""The UV rasteriser's contract restated in numpy and Python integers: the yardstick of tests/test_texture.py and
tests/test_texture_cpu.py.  A helper, not a test; nothing here is shared with the implementation.

  texel (r, c) of an H x W texture: centre u = (c + .5) / W, v = (r + .5) / H, row 0 at v ~ 0
  snapping     X = rint(float64(u) * W * 256), Y = rint(float64(v) * H * 256) (round half to even, as llrint); a centre is (256 c + 128, 256 r + 128)
  edges        int64 E_ab(p) = (bx - ax)(py - ay) - (by - ay)(px - ax); A = E_01(v2); A == 0 covers nothing; all three times sign(A): inside is >= 0
  ties         E == 0 counts only where the interior lies on the +x side of the edge or, for an edge whose inward normal has no x component, on the +y side
  overlap      the lowest face index wins; uncovered: -1
  barycentrics b0 = float32(float64(E_12) / float64(|A|)), b1 = float32(float64(E_20) / float64(|A|)), b2 = float32(1) - b0 - b1
  position     float32, every operation rounded on its own: ((b0 * v0) + (b1 * v1)) + (b2 * v2), the vertices named by f[face]
"""
import numpy as np

SUB = 256


def snap(vt, H, W):
    vt = np.asarray(vt, np.float32).astype(np.float64)
    return np.rint(vt[:, 0] * W * SUB).astype(np.int64), np.rint(vt[:, 1] * H * SUB).astype(np.int64)


def _oriented_edges(x, y):
    """x, y: the three snapped vertices (Python ints) -> (|A|, [(gx, gy, c, keeps_zero)] for the edges 01, 12, 20) with E(p) = gx px + gy py + c, or None"""
    A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if A == 0:
        return None
    s = 1 if A > 0 else -1
    edges = []
    for a, b in ((0, 1), (1, 2), (2, 0)):
        # s * ((bx - ax)(py - ay) - (by - ay)(px - ax)): the inward normal is its gradient
        gx, gy = -s * (y[b] - y[a]), s * (x[b] - x[a])
        edges.append((gx, gy, -(gx * x[a] + gy * y[a]), gx > 0 or (gx == 0 and gy > 0)))
    return A * s, edges


def coverage(vt, ft, tex_res):
    """-> count (H, W) int32: how many faces cover each texel centre, and ids (H, W) int32: the lowest of them (-1: none)"""
    H, W = (tex_res, tex_res) if np.isscalar(tex_res) else tex_res
    X, Y = snap(vt, H, W)
    ids = np.full((H, W), -1, np.int32)
    count = np.zeros((H, W), np.int32)
    px_all = np.arange(W, dtype=np.int64) * SUB + SUB // 2
    py_all = np.arange(H, dtype=np.int64) * SUB + SUB // 2
    for face in range(len(ft) - 1, -1, -1):                 # descending: the lowest index is written last
        i = [int(k) for k in ft[face]]
        x, y = [int(X[k]) for k in i], [int(Y[k]) for k in i]
        tri = _oriented_edges(x, y)
        if tri is None:
            continue
        c0, c1 = max(0, -((min(x) - SUB // 2) // -SUB)), min(W - 1, (max(x) - SUB // 2) // SUB)          # ceil and floor in Python integers
        r0, r1 = max(0, -((min(y) - SUB // 2) // -SUB)), min(H - 1, (max(y) - SUB // 2) // SUB)
        if c0 > c1 or r0 > r1:
            continue
        px, py = np.meshgrid(px_all[c0:c1 + 1], py_all[r0:r1 + 1])
        inside = np.ones(px.shape, bool)
        for gx, gy, c, keeps_zero in tri[1]:
            E = gx * px + gy * py + c                       # int64: |E| < 2^47 under the host checks
            inside &= (E >= 0) if keeps_zero else (E > 0)
        count[r0:r1 + 1, c0:c1 + 1] += inside
        ids[r0:r1 + 1, c0:c1 + 1][inside] = face
    return count, ids


def rasterize_uv_ref(vt, ft, v, f, tex_res):
    """-> {'ids' (H, W) int32, 'mask' (H, W) bool, 'bary' (H, W, 2) float32, 'xyz' (H, W, 3) float32, 'count' (H, W) int32}; zeros where uncovered"""
    H, W = (tex_res, tex_res) if np.isscalar(tex_res) else tex_res
    v = np.asarray(v, np.float32)
    count, ids = coverage(vt, ft, (H, W))
    X, Y = snap(vt, H, W)
    bary = np.zeros((H, W, 2), np.float32)
    xyz = np.zeros((H, W, 3), np.float32)
    one = np.float32(1.0)
    for r, c in zip(*np.nonzero(ids >= 0)):
        face = int(ids[r, c])
        i = [int(k) for k in ft[face]]
        area, edges = _oriented_edges([int(X[k]) for k in i], [int(Y[k]) for k in i])
        px, py = SUB * int(c) + SUB // 2, SUB * int(r) + SUB // 2
        E12 = edges[1][0] * px + edges[1][1] * py + edges[1][2]
        E20 = edges[2][0] * px + edges[2][1] * py + edges[2][2]
        b0 = np.float32(np.float64(E12) / np.float64(area))
        b1 = np.float32(np.float64(E20) / np.float64(area))
        b2 = np.float32(np.float32(one - b0) - b1)
        v0, v1, v2 = (v[int(k)] for k in f[face])
        bary[r, c] = (b0, b1)
        xyz[r, c] = (b0 * v0 + b1 * v1) + b2 * v2          # float32 arrays: every product and sum rounds to float32
    return {"ids": ids, "mask": ids >= 0, "bary": bary, "xyz": xyz, "count": count}


def quantize_ref(x):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return (np.clip(np.where(np.isnan(x), np.float32(0), x), 0, 1) * np.float32(255)).astype(np.uint8)
