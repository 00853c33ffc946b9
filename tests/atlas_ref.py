"""The area-proportional atlas and the seam dilation restated in numpy float64 and Python integers: the yardstick of
tests/test_atlas.py and tests/test_atlas_cpu.py.  A helper, not a test; nothing here is imported from the package.

  measure    float64 (float32 vertices converted first), every product and sum rounded on its own, sums left to right: e1 = p1 - p0, e2 = p2 - p0, c = e1 x e2,
             S = cx^2 + cy^2 + cz^2;  l0 = |p2 - p1|^2, l1 = |p0 - p2|^2, l2 = |p1 - p0|^2;  corner = argmax, first maximum.  A face naming a vertex out of
             range, or with S not finite or <= 0: S = 0, corner = 0.
  ladder     D_j = M[j mod 2] 2^floor(j / 2), M = (1, 1.4142135623730951), j in [-800, 800]
  class      k_f = the smallest k in [2, KMAX] (2^KMAX = R) with 4 16^k >= S_f D_j, else KMAX; cells_k = ceil(n_k / 2); j fits when sum cells_k 4^k <= R^2;
             the step used is what this bisection returns: lo = -800 (must fit), hi = 801, mid = (lo + hi) // 2 -> lo when it fits, hi when not, until
             hi - lo = 1; j = lo.  It fits and j + 1 does not (or j = 800).  (The texel sum is not strictly monotone in j: a face that moves up into the free
             half of a cell gives back its own cell; so the bisection, not "the largest j that fits", is the contract.)
  place      rank r by face index within the class; cell r // 2, lower half for even r, upper for odd; classes from the largest down;
             o = base_k + (r // 2) 4^k; (x0, y0) = the even and the odd bits of o, compacted; grid_atlas's two triangles inside the cell (margin .25, half gap .25);
             mesh corner (corner + i) mod 3 takes P_i; UV = texels / R
  dilate     an uncovered texel takes the covered texel within Chebyshev distance n of smallest (squared distance, row, column)
"""
import math

import numpy as np

KMIN, JMIN, JMAX = 2, -800, 800
M = (1.0, 1.4142135623730951)


class AtlasError(ValueError):
    pass


def check_res(tex_res):
    """-> (R, KMAX); AtlasError unless tex_res is a square power of two in [4, 8192]"""
    if isinstance(tex_res, (tuple, list)):
        if len(tex_res) != 2 or tex_res[0] != tex_res[1]:
            raise AtlasError(f"tex_res = {tex_res!r}: the area atlas needs a square texture")
        tex_res = tex_res[0]
    if isinstance(tex_res, bool) or not isinstance(tex_res, (int, np.integer)):
        raise AtlasError(f"tex_res = {tex_res!r}: an integer")
    R = int(tex_res)
    if R < 4 or R > 8192 or R & (R - 1):
        raise AtlasError(f"tex_res = {R}: a power of two in [4, 8192]")
    return R, R.bit_length() - 1


def min_res(F):
    """the smallest power of two R with ceil(F / 2) 16 <= R^2"""
    R = 4
    while (F + 1) // 2 * 16 > R * R:
        R *= 2
    return R


def density(j):
    assert JMIN <= j <= JMAX
    return math.ldexp(M[j % 2], j // 2)          # Python's % and // floor: j mod 2 in {0, 1}


def _sq3(d):
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def measure(v, f):
    """-> S (F) float64, corner (F) uint8"""
    v = np.asarray(v, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(f).astype(np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < v.shape[0])).all(1)
    g = np.where(ok[:, None], f, 0)
    if v.shape[0] == 0:
        return np.zeros(f.shape[0]), np.zeros(f.shape[0], np.uint8)
    p0, p1, p2 = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2, d = p1 - p0, p2 - p0, p2 - p1
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        S = _sq3(c)
        l0, l1, l2 = _sq3(d), _sq3(p0 - p2), _sq3(e1)
        corner = np.zeros(f.shape[0], np.uint8)
        corner[l1 > l0] = 1
        corner[l2 > np.where(corner == 1, l1, l0)] = 2
        bad = ~ok | ~np.isfinite(S) | ~(S > 0)
    return np.where(bad, 0.0, S), np.where(bad, 0, corner).astype(np.uint8)


def classes(S, j, kmax):
    """-> k (F) uint8, histogram (kmax + 1) int64, faces clamped at KMIN, at KMAX"""
    with np.errstate(over="ignore"):
        p = S * density(j)
    k = np.full(S.shape[0], kmax, np.int64)
    for c in range(kmax - 1, KMIN - 1, -1):
        k[4.0 * 16.0 ** c >= p] = c
    return k.astype(np.uint8), np.bincount(k, minlength=kmax + 1).astype(np.int64), int((4.0 * 16.0 ** (KMIN - 1) >= p).sum()), int((~(4.0 * 16.0 ** kmax >= p)).sum())


def texels_needed(hist):
    return sum((int(n) + 1) // 2 * 4 ** k for k, n in enumerate(hist))


def fits(S, j, R, kmax):
    return texels_needed(classes(S, j, kmax)[1]) <= R * R


def choose_j(S, R, kmax):
    F = S.shape[0]
    if (F + 1) // 2 * 16 > R * R:
        raise AtlasError(f"{F} faces need {(F + 1) // 2} cells of 4 x 4 texels: tex_res = {R} holds {R * R // 16}; the smallest that fits is {min_res(F)}")
    if not fits(S, JMIN, R, kmax):
        raise AtlasError("the faces do not fit at the ladder's lowest density")
    lo, hi = JMIN, JMAX + 1                       # fits(lo), not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(S, mid, R, kmax):
            lo = mid
        else:
            hi = mid
    return lo


def even_bits(o):
    """bits 0, 2, 4, ... of the integers o, compacted"""
    o = np.asarray(o, np.int64)
    out = np.zeros_like(o)
    for b in range(16):
        out |= ((o >> (2 * b)) & 1) << b
    return out


def area_atlas_ref(v, f, tex_res):
    """-> vt (3 F, 2) float32, ft (F, 3) int32, report"""
    R, kmax = check_res(tex_res)
    f = np.asarray(f).reshape(-1, 3)
    F = f.shape[0]
    S, corner = measure(v, f)
    j = choose_j(S, R, kmax)
    k, hist, at_min, at_max = classes(S, j, kmax)
    base = np.zeros(kmax + 2, np.int64)
    for c in range(kmax, -1, -1):
        base[c] = base[c + 1] + (int(hist[c]) + 1) // 2 * 4 ** c          # base[c + 1] is where class c starts
    k = k.astype(np.int64)
    r = np.zeros(F, np.int64)
    for c in range(KMIN, kmax + 1):
        sel = k == c
        r[sel] = np.arange(int(sel.sum()))
    o = base[k + 1] + (r // 2) * 4 ** k
    x0, y0 = even_bits(o).astype(np.float64), even_bits(o >> 1).astype(np.float64)
    s = (2.0 ** k)
    x1, y1 = x0 + s, y0 + s
    m = g = 0.25
    lower = np.stack([np.stack([x0 + m, y0 + m], -1), np.stack([x1 - m - g, y0 + m], -1), np.stack([x0 + m, y1 - m - g], -1)], 1)      # (F, 3, 2)
    upper = np.stack([np.stack([x1 - m, y1 - m], -1), np.stack([x0 + m + g, y1 - m], -1), np.stack([x1 - m, y0 + m + g], -1)], 1)
    P = np.where((r % 2 == 1)[:, None, None], upper, lower)
    tri = np.zeros((F, 3, 2))
    rows = np.arange(F)
    for i in range(3):
        tri[rows, (corner.astype(np.int64) + i) % 3] = P[:, i]
    vt = (tri / R).reshape(-1, 2).astype(np.float32)
    report = {"j": j, "D_j": density(j), "histogram": [int(n) for n in hist], "used": texels_needed(hist) / (R * R), "clamped_min": at_min, "clamped_max": at_max}
    return vt, np.arange(3 * F, dtype=np.int32).reshape(F, 3), report


def dilate_ref(ids, albedo, rm, n):
    """-> (albedo, rm) copies with the uncovered texels filled"""
    ids = np.asarray(ids)
    H, W = ids.shape
    out = [np.array(albedo, copy=True), np.array(rm, copy=True)]
    if not 0 <= n <= 4:
        raise AtlasError(f"dilate = {n}: an integer in [0, 4]")
    for r, c in zip(*np.nonzero(ids < 0)):
        best = None
        for rr in range(max(0, r - n), min(H - 1, r + n) + 1):
            for cc in range(max(0, c - n), min(W - 1, c + n) + 1):
                if ids[rr, cc] >= 0:
                    key = ((rr - r) ** 2 + (cc - c) ** 2, rr, cc)
                    if best is None or key < best:
                        best = key
        if best is not None:
            for img, src in zip(out, (albedo, rm)):
                img[r, c] = src[best[1], best[2]]
    return out[0], out[1]
