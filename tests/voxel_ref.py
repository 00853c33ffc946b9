"""Helper (not a test): the voxel radiance cache's index and the operations built on it (reference model/slf.py:41-70, slf_bake.py:104-110,
model/emitter.py:180-221) restated in numpy, with the grids, the row tables and the checks that tests/test_voxel_slf_cpu.py (the oracle and this
restatement) and tests/test_voxel_slf.py (the HIP kernels through VoxelSLF, voxel_histogram and SLFEmitter.eval_emitter) share.  tests/test_gbuffer.py
takes its two restatements from here as well.  No torch, nothing taken from oracle/iris_oracle.c.

The index is, by contract, the reference's own float32 expression (model/slf.py:41-54)
    ((x - vmin) / (vmax - vmin) * H).long().clamp(0, H - 1)          vmin = float32(voxel_min), vmax - vmin = float32 of the Python difference
and then inds[z, y, x].  Each step is ONE IEEE float32 operation (the kernels are built with -ffp-contract=off), so the index is EXACT on every row: there is no
tolerance.  The cast is written out, not left to numpy's platform behaviour (cast_int64): truncation toward zero where the value is finite and below
2^63 in magnitude, INT64_MIN otherwise (NaN, +-inf, magnitude >= 2^63: what .long() gives on the reference's platform), then the clip.

The float64 cross-check (check_float64_agreement) says what that contract costs: floor of the same expression in float64 disagrees with the float32 index
only within 4 ulp of a grid plane -- the subtraction's rounding is half an ulp of x - vmin, the quotient and the product add 2 u (x - vmin) -- and on at
most 1 % of the uniformly drawn rows (measured: 1 row in 2^20 in the golden box).  The constructed plane rows are outside that cap: they are there to
disagree.

Sums (scatter_add): per voxel and channel within K u sum |addend|, K the voxel's count, u = 2^-24 -- K - 1 float32 additions in any order, each off by at
most u times a partial sum that the sum of magnitudes bounds (the rule of tests/test_propagation.py).  Counts and histograms are integers: exact.
"""
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24
INT64_MIN = np.iinfo(np.int64).min
B = 1 << 15
ONE_PASS = 8192 * 256                                  # iris_slf_lookup's launch1d: 8192 blocks of 256 threads, then the grid-stride loop
LENGTHS = (1, 63, 64, 65, ONE_PASS + 3)
GRIDS = ((1, -1.0, 5.0), (2, 0.0, 1.0), (31, -0.37, 4.21), (32, -0.37, 4.21), (64, 1000.3, 1004.7), (256, -3.3, 7.9))
HUGE_GRID = 1                                          # (2, 0, 1): f = 2 x, the grid the rows around 2^31 and 2^63 are written for
MUTATIONS = ("h_before_den", "round", "swap_x_z", "threshold_9.2e18")
TRACE_ROUGHNESS = 0.6
NF = 7                                                 # the emitter table of the eval_emitter check: 7 triangles, 3 of them emitters
IS_EMITTER = np.array([0, 1, 0, 0, 1, 0, 1], bool)


def grid_id(gi):
    H, lo, hi = GRIDS[gi]
    return f"H{H}[{lo:g},{hi:g}]"


# ============================================================================================================ the reference
def cast_int64(f):
    """.long() of a float32 array: truncated toward zero if finite and |f| < 2^63, else INT64_MIN"""
    f = np.asarray(f, F32)
    ok = np.isfinite(f) & (np.abs(f) < F32(2.0 ** 63))
    v = np.full(f.shape, INT64_MIN, np.int64)
    v[ok] = np.trunc(f[ok].astype(np.float64)).astype(np.int64)      # (a float32 below 2^63 is an exact double and an exact int64)
    return v


def voxel_coords(x, vmin, vmax, H, mut=None):
    """(B,3) float32 -> (B,3) int64 (x, y, z) cell coordinates: the literal float32 expression.  mut: one of MUTATIONS (for the CPU twin)."""
    x = np.asarray(x, F32)
    lo, den, Hf = F32(vmin), F32(vmax - vmin), F32(H)
    with np.errstate(all="ignore"):
        f = (x - lo) * Hf / den if mut == "h_before_den" else (x - lo) / den * Hf
        if mut == "round":
            f = np.rint(f)
    v = cast_int64(f)
    if mut == "threshold_9.2e18":
        v[~(f < F32(9.2e18))] = INT64_MIN
    q = np.clip(v, 0, H - 1)
    return q[:, ::-1].copy() if mut == "swap_x_z" else q


def np_scatter_add(inds, H, vmin, vmax, x, rgb, kv):
    """model/slf.py:41-61 in numpy: spatial_idx, then sequential scatter_add of radiance and count."""
    q = voxel_coords(x, vmin, vmax, H)
    idx = inds[q[:, 2], q[:, 1], q[:, 0]]
    rad = np.zeros((kv, 3), np.float32); cnt = np.zeros(kv, np.int64)
    np.add.at(rad, idx, rgb); np.add.at(cnt, idx, 1)
    return rad, cnt


def np_voxel_histogram(x, vmin, vmax, H):
    """slf_bake.py:104-110: hist[x + y H + z H H] += 1, viewed (H, H, H) = [z][y][x]"""
    q = voxel_coords(x, vmin, vmax, H)
    lin = q[:, 0] + q[:, 1] * H + q[:, 2] * H * H
    return np.bincount(lin, minlength=H ** 3).astype(np.float32).reshape(H, H, H)


@functools.lru_cache(maxsize=None)
def grid_tables(gi):
    """-> {'mask' (H,H,H) bool [z][y][x], 'inds' int64 as VoxelSLF builds them (model/slf.py:24-31), 'radiance' (kv,3)}.  About 2 % of the H = 256 grid is
    occupied, 60 % of the middle ones; the 2-grid misses one cell, so that both coordinates of every axis are told apart."""
    H = GRIDS[gi][0]
    rng = np.random.default_rng([41, gi])
    if H == 1:
        mask = np.ones((1, 1, 1), bool)
    elif H == 2:
        mask = np.ones((2, 2, 2), bool); mask[0, 1, 0] = False
    else:
        mask = rng.random((H, H, H), dtype=F32) < (0.02 if H >= 256 else 0.6)
    kk, jj, ii = np.nonzero(mask)
    kv = len(ii)
    inds = np.full((H, H, H), -1, np.int64)
    inds[kk, jj, ii] = np.arange(kv)
    rad = (np.abs(rng.normal(size=(kv, 3))) * np.exp(rng.uniform(-3, 3, (kv, 1)))).astype(F32)
    kind = rng.integers(0, 8, kv)                                     # rows whose sum is zero, exactly zero rows, negative rows: the `(r + g) + b > 0` of eval_emitter
    rad[kind == 0] = 0
    rad[kind == 1] = (1.0, -1.0, 0.0)
    rad[kind == 2] *= -1
    if kv >= 4:
        rad[:4] = [[0.5, 0.25, 0.125], [0, 0, 0], [1, -1, 0], [-2, 1, 0.5]]
    out = {"mask": mask, "inds": inds, "radiance": rad}
    for v in out.values():
        v.setflags(write=False)
    return out


def near(x, k):
    """the 2k + 1 float32 values around x, ascending"""
    x = F32(x)
    lo, hi = [x], [x]
    for _ in range(k):
        lo.append(np.nextafter(lo[-1], F32(-np.inf)))
        hi.append(np.nextafter(hi[-1], F32(np.inf)))
    return np.array(lo[:0:-1] + hi, F32)


def planes(gi):
    """the H + 1 grid planes float32(vmin + (vmax - vmin) k / H)"""
    H, lo, hi = GRIDS[gi]
    return (lo + (hi - lo) * np.arange(H + 1) / H).astype(F32)


def huge_values():
    """coordinates of the (2, 0, 1) grid, f = 2 x: f just below and above 2^31, 3e9, inside [9.2e18, 2^63), at 2^63 and above; and their negatives"""
    v = list(near(2.0 ** 30, 1)) + [F32(1.5e9), F32(4.605e18), np.nextafter(F32(2.0 ** 62), F32(0)), F32(4.61e18), F32(2.0 ** 62),
                                    np.nextafter(F32(2.0 ** 62), F32(np.inf)), F32(1e19)]
    return np.array(v + [-a for a in v], F32)


def edge_values(gi):
    """per-axis values: every plane with two float neighbours on either side, vmin and vmax, +-0, a subnormal, +-1e30, +-inf, NaN (and huge_values())"""
    H, lo, hi = GRIDS[gi]
    v = [near(p, 2) for p in planes(gi)] + [np.array([lo, hi, 0.0, -0.0, 2.0 ** -140, -2.0 ** -149, 1e30, -1e30, np.inf, -np.inf, np.nan], F32)]
    if gi == HUGE_GRID:
        v.append(np.repeat(huge_values(), 4))
    return np.concatenate(v)


def _uniform(rng, gi, n, scale):
    H, lo, hi = GRIDS[gi]
    c, h = 0.5 * (lo + hi), 0.5 * scale * (hi - lo)
    return rng.uniform(c - h, c + h, (n, 3)).astype(F32)


def table(gi, n=None):
    """-> (x (n,3) float32, is_random (n,) bool).  n = None: the main table, 2^15 uniform rows over 1.2 x the box and every edge row (one axis at an edge
    value, the others uniform in the box), at shuffled positions.  Given n: a table of exactly that length, edge rows first in line for the short ones."""
    rng = np.random.default_rng([17, gi, n or 0])
    vals = edge_values(gi)
    E = _uniform(rng, gi, 3 * len(vals), 1.0)
    for a in range(3):
        E[a * len(vals):(a + 1) * len(vals), a] = vals
    if n is not None and n < 2 * len(E):
        E = E[rng.permutation(len(E))[:(n + 1) // 2]]
    nr = B if n is None else n - len(E)
    x = np.concatenate([E, _uniform(rng, gi, nr, 1.2)])
    rand = np.concatenate([np.zeros(len(E), bool), np.ones(nr, bool)])
    p = rng.permutation(len(x))
    return x[p], rand[p]


@functools.lru_cache(maxsize=None)
def main_table(gi):
    x, r = table(gi)
    x.setflags(write=False); r.setflags(write=False)
    return x, r


def lookup_ref(gi, x):
    """-> (idx (B,) int64, rgb (B,3) float32): inds[z, y, x] of the exact coordinates; the radiance row, zeros where idx = -1 (model/slf.py:63-70)"""
    H, lo, hi = GRIDS[gi]
    t = grid_tables(gi)
    q = voxel_coords(x, lo, hi, H)
    idx = t["inds"][q[:, 2], q[:, 1], q[:, 0]]
    rgb = np.where((idx >= 0)[:, None], t["radiance"][np.maximum(idx, 0)], F32(0))
    return idx, rgb


def check_float64_agreement(gi, x, is_random):
    """floor of the float64 expression against the float32 index, on the finite rows below 2^31: every disagreement within 4 ulp of a plane, at most 1 % of
    the random rows.  Returns the share among the random rows."""
    H, lo, hi = GRIDS[gi]
    lo32, den32 = float(F32(lo)), float(F32(hi - lo))
    with np.errstate(all="ignore"):
        ok = np.isfinite(x) & (np.abs(x) < 1e8)
        x64 = np.where(ok, x, 0).astype(np.float64)
        f = (x64 - lo32) / den32 * H
        c64 = np.clip(np.floor(f), 0, H - 1).astype(np.int64)
        c32 = voxel_coords(x, lo, hi, H)
        dis = ok & (c64 != c32)
        k = np.clip(np.rint(f), 0, H)
        dist = np.abs(x64 - (lo32 + den32 * k / H))
        ulp = np.spacing(np.maximum(np.abs(x64), np.abs(x64 - lo32)).astype(F32)).astype(np.float64)
    assert (dist[dis] <= 4 * ulp[dis]).all(), f"{grid_id(gi)}: float64 and float32 disagree away from a plane at {x[dis.any(-1)][:4].tolist()}"
    share = float(dis[is_random].any(-1).mean()) if is_random.any() else 0.0
    assert share <= 0.01, f"{grid_id(gi)}: {share:.4f} of the random rows disagree with float64"
    return share


# ============================================================================================================ backends of the CPU twin
class Numpy32:
    """this restatement (and, with mut, one of its mutations) behind the interface the checks use"""
    HANDLES = ("host",)

    def __init__(self, mut=None):
        self.mut, self.name = mut, "numpy-f32" + (f"[{mut}]" if mut else "")

    def _idx(self, gi, x):
        H, lo, hi = GRIDS[gi]
        q = voxel_coords(x, lo, hi, H, self.mut)
        return q, grid_tables(gi)["inds"][q[:, 2], q[:, 1], q[:, 0]]

    def lookup(self, gi, x, handle):
        idx = self._idx(gi, x)[1]
        rad = grid_tables(gi)["radiance"]
        return idx, np.where((idx >= 0)[:, None], rad[np.maximum(idx, 0)], F32(0))

    def scatter_add(self, gi, x, rgb):
        idx = self._idx(gi, x)[1]
        kv = len(grid_tables(gi)["radiance"])
        keep = idx >= 0
        rad = np.zeros((kv, 3), F32); cnt = np.zeros(kv, np.int64)
        np.add.at(rad, idx[keep], rgb[keep]); np.add.at(cnt, idx[keep], 1)
        return rad, cnt

    def histogram(self, gi, x):
        H = GRIDS[gi][0]
        q = self._idx(gi, x)[0]
        return np.bincount(q[:, 0] + q[:, 1] * H + q[:, 2] * H * H, minlength=H ** 3).astype(F32).reshape(H, H, H)

    def eval_emitter(self, gi, x, tri, rough, trace_roughness):
        return eval_emitter_ref(gi, x, tri, rough, trace_roughness, self.lookup(gi, x, "host")[1])


class Oracle:
    """oracle.VoxelSLF / oracle.SLFEmitter (no pooling there: scatter_add and histogram are the restatement's and the kernels' alone)"""
    HANDLES = ("host",)

    def __init__(self, oracle_mod, mode):
        self.o, self.mode, self.name, self._slf = oracle_mod, mode, ("oracle-libm", "oracle-device-arithmetic")[mode], {}

    def slf(self, gi):
        if gi not in self._slf:
            t = grid_tables(gi)
            self._slf = {gi: self.o.VoxelSLF(t["inds"], t["radiance"], GRIDS[gi][1], GRIDS[gi][2])}      # (one at a time: the 256-grid is 128 MiB)
        return self._slf[gi]

    def _in_mode(self, fn):
        prev = self.o.get_mode()
        self.o.set_mode(self.mode)
        try:
            return fn()
        finally:
            self.o.set_mode(prev)

    def lookup(self, gi, x, handle):
        s = self.slf(gi)
        return self._in_mode(lambda: (s.spatial_idx(x), s.forward(x)))

    def eval_emitter(self, gi, x, tri, rough, trace_roughness):
        em = emitter_tables()
        e = self.o.SLFEmitter(IS_EMITTER, em["radiance"], em["area"], self.slf(gi))
        return self._in_mode(lambda: e.eval_emitter(x, tri, rough, trace_roughness))


# ============================================================================================================ the checks
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def check_lookup(back, gi, x, log=print):
    """spatial_idx exact; forward the exact radiance row (bits), exact zeros for -1; every handle of the backend alike"""
    idx, rgb = lookup_ref(gi, x)
    for h in back.HANDLES:
        gi_, gr = back.lookup(gi, x, h)
        gi_, gr = np.asarray(gi_), np.asarray(gr)
        assert gi_.dtype == np.int64 and gi_.shape == idx.shape and gr.shape == rgb.shape
        bad = gi_ != idx
        assert not bad.any(), (f"spatial_idx[{back.name}, {grid_id(gi)}, {h}, {len(x)} rows]: {int(bad.sum())} rows differ, first at rows "
                               f"{np.nonzero(bad)[0][:4].tolist()}: x = {x[bad][:4].tolist()}, got {gi_[bad][:4].tolist()}, want {idx[bad][:4].tolist()}")
        assert (_bits(gr) == _bits(rgb)).all(), f"forward[{back.name}, {grid_id(gi)}, {h}]: radiance rows differ"
    log(f"lookup[{back.name}, {grid_id(gi)}, {len(x)} rows]: exact on {'/'.join(back.HANDLES)}; {int((idx < 0).sum())} rows in empty voxels")


@functools.lru_cache(maxsize=None)
def scatter_case(gi):
    x = main_table(gi)[0]
    rng = np.random.default_rng([23, gi])
    rgb = (rng.normal(size=(len(x), 3)) * np.exp(rng.uniform(-3, 3, (len(x), 1)))).astype(F32)
    rgb.setflags(write=False)
    return x, rgb


def check_scatter_add(back, gi, log=print):
    x, rgb = scatter_case(gi)
    idx = lookup_ref(gi, x)[0]
    kv = len(grid_tables(gi)["radiance"])
    keep = idx >= 0
    cnt = np.bincount(idx[keep], minlength=kv)
    ref = np.zeros((kv, 3)); mag = np.zeros((kv, 3))
    np.add.at(ref, idx[keep], rgb[keep].astype(np.float64)); np.add.at(mag, idx[keep], np.abs(rgb[keep]).astype(np.float64))
    got, gcnt = back.scatter_add(gi, x, rgb)
    got, gcnt = np.asarray(got, np.float64), np.asarray(gcnt)
    assert 0 < keep.sum() and (gi == 0 or keep.sum() < len(x))                    # rows in empty voxels are in the table ...
    assert np.array_equal(gcnt, cnt), f"scatter_add[{back.name}, {grid_id(gi)}]: counts differ"          # ... and are dropped: the counts are exact
    tol = cnt[:, None] * U * mag
    err = np.abs(got - ref)
    worst = float(np.divide(err, tol, out=np.where(err > 0, np.inf, 0.0), where=tol > 0).max())
    log(f"scatter_add[{back.name}, {grid_id(gi)}]: {int(keep.sum())} of {len(x)} rows kept, largest count {int(cnt.max())}, worst |err| / tol {worst:.3f}")
    assert (err <= tol).all(), f"scatter_add[{back.name}, {grid_id(gi)}]: worst |err| / tol {worst:.3g}"
    return worst


@functools.lru_cache(maxsize=None)
def histogram_case(gi):
    """the main table and an asymmetric cloud: x over the whole box, y over its lower two thirds, z over its lower third"""
    H, lo, hi = GRIDS[gi]
    rng = np.random.default_rng([29, gi])
    c = rng.uniform(0, 1, (B, 3)) * np.array([1.0, 0.66, 0.33])
    x = np.concatenate([main_table(gi)[0], (lo + (hi - lo) * c).astype(F32)])
    x.setflags(write=False)
    return x


def check_histogram(back, gi, log=print):
    H, lo, hi = GRIDS[gi]
    x = histogram_case(gi)
    ref = np_voxel_histogram(x, lo, hi, H)
    got = np.asarray(back.histogram(gi, x))
    assert got.shape == (H, H, H) and got.dtype == F32
    assert np.array_equal(got, ref), f"voxel_histogram[{back.name}, {grid_id(gi)}]: {int((got != ref).sum())} cells differ"
    if H > 2:                                                                     # the cloud is asymmetric: a swapped axis is another histogram
        assert not np.array_equal(ref, ref.transpose(2, 1, 0)) and not np.array_equal(ref, ref.transpose(0, 2, 1)) and not np.array_equal(ref, ref.transpose(1, 0, 2))
    log(f"voxel_histogram[{back.name}, {grid_id(gi)}]: exact, {int((ref > 0).sum())} of {H ** 3} cells hit, largest count {int(ref.max())}")


@functools.lru_cache(maxsize=None)
def emitter_tables():
    """`emitter.pth` of the eval_emitter check: NF triangles, K = 3 emitters with areas and radiance rows; emitter_pdf = 1 / K"""
    K = int(IS_EMITTER.sum())
    out = {"radiance": np.array([[3.0, 2.0, 1.0], [0.0, 0.0, 0.0], [0.5, 0.25, 4.0]], F32), "area": np.array([0.5, 2.0, 1e-13], F32),
           "verts": np.zeros((K, 3, 3), F32)}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emitter_case(gi):
    """the main table's points with a triangle each (a miss -1, non-emitters, emitters, negative indices in [-NF, -1) that wrap) and a roughness each,
    some of them trace_roughness itself"""
    x = main_table(gi)[0]
    rng = np.random.default_rng([31, gi])
    tri = rng.choice(np.array([-1, 0, 0, 2, 2, 3, 5, 5, 1, 4, 6, -NF, -2, -4, -3], np.int64), len(x))
    rough = rng.uniform(0.02, 1.0, len(x)).astype(F32)
    rough[rng.permutation(len(x))[:64]] = F32(TRACE_ROUGHNESS)
    for a in (tri, rough):
        a.setflags(write=False)
    return x, tri, rough


def eval_emitter_ref(gi, x, tri, rough, trace_roughness, slf_rgb):
    """model/emitter.py:180-221 on the rows slf_rgb the lookup gives: (Le (B,3), emit_pdf (B,1), valid_next (B,))"""
    em = emitter_tables()
    vis = tri != -1
    is_area = IS_EMITTER[tri] & vis                                               # (a negative index wraps, as the reference's tensor indexing does)
    e_idx = (np.cumsum(IS_EMITTER) - 1)[tri]
    Le = np.zeros((len(x), 3), F32); pdf = np.zeros((len(x), 1), F32)
    Le[is_area] = em["radiance"][e_idx[is_area]]
    pdf[is_area, 0] = (F32(1) / F32(len(em["area"]))) / np.maximum(em["area"][e_idx[is_area]], F32(1e-12))
    valid_next = ~is_area & vis
    if rough is not None:
        diffuse = ~is_area & vis & (rough > F32(trace_roughness))                 # strict: a row at trace_roughness itself looks nothing up
        Le[diffuse] = slf_rgb[diffuse]
        lit = (slf_rgb[:, 0] + slf_rgb[:, 1]) + slf_rgb[:, 2] > 0
        valid_next &= ~(diffuse & lit)
    return Le, pdf, valid_next


def check_eval_emitter(back, gi, log=print):
    x, tri, rough = emitter_case(gi)
    Le, pdf, vn = eval_emitter_ref(gi, x, tri, rough, TRACE_ROUGHNESS, lookup_ref(gi, x)[1])
    at = rough == F32(TRACE_ROUGHNESS)
    surf = (tri != -1) & ~IS_EMITTER[tri]
    assert (at & surf).sum() >= 8 and (Le[at & surf] == 0).all() and vn[at & surf].all()
    gLe, gpdf, gvn = (np.asarray(a) for a in back.eval_emitter(gi, x, tri, rough, TRACE_ROUGHNESS))
    assert (_bits(gLe) == _bits(Le)).all(), f"eval_emitter[{back.name}, {grid_id(gi)}]: Le differs on {int((_bits(gLe) != _bits(Le)).any(-1).sum())} rows"
    assert (_bits(gpdf.reshape(-1, 1)) == _bits(pdf)).all(), f"eval_emitter[{back.name}, {grid_id(gi)}]: emit_pdf differs"
    assert np.array_equal(gvn.astype(bool), vn), f"eval_emitter[{back.name}, {grid_id(gi)}]: valid_next differs"
    log(f"eval_emitter[{back.name}, {grid_id(gi)}]: exact; {int((surf & (rough > F32(TRACE_ROUGHNESS))).sum())} rows read the cache, {int(vn.sum())} go on")
