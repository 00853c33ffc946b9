"""Helper (not a test): the BRDF trainer's shading combine (reference train_brdf_crf.py:195-203 over utils/ops.py:107-118) and its three gradients
restated from the closed form in numpy, in a chosen dtype, with the case tables and the checks that tests/test_shading_cache_cpu.py (the oracle's
shade_cached and the float32 run of this restatement) and tests/test_shading_cache.py (shade_cached_fwd_kernel / shade_cached_bwd_kernel through
ShadingCache.shade and autograd) share.  No torch, nothing taken from oracle/iris_oracle.c.

The combine, per pixel and channel, on the float32 inputs (a albedo, m metallic, d the cached diffuse map, s0 / s1 the cached specular maps at the two
levels r0 <= r1 and the weight w of brdf_ref64.lerp_plan, which is exact float32 arithmetic and so the same for everybody):
    S0 = s0[r0] (1 - w) + s0[r1] w        S1 = s1[r0] (1 - w) + s1[r1] w                                  ops.py:116-118
    kd = a (1 - m)      ks = 0.04 (1 - m) + a m      L = kd d + (ks S0 + S1)                               train_brdf_crf.py:197-203
and, for a cotangent g, from the closed form (no autograd):
    g_albedo    = g (d (1 - m) + S0 m)
    g_metallic  = sum_c g (S0 (a - 0.04) - a d)
    g_roughness = sum_c g (ks (s0[r1] - s0[r0]) + (s1[r1] - s1[r0])) (R - 1) / 0.98      -- 0 where r0 = r1: at a level knot and outside [0.02, 1]
(r0 and r1 are integers: the weight alone carries the derivative, d w / d roughness = (R - 1) / 0.98, ops.py:110-115.)  0.04 and 0.98 are the float32
constants the float32 program holds, in every dtype.

Tolerances, per element, k u (sum of the magnitudes of the terms), u = 2^-24, k the float32 roundings on the longest path of the kernel's expression plus
one for the second-order terms (iris_cache.h):
    L            9 + 1: m1 = 1 - m, 0.04 m1, + a m (ks: 3); w1 = 1 - w, s0a w1, + s0b w (S0: 3); ks S0; + S1; Ld + Ls
                 terms |a m1 d| + (|0.04 m1| + |a m|)(|s0a w1| + |s0b w|) + |s1a w1| + |s1b w|
    g_albedo     6 + 1: S0 (3), g S0, (g S0) m, the sum                          terms |g d m1| + |g| (|s0a w1| + |s0b w|) |m|
    g_metallic   9 + 1: S0 (3), g S0, (g S0) 0.04, + (g d) a, two accumulations over the channels, g_m - g_m1
                 terms sum_c |g| ((|s0a w1| + |s0b w|)(|a| + 0.04) + |a d|)
    g_roughness  11 + 1: ks (3), g ks, s0b - s0a, their product, + g (s1b - s1a), two accumulations, (R - 1), / 0.98
                 terms sum_c |g| ((|0.04 m1| + |a m|)(|s0a| + |s0b|) + |s1a| + |s1b|) (R - 1) / 0.98
tests/test_shading_cache_cpu.py asserts that the oracle and the float32 run of this restatement stay inside the same bounds: that validates the counts.
"""
import functools

import numpy as np

import brdf_ref64 as BR

F32 = np.float32
U = 2.0 ** -24
K_L, K_A, K_M, K_R = 10, 7, 10, 12
F0 = F32(0.04)
SPAN = F32(1.0 - 0.02)
N_ROWS = 4099
LEVELS = (1, 2, 5, 6, 8)
BATCHES = ((1, "permutation"), (63, "permutation"), (65, "repeats"), (1 << 15, "repeats"), (N_ROWS, None))
MUTATIONS = ("r1_is_r0_plus_1", "swap_w", "f0_times_m", "g_metallic_sign")


def batch_id(b):
    return f"B{b[0]}-{b[1] or 'all-rows'}"


def _specials(R):
    """the distinct planted roughness values of brdf_ref64.lerp_case(R): the first 32 n rows of its table hold n values 32 times each"""
    rough = BR.lerp_case(R)["rough"]
    n = 14 + (5 * R if R > 1 else 0)
    block = rough[:32 * n].reshape(n, 32)
    assert (block == block[:, :1]).all()
    return block[:, 0]


@functools.lru_cache(maxsize=None)
def cache_maps(R):
    """the 1 + 2 R maps of a cache of N_ROWS pixels: both signs over e^-3 ... e^6, brdf_ref64.lerp_case's `spec`"""
    spec = BR.lerp_case(R)["spec"]
    rng = np.random.default_rng([7, 700, R])
    d = (rng.normal(size=(N_ROWS, 3)) * np.exp(rng.uniform(-3, 6, (N_ROWS, 1)))).astype(F32)
    s0 = [np.ascontiguousarray(spec[:N_ROWS, j]) for j in range(R)]
    s1 = [np.ascontiguousarray(spec[N_ROWS:2 * N_ROWS, j]) for j in range(R)]
    for a in [d] + s0 + s1:
        a.setflags(write=False)
    return d, s0, s1


def _unit_with_ends(rng, shape):
    """uniform in [0, 1] with exact 0 and exact 1 on an eighth of the entries each"""
    v = rng.random(shape, dtype=F32)
    k = rng.integers(0, 8, shape)
    v[k == 0] = 0
    v[k == 1] = 1
    return v


@functools.lru_cache(maxsize=None)
def case(R, B, idx_mode):
    """roughness: brdf_ref64.lerp_case(R) -- every level knot with two float neighbours on each side, values below 0.02 and above 1, at least 32 rows of
    weight exactly 0 -- whole and shuffled for B = 2^15, its planted values in turn for the short batches"""
    rng = np.random.default_rng([7, 701, R, B])
    full = BR.lerp_case(R)["rough"]
    if B == len(full):
        rough = full[rng.permutation(B)]
    else:
        sp = _specials(R)
        rough = np.concatenate([sp[rng.permutation(len(sp))], full[-max(B - len(sp), 0):][::-1]])[:B] if B > 1 else sp[:1]
        if B > len(sp):
            rough = rough[rng.permutation(B)]
    idx = {None: None, "permutation": rng.permutation(N_ROWS)[:B].astype(np.int64), "repeats": rng.integers(0, N_ROWS, B).astype(np.int64)}[idx_mode]
    if idx_mode == "repeats":
        idx[:2] = idx[2]                                                          # (a repeat for certain, also at B = 65)
    c = {"R": R, "idx": idx, "rough": np.ascontiguousarray(rough.reshape(B, 1)), "albedo": _unit_with_ends(rng, (B, 3)),
         "metallic": _unit_with_ends(rng, (B, 1)), "gL": (rng.normal(size=(B, 3)) * np.exp(rng.uniform(-2, 2, (B, 1)))).astype(F32)}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ============================================================================================================ the restatement
def restate(c, T=np.float64, mut=None, end_level_alone=False):
    """-> {'L' (B,3), 'g_albedo' (B,3), 'g_metallic' (B,), 'g_roughness' (B,)} in T and {...} of tolerances in float64.
    end_level_alone: outside [0.02, 1] the level the roughness is clamped to, without the blend (what L there must be)."""
    R = c["R"]
    d, s0, s1 = cache_maps(R)
    B = c["rough"].shape[0]
    rows = np.arange(N_ROWS) if c["idx"] is None else c["idx"]
    rough = c["rough"].reshape(-1)
    r0, r1, w32 = BR.lerp_plan(rough, R)
    if mut == "r1_is_r0_plus_1":
        r1 = np.where((rough >= F32(0.02)) & (rough <= F32(1)), np.minimum(r0 + 1, R - 1), r1)     # (inside the range: ceil and floor + 1 differ at the knots alone)
    S0m, S1m = np.stack(s0, 1), np.stack(s1, 1)                                   # (n, R, 3)
    a0, b0 = S0m[rows, r0].astype(T), S0m[rows, r1].astype(T)
    a1, b1 = S1m[rows, r0].astype(T), S1m[rows, r1].astype(T)
    w = w32.astype(T)[:, None]
    if end_level_alone:
        out = (rough < F32(0.02)) | (rough > F32(1))
        w = np.where(out[:, None], T(0), w)
    w1 = T(1) - w
    if mut == "swap_w":
        w, w1 = w1, w
    dd = d[rows].astype(T)
    a, m, g = c["albedo"].astype(T), c["metallic"].astype(T), c["gL"].astype(T)
    m1 = T(1) - m
    f0 = T(F0)
    S0, S1 = a0 * w1 + b0 * w, a1 * w1 + b1 * w
    ks = f0 * (m if mut == "f0_times_m" else m1) + a * m
    L = a * m1 * dd + (ks * S0 + S1)
    ga = g * (dd * m1 + S0 * m)
    gm = (g * (S0 * (a - f0) - a * dd)).sum(-1)
    if mut == "g_metallic_sign":
        gm = -gm
    scale = T(R - 1) / T(SPAN)
    gr = (g * (ks * (b0 - a0) + (b1 - a1))).sum(-1) * scale
    f = lambda v: np.abs(v).astype(np.float64)
    mS0, ks_m = f(a0 * w1) + f(b0 * w), f(f0 * m1) + f(a * m)
    tol = {"L": K_L * U * (f(a * m1 * dd) + ks_m * mS0 + f(a1 * w1) + f(b1 * w)),
           "g_albedo": K_A * U * (f(g * dd * m1) + f(g) * mS0 * f(m)),
           "g_metallic": K_M * U * (f(g) * (mS0 * (f(a) + float(F0)) + f(a * dd))).sum(-1),
           "g_roughness": K_R * U * (f(g) * (ks_m * (f(a0) + f(b0)) + f(a1) + f(b1))).sum(-1) * float(scale)}
    return {"L": L, "g_albedo": ga, "g_metallic": gm, "g_roughness": gr}, tol


class Numpy32:
    """the restatement run in float32 (and, with mut, one of its mutations)"""

    def __init__(self, mut=None):
        self.mut, self.name = mut, "numpy-f32" + (f"[{mut}]" if mut else "")

    def shade(self, c):
        o = restate(c, F32, self.mut)[0]
        return o["L"], o["g_albedo"], o["g_metallic"], o["g_roughness"]


class Oracle:
    """oracle.shade_cached on oracle.cache_pack's rows (the oracle has one arithmetic here: both modes are run and must agree)"""

    def __init__(self, oracle_mod, mode):
        self.o, self.mode, self.name = oracle_mod, mode, ("oracle-libm", "oracle-device-arithmetic")[mode]

    def shade(self, c):
        d, s0, s1 = cache_maps(c["R"])
        prev = self.o.get_mode()
        self.o.set_mode(self.mode)
        try:
            rows = self.o.cache_pack(d, s0, s1)
            L, ga, gm, gr = self.o.shade_cached(rows, c["idx"], c["albedo"], c["metallic"], c["rough"], c["gL"])
        finally:
            self.o.set_mode(prev)
        return L, ga, gm.reshape(-1), gr.reshape(-1)


# ============================================================================================================ the check
def check_shade(back, R, batch, log=print):
    """L and the three gradients per element inside their bounds; g_roughness exactly 0 where r0 = r1; L outside [0.02, 1] what the end level alone gives.
    Returns the worst |err| / tol of (L, g_albedo, g_metallic, g_roughness)."""
    B, idx_mode = batch
    c = case(R, B, idx_mode)
    ref, tol = restate(c)
    rough = c["rough"].reshape(-1)
    r0, r1, w = BR.lerp_plan(rough, R)
    if B == 1 << 15:                                                              # the table holds what it is for
        assert set(r0.tolist()) == set(range(R)) and (w == 0).sum() >= 32 and (rough < F32(0.02)).sum() >= 32 and (rough > 1).sum() >= 32
        knots = {float(F32(0.02 + k * 0.98 / (R - 1))) for k in range(R)} if R > 1 else {float(F32(0.02))}
        assert knots <= set(rough.tolist())
        assert (c["metallic"] == 0).any() and (c["metallic"] == 1).any() and (c["albedo"] == 0).any() and (c["albedo"] == 1).any()
        assert (c["gL"] > 0).any() and (c["gL"] < 0).any()
    got = dict(zip(("L", "g_albedo", "g_metallic", "g_roughness"), (np.asarray(a) for a in back.shade(c))))
    worst = {}
    for k in ("L", "g_albedo", "g_metallic", "g_roughness"):
        assert got[k].dtype == F32 and got[k].shape == ref[k].shape, (k, got[k].shape)
        err = np.abs(got[k].astype(np.float64) - ref[k])
        worst[k] = float(np.divide(err, tol[k], out=np.where(err > 0, np.inf, 0.0), where=tol[k] > 0).max())
    log(f"shade[{back.name}, R = {R}, {batch_id(batch)}]: worst |err| / tol  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1, f"shade[{back.name}, R = {R}, {batch_id(batch)}]: {k} outside its bound, worst |err| / tol {v:.3g}"
    flat = r0 == r1
    gr = got["g_roughness"]
    assert (gr[flat] == 0).all(), (f"shade[{back.name}, R = {R}, {batch_id(batch)}]: g_roughness is not 0 at roughness "
                                   f"{rough[flat][gr[flat] != 0][:6].tolist()} (a level knot, or outside [0.02, 1]): {gr[flat][gr[flat] != 0][:6].tolist()}")
    out = (rough < F32(0.02)) | (rough > F32(1))
    if out.any():
        end, etol = restate(c, end_level_alone=True)
        assert (np.abs(got["L"].astype(np.float64) - end["L"])[out] <= etol["L"][out]).all(), f"shade[{back.name}, R = {R}]: L outside [0.02, 1] is not the end level's"
    return worst
