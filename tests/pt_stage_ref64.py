"""Helper (not a test): the path tracer's MIS stages restated per path from their formulas in numpy, in a chosen dtype -- utils/path_tracing.py:357-382
and :394-404 (path_tracing_single: g_eps, pdf_eps, mis_eps = 1e-6, 1e-6, 1e-6), :443-461 and :476-486 (trace_indirect: 1e-12, 1e-12, no MIS clamp),
model/emitter.py:180-221 (eval_emitter with and without a roughness), model/slf.py:41-70 -- with the inputs, the branch table and the checks that
tests/test_pt_stage_ref64_cpu.py (the oracle in both modes and the float32 run of this restatement) and tests/test_pt_stage_ref64.py (the HIP kernels)
share.  numpy only; nothing is taken from oracle/iris_oracle.c.  The float64 formulas are themselves held to the reference's own Python run in float64, per path,
to 1e-12 (tests/golden/pt_stage_ref.npz, test_pt_stage_ref64_cpu.py::test_restatement_is_the_references_*).

Stage-wise continuation.  What earlier files pin is taken from the code under test as the float32 values it works with (exact in float64):
wi / emit_pdf / emit_triangle_idx from its sample_emitter on the same draws (tests/brdf_ref64.py); wi / pdf / weight / position_next / normal_next /
triangle_next from its BRDF-sampling stage (brdf_ref64.py, hit_ref64.py).  The visibility ray's hit is NOT taken from it: it is decided by
hit_ref64.exact_hits over all triangles, from the origin x + RayEpsilon * wi formed in float32 as the kernel forms it (one product, one sum per
component).  eval_brdf's brdf and pdf are brdf_ref64.cosines / f_brdf.

Perturbation envelope of the emitter-sampling stage (coef1), per element, as brdf_ref64.envelope builds it.  f = f(c, den, d^2, |cos|): the four cosines
c, the GGX denominator, and d^2 = |p* - x|^2 and |cos| = |wi . N| of the geometry term at the exact hit p* with the exact normal N.
    tol = 64 u |f| + sum_i max|f(c +- 8 u e_i) - f| + max|f(den +- 4 u) - f| + max|f(d^2 +- dd2) - f| + max|f(|cos| +- dcos) - f| + 2^-100
    dd2  = 2 |p* - x|_1 C_p unit_p + 3 (C_p unit_p)^2 + 4 u d^2          dcos = sqrt(3) C_n unit_n + 4 u
C_p unit_p and C_n unit_n are what hit_ref64 allows the hit position and the normal (hit_ref64.measured(), units of the hit triangle and this ray); 4 u d^2
and 4 u are the float32 roundings of the three-term sums.  64 u counts the roundings after them, u |result| for each operation: 16 u for brdf (brdf_ref64), 2 u for G and
G / max(emit_pdf, eps), 2 u for the two products with brdf, and for w_mis, whose relative sensitivity to brdf_pdf is at most 2, 2 (16 + 2) u for brdf_pdf = pdf G and
4 u for its own two squares, sum and quotient: 60 u, rounded up.  2^-100 stands for float32 products that underflow.  A row whose box holds the pole of D_GGX (brdf_ref64.envelope) has
tol = inf and is counted.
The finish stage and iris_pt_apply are pure functions of float32 arguments: tol = 8 u |f| + 2^-100 for coef2 / const2 (two squares, a sum and a quotient
for w_mis, up to two products after it: 6 u, rounded up), and 3 u |t| (|cst| + |coef radiance|) + u (|L| + |v|) for the accumulated row of apply (a product, a sum
and a product for v, u |result| each, and the sum into L).

Float32 overflow is part of the reference value: where brdf_pdf or emit_pdf^2 + brdf_pdf^2 exceeds FLT_MAX the float32 formula has inf there, and
`~brdf_pdf.isinf()` or e^2 / inf gives w_mis = 0; the float64 run substitutes inf above FLT_MAX, and such rows are not excluded (a row whose box straddles
FLT_MAX has a tolerance as large as its value, by the envelope).  Through a traced ray it cannot happen away from the pole of D_GGX, though: the hit lies at
least RayEpsilon from x, so G <= 1.25e8 even under g_eps = 1e-12, pdf <= D / (4 * 1e-4) <= 5e9 at r = 0.02, and brdf_pdf^2 <= 4e35 < FLT_MAX.

The constants.  E is the worst |err| / tol of the float32 run of this restatement and of the libm oracle against float64 on an input and variant, measured
when the tests run; the code under test must stay within C = 4 E on that input (hit_ref64.constants' rule), and E above 1 fails as a fault of the
envelope's derivation.  Measured on the machine this was written on, the largest over the inputs and variants:
    emitter-sampling stage E = 0.149 (box 0.10, open scenes 0.14 .. 0.149)      finish stage E = 0.383 (synthetic table 0.19)
    apply: the bound is derived, not measured; the worst |err| / tol is 0.91
A row outside its envelope is a finding, not a reason to widen these.

Discrete outputs (e1; e2, valid_next) are equal exactly on every decided row.  A row is undecided for one of four reasons, counted by reason:
    edge       the exact geometry puts a crossing that could be the visibility hit within C_b unit_b of a triangle edge (or within C_t unit_t of t = 0)
    second     a second triangle's t lies within C_t (unit_t + unit_t') of the hit's
    cdf        s1 within one ulp of a cdf entry
    threshold  the float32 and the float64 sum of the cache row disagree about `> 0`, or (never, the comparison is of two float32 values) the roughness test
At most 2 % of any input may be undecided (CAP), from the float64 reference alone.

Branches whose two sides cannot differ in an output (not tested; UNOBSERVABLE):
    nee  brdf_pdf == 0 -> w_mis = 1      brdf_pdf = pdf G is 0 only where NoL = 0 (then brdf = 0) or |cos| = 0 (then G = 0): coef1 = 0 either way
    nee  emit_pdf > 0  (and `>=`)        emit_pdf = (1/K) / max(area, 1e-12) > 0 always; with an infinite area, e = 0 gives e^2 / den = 0 = the other side
    nee  emit_pdf.isinf()                unreachable: area is clamped at 1e-12
    nee  brdf_pdf^2 overflows            unreachable through a ray, see above
    nee  d^2 < 1e-12                     unreachable through a ray: the hit lies at least RayEpsilon (8.9e-5) from x, d^2 >= 7.9e-9
    finish  d^2 < g_eps, and G itself    G = 1 where the hit is an emitter (valid_next false), and elsewhere emit_pdf = 0 sets w_mis = 1 whatever brdf_pdf is
    finish  brdf_pdf > 0 (and `>=`)      brdf_pdf = 0 gives 0 / e^2 = 0 = the other side (e > 0 on an emitter)
    finish  w_mis in const2              const2 != 0 only on a surface hit, where emit_pdf = 0 sets w_mis = 1 (eval_emitter never adds the cache to an emitter's Le)
(G selected by "hit" instead of valid_next IS observable: an emitter hit then carries G != 1 into w_mis.)
"""
import functools

import numpy as np

import brdf_ref64 as R
import hit_ref64 as H

F32, F64, U = np.float32, np.float64, 2.0 ** -24
RAY_EPS = F32(1500 * 2.0 ** -24)                       # mitsuba.math.RayEpsilon in float32
FLT_MAX = float(np.finfo(F32).max)
VARIANTS = {"single": (F32(1e-6), F32(1e-6), F32(1e-6)), "indirect": (F32(1e-12), F32(1e-12), F32(0.0))}
C_ROUND_NEE, C_ROUND_FINISH, FLOOR = 64.0, 8.0, 2.0 ** -100
CAP = 0.02
MIN_SIDE = 8
ROW_COUNTS = (1, 63, 64, 65, 257, None)
UNOBSERVABLE = ("nee brdf_pdf == 0", "nee emit_pdf > 0", "nee emit_pdf.isinf()", "nee brdf_pdf^2 overflows", "nee d2 < 1e-12", "finish d2 < g_eps", "finish brdf_pdf > 0", "finish w_mis in const2")


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ============================================================================================================ the radiance cache, model/slf.py:41-70
def slf_tables(Hn, vmin, vmax):
    """An Hn^3 grid with every class of voxel in a fixed pattern: 0 empty, 1 zero radiance, 2 the row (1, -1, 0) (its sum is 0: the path goes on, yet
    const2 is not 0), 3 a positive row.  inds is [z][y][x] with -1 = empty, rows numbered as torch.where(mask) orders them."""
    z, y, x = np.meshgrid(np.arange(Hn), np.arange(Hn), np.arange(Hn), indexing="ij")
    cls = (x + 2 * y + 3 * z) % 4
    mask = cls > 0
    kk, jj, ii = np.nonzero(mask)
    inds = np.full((Hn, Hn, Hn), -1, np.int64)
    inds[kk, jj, ii] = np.arange(len(ii))
    c = cls[kk, jj, ii]
    rng = np.random.default_rng(77)
    rad = np.zeros((len(ii), 3), F32)
    rad[c == 2] = (1.0, -1.0, 0.0)
    rad[c == 3] = rng.uniform(0.05, 2.0, (int((c == 3).sum()), 3)).astype(F32)
    return {"H": Hn, "mask": mask, "inds": inds, "radiance": rad, "vmin": float(vmin), "vmax": float(vmax), "cls": cls}


def slf_lookup(slf, p32, T=F32):
    """-> (row index or -1, rgb (B, 3) float32).  x_ = (x - voxel_min) / (voxel_max - voxel_min); (x_ * H).long().clamp(0, H - 1): float32 operations on a float32
    tensor and Python scalars, each IEEE exact, so float32 IS the reference here (T = float64: a float64 run of the reference)"""
    vmin, den, Hn = T(slf["vmin"]), T(slf["vmax"] - slf["vmin"]), slf["H"]
    with np.errstate(all="ignore"):
        q = (p32.astype(T) - vmin) / den * T(Hn)
        q = np.where(np.isfinite(q), q, -1.0)                     # (.long() of a non-finite value is INT64_MIN on the reference's platform: clamped to 0)
    i = np.clip(np.trunc(q).astype(np.int64), 0, Hn - 1)
    j = slf["inds"][i[:, 2], i[:, 1], i[:, 0]]
    rgb = np.where((j >= 0)[:, None], slf["radiance"][np.maximum(j, 0)], F32(0))
    return j, rgb.astype(F32)


# ============================================================================================================ inputs
def _emitter_tables(key, tri_verts, is_emitter, area):
    K = int(is_emitter.sum())
    pdf = F32(1) / F32(K)                                           # NF.normalize(ones(K), p=1)
    return {"key": key, "K": K, "verts": np.ascontiguousarray(tri_verts[is_emitter], F32), "area": np.asarray(area, F32), "is_emitter": is_emitter,
            "triangle_idx": np.nonzero(is_emitter)[0].astype(np.int64), "emitter_pdf": pdf, "cdf": np.cumsum(np.full(K, pdf, F32), dtype=F32)}


def _rows(rng, pos, nrm, pick=None, K=1, s2=None):
    """materials, directions and draws for the shading points; pick: the emitter ordinal each row's s1 selects (None: uniform draws)"""
    n = len(pos)
    nrm = np.ascontiguousarray(nrm, F32)
    albedo, metal = R._materials(rng, n)
    s1 = rng.random(n, dtype=F32) if pick is None else ((pick + 0.1 + 0.8 * rng.random(n)) / K).astype(F32)
    rn = np.array([0.02, 0.412, F32(0.6), np.nextafter(F32(0.6), F32(1)), 0.804], F32)
    return {"pos": np.ascontiguousarray(pos, F32), "nrm": nrm, "wo": _directions(rng, nrm), "albedo": albedo, "metal": metal,
            "rough": np.array(R.ROUGH_LEVELS, F32)[rng.integers(0, len(R.ROUGH_LEVELS), n)], "s1": s1,
            "s2": rng.random((n, 2), dtype=F32) if s2 is None else np.ascontiguousarray(s2, F32),
            "s1b": rng.random(n, dtype=F32), "s2b": rng.random((n, 2), dtype=F32), "rough_next": rn[rng.integers(0, len(rn), n)]}


def _directions(rng, n32):
    d = n32.astype(F64) + 0.8 * rng.normal(size=n32.shape)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)


E0 = np.array([[-0.5, -0.5, 2.5], [0.75, -0.5, 2.5], [-0.5, 0.75, 2.5]])
TINY = 2.0 ** -17
LIFT = 2.0 ** -10      # the "floor" points float this far above it: at scale 2^9 a float32 coordinate of 2000 resolves 1.2e-4 > RayEpsilon, so a point ON the floor is within the
                       # closest hit's own tolerance of hitting the floor at t = 0 -- undecided by the exact geometry, for the reference as for any float32 tracer


def _open_scene(k=0):
    """floor (0, 1); an occluder at z = 1 (2, 3); emitters: E0 (4), E1 behind it at z = 3 (5), a triangle of side 2^-17 and area 2.9e-11 just above the floor (6), two
    whose table area is 1e7 and 1e13 (7, 8: emit_pdf 1.7e-8 and 1.7e-14, below both pdf_eps) and one with table area 0 (9: the area clamp, emit_pdf 1.7e11).  emitter_area is a table the model loads and the stages read; they never recompute it.  Everything scaled by 2^k, exactly."""
    t = np.array([[[-4, -4, 0], [4, -4, 0], [4, 4, 0]], [[-4, -4, 0], [4, 4, 0], [-4, 4, 0]],
                  [[-1.5, -1, 1], [0.5, -1, 1], [0.5, 1, 1]], [[-1.5, -1, 1], [0.5, 1, 1], [-1.5, 1, 1]],
                  E0, [[-1, -1, 3], [1.5, -1, 3], [-1, 1.5, 3]],
                  [[0, 0, 2.0 ** -5], [TINY, 0, 2.0 ** -5], [0, TINY, 2.0 ** -5]],
                  [[2, -3, 2], [3.5, -3, 2], [2, -1.5, 2]], [[-3.5, 1.5, 2.25], [-2, 1.5, 2.25], [-3.5, 3, 2.25]],
                  [[2, 2, 2.5], [3, 2, 2.5], [2, 3, 2.5]]], F64)
    is_emitter = np.zeros(len(t), bool)
    is_emitter[4:] = True
    area = np.array([0.78125, 3.125, 0.5 * TINY * TINY, 1e7, 1e13, 0.0])
    s = 2.0 ** k
    rng = np.random.default_rng(5)
    P, Nn, pick, S2 = [], [], [], []
    up = np.array([0.0, 0.0, 1.0])

    def add(p, n, e, s2=None):
        P.append(p); Nn.append(np.broadcast_to(n, p.shape)); pick.append(e)
        S2.append(rng.random((len(p), 2)) if s2 is None else s2)
    others = np.array([0, 1, 3, 4, 5])
    n = 1400                                                                           # on the floor, a fifth of them under the occluder
    add(np.stack([rng.uniform(-3.5, 3.5, n), rng.uniform(-3.5, 3.5, n), np.full(n, LIFT)], -1), up, others[rng.integers(0, 5, n)])
    n = 300                                                                            # anywhere, above the emitters too, any normal
    nr = rng.normal(size=(n, 3))
    add(np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(0.2, 3.5, n)], -1), nr / np.linalg.norm(nr, axis=-1, keepdims=True), others[rng.integers(0, 5, n)])
    n = 400                                                                            # next to the tiny emitter, sampling it
    a, r = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.02, 0.06, n)
    add(np.stack([r * np.cos(a), r * np.sin(a), np.full(n, LIFT)], -1), up, np.full(n, 2))
    # below E0, the sample aimed at the point above: d^2 < 1e-6; from 1e-7 the ray starts beyond E0 and meets E1.  Below the emitter of area 1e7, which has nothing
    # above it: the ray starts beyond it and leaves the scene
    # (scaled up, float32 no longer resolves 5e-5 at z = 1024: those rows would all be undecided, so they stay at the distance of the first group there)
    for em_i, lo, hi, n in ((0, 2e-4, 9e-4, 300), (0, 1e-4, 1e-4, 100), (0, 1e-7, 1e-7, 100), (3, 1e-7, 5e-5, 100) if k <= 0 else (3, 2e-4, 9e-4, 100)):
        b = rng.dirichlet([2.0, 2.0, 2.0], n)
        tg = b @ t[4 + em_i]
        dz = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
        add(tg - np.stack([rng.normal(scale=0.2, size=n) * dz, rng.normal(scale=0.2, size=n) * dz, dz], -1), up, np.full(n, em_i),
            np.stack([(1 - b[:, 0]) ** 2, b[:, 1] / (1 - b[:, 0])], -1))               # u = 1 - sqrt(u0) = b0, v = sqrt(u0) u1 = b1
    n = 200                                                                            # far away: G 1e-3, e^2 + brdf_pdf^2 < 1e-6 with the large emitters
    a, r = rng.uniform(0, 2 * np.pi, n), rng.uniform(20, 30, n)
    add(np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(0, 1, n)], -1), up, np.array([3, 4])[rng.integers(0, 2, n)])
    tv = (t * s).astype(F32)
    assert (tv.astype(F64) == t * s).all()
    pos = (np.concatenate(P) * s).astype(F32)
    rows = _rows(rng, pos, np.concatenate(Nn), np.concatenate(pick), 6, np.minimum(np.concatenate(S2), float(R.TOP)))
    verts, faces = np.ascontiguousarray(tv.reshape(-1, 3)), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)
    return {"name": f"open*2^{k}", "verts": verts, "faces": faces, "geom": H.Geometry(verts, faces), "is_emitter": is_emitter,
            "em": _emitter_tables(("open", k), tv, is_emitter, area), "slf": slf_tables(8, -4.0 * s, 4.0 * s), "rows": _frozen(rows)}


def _box_scene():
    from conftest import golden
    g = golden("bake_box.npz")
    verts, faces, is_emitter = g["verts"].astype(F32), g["faces"].astype(np.int32), g["is_emitter"].astype(bool)
    keep = g["prim_valid"] & ~is_emitter[np.maximum(g["prim_idx"], 0)]
    rng = np.random.default_rng(6)
    rows = _rows(rng, g["prim_position"][keep], g["prim_normal"][keep])
    rows["wo"] = np.ascontiguousarray(-g["rays_d"][keep], F32)
    slf = {"H": int(g["slf_inds"].shape[0]), "mask": g["slf_mask"], "inds": g["slf_inds"], "radiance": g["slf_radiance"], "vmin": float(g["voxel_min"]), "vmax": float(g["voxel_max"])}
    return {"name": "box", "verts": verts, "faces": faces, "geom": H.Geometry(verts, faces), "is_emitter": is_emitter,
            "em": _emitter_tables(("box",), verts[faces], is_emitter, g["emitter_area"]), "slf": slf, "rows": _frozen(rows)}


SCENES = ("box", "open", "open/128", "open*512")


@functools.lru_cache(maxsize=None)
def scene(name):
    sc = _box_scene() if name == "box" else _open_scene({"open": 0, "open/128": -7, "open*512": 9}[name])
    assert len(sc["faces"]) <= 64 and len(sc["rows"]["pos"]) <= 4096
    sc["ord_of"] = np.where(sc["is_emitter"], np.cumsum(sc["is_emitter"]) - 1, -1).astype(np.int64)
    return sc


def head(rows, n):
    return rows if n is None else {k: v[:n] for k, v in rows.items()}


PDFS = (0.0, 1e-40, 1.0, 9e4, np.inf, np.nan)
D2S = (0.25e-12, 4e-12, 0.25e-6, 4e-6, 1.0)
ROUGHS = (F32(-0.25), F32(0.0), F32(0.412), F32(0.6), np.nextafter(F32(0.6), F32(1)), F32(0.9))
TRI_CLASSES = ("miss", "emitter", "empty", "zero", "1-10", "positive")


@functools.lru_cache(maxsize=None)
def finish_table():
    """The finish stage's argument classes crossed, on the open scene's emitter and cache tables, without tracing: the hit (a miss, an emitter -- all six in turn --,
    the floor over an empty / zero / (1, -1, 0) / positive voxel) x roughness_next (below, at and above 0 and 0.6) x pdf (PDFS) x d^2 (on both sides of 1e-12 and
    1e-6) x weight (positive, with zeros).  position_next sits at a voxel centre, so the voxel is the same in every arithmetic."""
    sc = scene("open")
    rng = np.random.default_rng(8)
    grid = np.stack(np.meshgrid(range(6), range(6), range(6), range(5), range(2), indexing="ij"), -1).reshape(-1, 5)
    n = len(grid)
    tc, ri, pi, di, wi_ = grid.T
    layer = sc["slf"]["cls"][4]                                     # z in [0, 1): (z + 4) / 8 * 8 = 4
    pn = np.zeros((n, 3))
    tri = np.zeros(n, np.int64)
    for c, want in ((2, 0), (3, 1), (4, 2), (5, 3)):
        ys, xs = np.nonzero(layer == want)
        m = np.nonzero(tc == c)[0]
        j = rng.integers(0, len(xs), len(m))
        pn[m] = np.stack([xs[j] - 4 + 0.5, ys[j] - 4 + 0.5, np.full(len(m), 0.5)], -1)     # (a point above the floor: the stage does not ask that it lie on the triangle)
    m = np.nonzero(tc == 1)[0]
    tri[m] = 4 + np.arange(len(m)) % 6
    pn[m] = sc["verts"].astype(F64).reshape(-1, 3, 3)[tri[m]].mean(1)
    tri[tc == 0] = -1
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    pn32 = pn.astype(F32)
    x = (pn32.astype(F64) + np.sqrt(np.array(D2S))[di][:, None] * d).astype(F32)
    nn = rng.normal(size=(n, 3))
    nn = (nn / np.linalg.norm(nn, axis=-1, keepdims=True)).astype(F32)
    w = rng.uniform(0.1, 3.0, (n, 3)).astype(F32)
    w[wi_ == 1] *= (rng.random((int((wi_ == 1).sum()), 3)) > 0.5).astype(F32)
    with np.errstate(all="ignore"):
        pdf = np.array(PDFS, F64).astype(F32)[pi]
    p = rng.permutation(n)
    tb = {"pos": x, "pos_next": pn32, "nrm_next": nn, "wi": (-d).astype(F32), "tri_next": tri, "rough_next": np.array(ROUGHS, F32)[ri], "pdf": pdf, "weight": w,
          "tri_class": tc, "d2_class": di}
    return _frozen({k: np.ascontiguousarray(v[p]) for k, v in tb.items()})


@functools.lru_cache(maxsize=None)
def apply_table():
    rng = np.random.default_rng(9)
    n, M, K = 1000, 1300, 6
    tb = {"L": rng.uniform(0, 2, (M, 3)).astype(F32), "rows": rng.permutation(M)[:n].astype(np.int32), "throughput": rng.uniform(0, 2, (n, 3)).astype(F32),
          "radiance": rng.uniform(0, 50, (K, 3)).astype(F32), "e": rng.integers(-1, K, n).astype(np.int32), "coef": rng.uniform(-1, 4, (n, 3)).astype(F32),
          "cst": rng.uniform(0, 3, (n, 3)).astype(F32), "weight": (rng.uniform(0, 2, (n, 3)) * (rng.random((n, 3)) > 0.2)).astype(F32)}
    tb["cst"][::37, 0] = np.nan
    tb["coef"][5::41, 1] = np.inf
    tb["throughput"][7::43, 2] = np.nan
    tb["throughput"][11::47, 0] = 0.0                               # 0 * inf, 0 * nan
    tb["coef"][11::47, 0] = np.inf
    return _frozen(tb)


APPLY_CASES = tuple((nz, drop) for nz in (1, 0) for drop in (None, "rows", "throughput", "e", "cst", "weight"))


# ============================================================================================================ the formulas, in T
def nee_formula(c, dden, d2, cosv, hit, visible, epdf32, rows, variant, T=F64):
    """utils/path_tracing.py:369-382 / :447-459 after the visibility ray -> coef (N, 3) with term1 = coef * radiance[e1], and the branch masks"""
    g_eps, pdf_eps, mis_eps = (T(v) for v in variant)
    with np.errstate(all="ignore"):
        v = R.f_brdf(c, rows["rough"], rows["albedo"], rows["metal"], T, dden)
        G = np.where(hit, np.asarray(cosv, T) / np.maximum(np.asarray(d2, T), g_eps), T(1))
        bp = v[:, 0] * G
        e = epdf32.astype(T)
        if T is F64:
            bp = np.where(np.abs(bp) > FLT_MAX, np.inf, bp)
        raw = e * e + bp * bp
        if T is F64:
            raw = np.where(raw > FLT_MAX, np.inf, raw)
        den = np.maximum(raw, mis_eps) if mis_eps > 0 else raw
        w = np.where((e > 0) & ~np.isinf(bp), e * e / den, T(0))
        w = np.where(np.isinf(e) | (bp == 0), T(1), w)
        ew = G / np.maximum(e, pdf_eps)
        s = visible.astype(T)
        coef = v[:, 1:] * (s * ew)[:, None] * w[:, None]
        mag = np.abs(v[:, 1:] * (s * ew)[:, None]).max(-1)
    br = {"emit_pdf < pdf_eps": (np.ones(len(e), bool), e < pdf_eps)}
    if g_eps > float(RAY_EPS) ** 2:                                 # (d >= RayEpsilon: the other variant's clamp is out of a ray's reach, see UNOBSERVABLE)
        br["d2 < g_eps"] = (hit, np.asarray(d2) < g_eps)
    if mis_eps > 0:
        br["mis den < mis_eps"] = (visible & (bp != 0), raw < mis_eps)
    return coef, br, mag


def finish_formula(sc, a, rough_next, trace_rough, g_eps, T=F64, use_slf=True, area=None):
    """utils/path_tracing.py:394-404 / :476-486 with eval_emitter (model/emitter.py:180-221) -> coef2, const2 (N, 3), e2, valid_next, branch masks, undecided mask.
    a: pos, pos_next, nrm_next, wi, tri_next, pdf, weight; rough_next None = the caller's promise that every roughness exceeds trace_roughness.
    area: None = the float32 table and a float32 quotient; a float64 table = emit_pdf and the cache index as a float64 run of the reference forms them."""
    em, tri = sc["em"], a["tri_next"]
    n = len(tri)
    vis = tri != -1
    ts = np.where(vis, tri, 0)
    is_area = vis & sc["is_emitter"][ts]
    ordv = np.where(is_area, sc["ord_of"][ts], -1)
    if area is None:
        e32 = np.where(is_area, em["emitter_pdf"] / np.maximum(em["area"][np.maximum(ordv, 0)], F32(1e-12)), F32(0)).astype(F32)     # (one float32 quotient: exact to restate)
    else:
        e32 = np.where(is_area, (1.0 / em["K"]) / np.maximum(area[np.maximum(ordv, 0)], 1e-12), 0.0)
    surf = ~is_area & vis
    valid = surf.copy()
    diffuse = surf & (np.ones(n, bool) if rough_next is None else rough_next > (F32(trace_rough) if area is None else float(trace_rough)))
    slf = np.zeros((n, 3), F32)
    undecided = np.zeros(n, bool)
    positive, empty = np.zeros(n, bool), np.zeros(n, bool)
    looked = diffuse & use_slf
    if looked.any():
        j, rgb = slf_lookup(sc["slf"], a["pos_next"][looked], F32 if area is None else F64)
        slf[looked] = rgb
        s32 = (rgb[:, 0] + rgb[:, 1]) + rgb[:, 2]
        s64 = rgb.astype(F64).sum(-1)
        positive[looked] = s32 > 0
        empty[looked] = j < 0
        undecided[looked] = (s32 > 0) != (s64 > 0)
    valid = valid & ~positive
    with np.errstate(all="ignore"):
        x, pn, nn, wi = (a[k].astype(T) for k in ("pos", "pos_next", "nrm_next", "wi"))
        dl = x - pn
        d2 = (dl[:, 0] * dl[:, 0] + dl[:, 1] * dl[:, 1]) + dl[:, 2] * dl[:, 2]
        G = np.abs(R._dot(-nn, wi)) / np.maximum(d2, T(g_eps))
        G = np.where(valid, G, T(1))
        bp = a["pdf"].astype(T) * G
        e = e32.astype(T)
        b2 = bp * bp
        if T is F64:
            bp = np.where(np.abs(bp) > FLT_MAX, np.inf, bp)
            b2 = np.where(b2 > FLT_MAX, np.inf, b2)
        w = np.where((bp > 0) & ~np.isinf(e), b2 / (e * e + b2), T(0))
        w = np.where(np.isinf(bp) | (e == 0), T(1), w)
        wt = a["weight"].astype(T)
        coef2 = wt * w[:, None]
        const2 = wt * slf.astype(T) * w[:, None]
    br = {"hit": (np.ones(n, bool), vis), "hit is an emitter": (vis, is_area), "roughness_next > trace_roughness": (surf, diffuse),
          "cache voxel is empty": (looked, empty),
          "cache sum > 0": (looked, positive), "brdf_pdf > 0 on an emitter": (is_area, bp > 0), "brdf_pdf.isinf() on an emitter": (is_area, np.isinf(bp))}
    return coef2, const2, ordv.astype(np.int32), valid, br, undecided


def apply_formula(tb, nan_to_zero, drop):
    """utils/path_tracing.py:459-461, :469, :484-486 -> L, throughput (float64 values of the float32 operation sequence), tolerance of L"""
    g = lambda k: None if drop == k else tb[k].astype(F64 if tb[k].dtype == F32 else tb[k].dtype)
    L, rows, thr, e, cst, weight = tb["L"].astype(F64), g("rows"), g("throughput"), g("e"), g("cst"), g("weight")
    rad, coef = tb["radiance"].astype(F64), tb["coef"].astype(F64)
    n = len(coef)
    with np.errstate(all="ignore"):
        v = np.zeros((n, 3)) if cst is None else cst.copy()
        mag = np.abs(v)
        if e is not None:
            m = e >= 0
            cr = coef[m] * rad[e[m]]
            v[m] = v[m] + cr
            mag[m] = mag[m] + np.abs(cr)
        if thr is not None:
            v = thr * v
            mag = np.abs(thr) * mag
        if nan_to_zero:
            v = np.where(np.isnan(v), 0.0, v)
        idx = np.arange(n) if rows is None else rows
        tol = np.full_like(L, FLOOR)                              # (a row that no path touches must keep its bits)
        tol[idx] = 3 * U * np.where(np.isfinite(mag), mag, 0.0) + U * (np.abs(L[idx]) + np.where(np.isfinite(v), np.abs(v), 0.0)) + FLOOR
        L[idx] = L[idx] + v
        t_out = None if thr is None else (thr * weight if weight is not None else thr)
    return L, t_out, tol


# ============================================================================================================ the exact visibility hit
def exact_visibility(sc, o32, d32, C):
    """the exact closest crossing of every ray (t >= 0, barycentrics >= 0) over all triangles, and the two geometric reasons for which a row is undecided"""
    g = sc["geom"]
    n, T = len(o32), len(g.faces)
    t, b, _ = H.exact_hits(sc["verts"], sc["faces"], o32, d32, g)
    o64, d64 = o32.astype(F64), d32.astype(F64)
    Rr = np.abs(g.Pabs[None, :, :, :] - o64[:, None, None, :]).max((2, 3))
    ar = np.arange(n)
    with np.errstate(all="ignore"):
        h = np.abs(d64 @ g.N.T) / g.L[None, :]
        ub, ut = U * Rr / h, U * Rr * g.L[None, :] / h
        bmin = b.min(0)
        ex = (bmin >= 0) & (t >= 0) & np.isfinite(t)
        te = np.where(ex, t, np.inf)
        k = te.argmin(1)
        hit = ex[ar, k]
        tk = te[ar, k]
        utk = np.where(hit, ut[ar, k], 0.0)
        reach = t <= tk[:, None] + C["t"] * (ut + utk[:, None])
        near_b = (np.abs(bmin) <= C["b"] * ub) & (t >= -C["t"] * ut)
        near_0 = (np.abs(t) <= C["t"] * ut) & (bmin >= -C["b"] * ub)
        edge = ((near_b | near_0) & reach).any(1)
        other = ex & (np.arange(T)[None, :] != k[:, None])
        second = hit & (other & (t - tk[:, None] <= C["t"] * (ut + utk[:, None]))).any(1)
    k = np.where(hit, k, -1)
    bk = b[:, ar, np.maximum(k, 0)]
    return {"k": k, "hit": hit, "bary": bk, "edge": edge, "second": second & ~edge}


def nee_reference(sc, rows, variant, wi32, epdf32, etri):
    """float64 coef1 with its base tolerance (C = 1), e1, the branch masks and the undecided rows by reason, given the code under test's sample_emitter outputs"""
    C = H.measured()[0]
    g, em = sc["geom"], sc["em"]
    x32 = rows["pos"]
    n = len(x32)
    wi32 = np.ascontiguousarray(wi32, F32).reshape(n, 3)
    epdf32, etri = np.asarray(epdf32, F32).reshape(n), np.asarray(etri, np.int64).reshape(n)
    o32 = x32 + RAY_EPS * wi32                                      # float32: one product, one sum per component
    vz = exact_visibility(sc, o32, wi32, C)
    k, hit = vz["k"], vz["hit"]
    kk = np.maximum(k, 0)
    ep = (vz["bary"].T[:, :, None] * g.Pabs[kk]).sum(1)
    dl = np.where(hit[:, None], ep - x32.astype(F64), 1.0)
    d2 = (dl * dl).sum(-1)
    with np.errstate(all="ignore"):
        Nh = g.N[kk] / g.Nlen[kk][:, None]
        cosv = np.where(hit, np.abs(R._dot(wi32.astype(F64), Nh)), 1.0)
        un = H.units(g, o32, wi32, kk)
        up, unn = np.where(hit, C["p"] * un["p"], 0.0), np.where(hit, C["n"] * un["n"], 0.0)
    up, unn = np.where(np.isfinite(up), up, np.inf), np.where(np.isfinite(unn), unn, np.inf)
    dd2 = np.where(hit, 2 * np.abs(dl).sum(-1) * up + 3 * up * up + 4 * U * d2, 0.0)
    dcos = np.where(hit, np.sqrt(3.0) * unn + 4 * U, 0.0)
    visible = ~hit | (etri == k)
    c = R.cosines(wi32, rows["wo"], rows["nrm"])
    fn = lambda c_, dden=0.0, d2_=d2, cos_=cosv: nee_formula(c_, dden, d2_, cos_, hit, visible, epdf32, rows, variant)[0]
    f, br, mag = nee_formula(c, 0.0, d2, cosv, hit, visible, epdf32, rows, variant)
    with np.errstate(all="ignore"):
        tol = C_ROUND_NEE * U * np.abs(f) + FLOOR
        dev = lambda a, b_: np.maximum(np.abs(a - f), np.abs(b_ - f))
        for i in range(4):
            e = np.zeros(4)
            e[i] = R.DELTA
            tol = tol + dev(fn(c + e), fn(c - e))
        tol = tol + dev(fn(c, 4 * U), fn(c, -4 * U))
        tol = tol + dev(fn(c, d2_=d2 + dd2), fn(c, d2_=np.maximum(d2 - dd2, 0.0)))
        tol = tol + dev(fn(c, cos_=np.minimum(cosv + dcos, 1.0)), fn(c, cos_=np.maximum(cosv - dcos, 0.0)))
        pole = R.ggx_den(c, rows["rough"]) - (2 * np.maximum(c[:, 3], 0) * R.DELTA + 4 * U) <= 0
    tol = np.where(np.isfinite(tol) & ~pole[:, None], tol, np.inf)
    cdf = em["cdf"]
    v = np.maximum(rows["s1"], F32(1e-12))
    near_cdf = (np.abs(v[:, None].astype(F64) - cdf[None, :].astype(F64)) <= np.spacing(cdf)[None, :]).any(1)
    und = {"edge": vz["edge"], "second": vz["second"] & ~vz["edge"], "cdf": near_cdf & ~vz["edge"] & ~vz["second"], "threshold": np.zeros(n, bool)}
    e1 = np.where(hit & sc["is_emitter"][kk], sc["ord_of"][kk], -1).astype(np.int32)
    br = dict(br)
    br["visibility ray hits"] = (np.ones(n, bool), hit)
    br["hit is the sampled triangle"] = (hit, etri == k)
    br["another triangle hit is an emitter"] = (hit & (etri != k), e1 >= 0)
    return {"f": f, "tol": tol, "e1": e1, "branches": br, "undecided": und, "mag": mag, "pole": pole}


def undecided_any(und):
    out = None
    for v in und.values():
        out = v.copy() if out is None else out | v
    return out


def count_branches(branches, decided):
    return {name: (int((dom & decided & side).sum()), int((dom & decided & ~side).sum())) for name, (dom, side) in branches.items()}


def add_counts(total, part):
    for k, (a, b) in part.items():
        t = total.get(k, (0, 0))
        total[k] = (t[0] + a, t[1] + b)
    return total


def ratio(got, f, tol):
    """worst |err| / tol over the finite-tolerance elements; the rows where `got` is not finite are returned separately"""
    got = np.asarray(got, F64).reshape(f.shape)
    with np.errstate(all="ignore"):
        ok = np.isfinite(tol) & np.isfinite(got) & np.isfinite(f)
        r = np.where(ok, np.abs(got - f) / tol, 0.0)
    return r, ~np.isfinite(got)


def same_class(got, f):
    """non-finite values agree in kind: nan with nan, +-inf with the same inf (a float64 value above FLT_MAX counts as inf)"""
    got = np.asarray(got, F64).reshape(f.shape)
    with np.errstate(all="ignore"):
        f = np.where(np.abs(f) > FLT_MAX, np.sign(f) * np.inf, f)
    nf = ~np.isfinite(got) | ~np.isfinite(f)
    return ~nf | (np.isnan(got) & np.isnan(f)) | (got == f)


# ============================================================================================================ the float32 run, the oracle
def accumulate_np(radiance, e0, path_of, e1, coef1, e2, coef2, const2, B, spp):
    """L[b] = (sum over s = 0, 1, ... in that order of term(b, s)) * (1.0f / spp), float32, one rounding per operation (include/iris_hip.h):
    term = radiance[e0] (or 0); if the path continues: term += coef1 * radiance[e1]; t2 = const2 (+= coef2 * radiance[e2]); term += t2"""
    acc = np.zeros((B, 3), F32)
    for s in range(spp):
        i = np.arange(B) * spp + s
        l = np.where((e0[i] >= 0)[:, None], radiance[np.maximum(e0[i], 0)], F32(0)).astype(F32)
        j = path_of[i]
        act = j >= 0
        jj = np.maximum(j, 0)
        m1 = act & (e1[jj] >= 0)
        l = np.where(m1[:, None], l + coef1[jj] * radiance[np.maximum(e1[jj], 0)], l)
        t2 = const2[jj]
        m2 = e2[jj] >= 0
        t2 = np.where(m2[:, None], t2 + coef2[jj] * radiance[np.maximum(e2[jj], 0)], t2)
        l = np.where(act[:, None], l + t2, l)
        acc = acc + l
    return acc * (F32(1.0) / F32(spp))


def accumulate_bwd_np(gL, e0, path_of, e1, coef1, e2, coef2, B, spp, n_rad, T=F64, per_pixel=None):
    """d radiance[e] += gL[b] * (1 / spp) * coefficient over every path; per_pixel: paths per pixel (n_calls * spp for the training step) -> (grad, addends per row)"""
    pp = spp if per_pixel is None else per_pixel
    g = np.zeros((n_rad, 3), T)
    cnt = np.zeros(n_rad, np.int64)
    gp = np.repeat(np.asarray(gL, T) * (T(1) / T(spp)), pp, 0)
    m = e0 >= 0
    np.add.at(g, e0[m], gp[m]); np.add.at(cnt, e0[m], 1)
    act = path_of >= 0
    j = path_of[act]
    for e, c in ((e1, coef1), (e2, coef2)):
        mm = e[j] >= 0
        np.add.at(g, e[j][mm], gp[act][mm] * c[j][mm].astype(T)); np.add.at(cnt, e[j][mm], 1)
    return g, cnt


def accumulate_case(B, spp, n_rad, spread, seed=0, per_pixel=None):
    """paths of B pixels: a third end at the primary hit (path_of = -1), e0 / e1 / e2 = -1 on a part of the rows; spread: the emitter rows the paths land on"""
    rng = np.random.default_rng([seed, B, spp, spread])
    n = B * (spp if per_pixel is None else per_pixel)
    act = rng.random(n) > 0.33
    N = int(act.sum())
    path_of = np.full(n, -1, np.int32)
    path_of[act] = rng.permutation(N).astype(np.int32)
    pick = lambda m, p: np.where(rng.random(m) < p, rng.integers(0, spread, m), -1).astype(np.int32)
    e0 = np.where(act, -1, pick(n, 0.5)).astype(np.int32)
    return {"radiance": rng.uniform(0, 40, (n_rad, 3)).astype(F32), "e0": e0, "path_of": path_of, "e1": pick(N, 0.7), "coef1": rng.uniform(0, 3, (N, 3)).astype(F32),
            "e2": pick(N, 0.4), "coef2": rng.uniform(0, 2, (N, 3)).astype(F32), "const2": (rng.uniform(0, 1, (N, 3)) * (rng.random((N, 1)) > 0.5)).astype(F32),
            "gL": rng.normal(size=(B, 3)).astype(F32), "B": B, "spp": spp, "n_rad": n_rad}


class Numpy32:
    """The restatement in float32 behind the call surface of the oracle and the HIP backends: brdf_ref64's float32 samplers, hit_ref64's float32 closest hit."""
    name = "numpy-f32"

    def __init__(self):
        self.b = R.Numpy32()

    def sample_emitter(self, sc, s1, s2, pos):
        return self.b.sample_emitter(sc["em"], s1, s2, pos)

    def nee(self, sc, rows, variant):
        wi, epdf, etri = self.sample_emitter(sc, rows["s1"], rows["s2"], rows["pos"])
        epdf = epdf.reshape(-1)
        o = rows["pos"] + RAY_EPS * wi
        h = H.restated_hit(sc["verts"], sc["faces"], o, wi, F32)
        hit = h["idx"] >= 0
        with np.errstate(all="ignore"):
            dl = h["p"] - rows["pos"]
            d2 = (dl[:, 0] * dl[:, 0] + dl[:, 1] * dl[:, 1]) + dl[:, 2] * dl[:, 2]
            cosv = np.abs(R._dot(-wi, h["n"]))
        coef = nee_formula(R.cosines(wi, rows["wo"], rows["nrm"], F32), 0.0, d2, cosv, hit, ~hit | (etri == h["idx"]), epdf, rows, variant, F32)[0]
        k = np.maximum(h["idx"], 0)
        return coef, np.where(hit & sc["is_emitter"][k], sc["ord_of"][k], -1).astype(np.int32)

    def brdf_trace(self, sc, rows):
        with np.errstate(all="ignore"):
            wi, pdf, w = self.b.sample_brdf(rows["s1b"], rows["s2b"], rows["wo"], rows["nrm"], rows["albedo"], rows["rough"], rows["metal"])
        h = H.restated_hit(sc["verts"], sc["faces"], rows["pos"] + RAY_EPS * wi, wi, F32)
        return wi, pdf.reshape(-1), w, h["p"], h["n"], h["idx"]

    def finish(self, sc, a, rough_next, trace_rough, g_eps, use_slf=True):
        return finish_formula(sc, a, rough_next, trace_rough, g_eps, F32, use_slf)[:4]

    def apply(self, tb, nan_to_zero, drop):
        g = lambda k: None if drop == k else tb[k]
        L, thr = tb["L"].copy(), (None if drop == "throughput" else tb["throughput"].copy())
        n = len(tb["coef"])
        with np.errstate(all="ignore"):
            v = np.zeros((n, 3), F32) if g("cst") is None else tb["cst"].copy()
            if g("e") is not None:
                m = tb["e"] >= 0
                v[m] = v[m] + tb["coef"][m] * tb["radiance"][tb["e"][m]]
            if thr is not None:
                v = thr * v
            if nan_to_zero:
                v[np.isnan(v)] = 0
            idx = np.arange(n) if g("rows") is None else tb["rows"]
            L[idx] = L[idx] + v
            if thr is not None and g("weight") is not None:
                thr = thr * tb["weight"]
        return L, thr

    def accumulate(self, c):
        return accumulate_np(c["radiance"], c["e0"], c["path_of"], c["e1"], c["coef1"], c["e2"], c["coef2"], c["const2"], c["B"], c["spp"])


class Oracle:
    """oracle/ in one of its two modes (0: libm, 1: the kernels' arithmetic): orc_pt_nee, orc_pt_brdf_trace, orc_pt_brdf_finish, _apply, orc_pt_accumulate"""

    def __init__(self, oracle_mod, mode):
        import oracle.oracle as OO
        self.o, self.OO, self.mode, self.name = oracle_mod, OO, int(mode), ("libm", "device-arithmetic")[int(mode)]
        self._sc = {}

    def _in_mode(self, fn, *a):
        prev = self.o.get_mode()
        self.o.set_mode(self.mode)
        try:
            return fn(*a)
        finally:
            self.o.set_mode(prev)

    def objects(self, sc):
        key = sc["em"]["key"]
        if key not in self._sc:
            s, em = sc["slf"], sc["em"]
            slf = self.o.VoxelSLF(s["inds"], s["radiance"], s["vmin"], s["vmax"])
            e = self.o.SLFEmitter(sc["is_emitter"], np.zeros((em["K"], 3), F32), em["area"], slf, em["verts"], em["cdf"])
            self._sc[key] = (self.o.Scene(sc["verts"], sc["faces"]), e, slf)
        return self._sc[key]

    def sample_emitter(self, sc, s1, s2, pos):
        return self._in_mode(self.objects(sc)[1].sample_emitter, s1, s2, pos)

    def nee(self, sc, rows, variant):
        import ctypes as C
        scn, e, _ = self.objects(sc)
        p, f = self.OO._p, self.OO._f32
        n = len(rows["pos"])
        coef1, e1 = np.empty((n, 3), F32), np.empty(n, np.int32)
        a = [f(rows[k]) for k in ("pos", "nrm", "wo", "albedo", "rough", "metal", "s1", "s2")]
        self._in_mode(lambda: self.o.lib().orc_pt_nee(scn.h, e.h, *[p(x) for x in a], C.c_int64(n), p(coef1), p(e1), *[C.c_float(float(v)) for v in variant]))
        return coef1, e1

    def brdf_trace(self, sc, rows):
        scn = self.objects(sc)[0]
        f = self.OO._f32
        mat = (f(rows["albedo"]), f(rows["rough"]), f(rows["metal"]))
        return self._in_mode(self.OO._lobe_trace, scn, f(rows["pos"]), f(rows["nrm"]), f(rows["wo"]), mat, f(rows["s1b"]), f(rows["s2b"]), 0)

    def finish(self, sc, a, rough_next, trace_rough, g_eps, use_slf=True):
        import ctypes as C
        _, e, slf = self.objects(sc)
        p, f = self.OO._p, self.OO._f32
        n = len(a["pos"])
        rn = f(np.full(n, 0.9, F32) if rough_next is None else rough_next)       # (the oracle has no NULL roughness: the promise, spelled out)
        coef2, const2, e2, vn = np.empty((n, 3), F32), np.empty((n, 3), F32), np.empty(n, np.int32), np.empty(n, np.uint8)
        args = [f(a[k]) for k in ("pos", "pos_next", "nrm_next", "wi")] + [np.ascontiguousarray(a["tri_next"], np.int64), rn, f(a["pdf"]), f(a["weight"])]
        self._in_mode(lambda: self.o.lib().orc_pt_brdf_finish(e.h, slf.h if use_slf else None, *[p(x) for x in args], C.c_int64(n), p(coef2), p(const2), p(e2), p(vn),
                                                               C.c_float(float(trace_rough)), C.c_float(float(g_eps))))
        return coef2, const2, e2, vn.astype(bool)

    def apply(self, tb, nan_to_zero, drop):
        """(the oracle's _apply has the trace_indirect form only: NaN -> 0, throughput, rows and e / coef present)"""
        if not nan_to_zero or drop in ("rows", "throughput", "e"):
            return None
        L, thr = tb["L"].copy(), tb["throughput"].copy()
        with np.errstate(all="ignore"):
            self.OO._apply(L, tb["rows"], thr, tb["radiance"], tb["e"], tb["coef"], None if drop == "cst" else tb["cst"].copy(), None if drop == "weight" else tb["weight"])
        return L, thr

    def accumulate(self, c):
        import ctypes as C
        p = self.OO._p
        L = np.empty((c["B"], 3), F32)
        self.o.lib().orc_pt_accumulate(*[p(np.ascontiguousarray(c[k])) for k in ("radiance", "e0", "path_of", "e1", "coef1", "e2", "coef2", "const2")],
                                       C.c_int64(c["B"]), C.c_int(c["spp"]), p(L))
        return L


# ============================================================================================================ the checks
class Yardstick:
    """E per stage: the worst |err| / tol of the float32 restatement and of the libm oracle (not of the code under test), cached per key.  C = 4 E."""
    E_MAX = 1.0        # the envelope is derived to hold float32's own error: an E above 1 means the derivation, not the code, is off

    def __init__(self, oracle_mod):
        self.backs = (Numpy32(), Oracle(oracle_mod, 0))
        self.E = {}

    def C(self, key, measure):
        if key not in self.E:
            e = max(measure(b) for b in self.backs)
            assert 0 < e <= self.E_MAX, f"E[{key}] = {e:.3g}: the yardstick itself is off"
            self.E[key] = e
        return 4.0 * self.E[key]

    def stage_E(self, stage):
        v = [e for k, e in self.E.items() if k[0] == stage]
        return max(v) if v else None


def _nee_run(back, sc, rows, variant):
    wi, epdf, etri = back.sample_emitter(sc, rows["s1"], rows["s2"], rows["pos"])
    ref = nee_reference(sc, rows, variant, wi, epdf, etri)
    coef1, e1 = back.nee(sc, rows, variant)
    return ref, np.asarray(coef1, F32), np.asarray(e1, np.int32).reshape(-1)


def _nee_ratio(back, sc, rows, variant):
    ref, coef1, _ = _nee_run(back, sc, rows, variant)
    r, _ = ratio(coef1, ref["f"], ref["tol"])
    return float(r[~undecided_any(ref["undecided"])].max(initial=0.0))


def check_nee(back, yard, scene_name, variant, n_rows=None, log=print):
    """the emitter-sampling stage (iris_pt_nee / orc_pt_nee) on the first n_rows rows of a scene's table"""
    sc = scene(scene_name)
    rows = head(sc["rows"], n_rows)
    var = VARIANTS[variant]
    Cc = yard.C(("nee", scene_name, variant), lambda b: _nee_ratio(b, sc, sc["rows"], var))
    ref, coef1, e1 = _nee_run(back, sc, rows, var)
    n = len(e1)
    und = undecided_any(ref["undecided"])
    dec = ~und
    name = f"nee[{back.name}, {scene_name}, {variant}, {n} rows]"
    bad = np.nonzero(dec & (e1 != ref["e1"]))[0]
    assert bad.size == 0, f"{name}: e1 differs on {bad.size} decided rows, first {bad[:5].tolist()}: got {e1[bad[:5]].tolist()} want {ref['e1'][bad[:5]].tolist()}"
    r, nonfinite = ratio(coef1, ref["f"], ref["tol"])
    allowed = ~np.isfinite(ref["tol"]) | (ref["mag"] >= 1e37)[:, None] | ~np.isfinite(ref["f"])
    nf_bad = np.nonzero((dec[:, None] & nonfinite & ~allowed).any(-1))[0]
    assert nf_bad.size == 0, f"{name}: non-finite coef1 on rows {nf_bad[:5].tolist()} where the float64 value is {ref['f'][nf_bad[:5]].tolist()}"
    worst = float((r[dec] / Cc).max(initial=0.0))
    counts = {k: int(v.sum()) for k, v in ref["undecided"].items()}
    log(f"{name}: worst |err| / (C tol) {worst:.3f} (C = {Cc:.2f}), excluded {counts}, pole rows {int((ref['pole'] & dec).sum())}, "
        f"vacuous {100.0 * (~np.isfinite(ref['tol']).all(-1) & dec).mean():.2f} %")
    out = np.nonzero(dec & (r > Cc).any(-1))[0]
    assert out.size == 0, (f"{name}: {out.size} rows outside the envelope, first {out[:5].tolist()}: got {coef1[out[:5]].tolist()} f64 {ref['f'][out[:5]].tolist()} "
                           f"C tol {(Cc * ref['tol'][out[:5]]).tolist()}")
    return {"undecided": counts, "n": n, "branches": count_branches(ref["branches"], dec), "worst": worst}


def _finish_args(back, sc, rows):
    wi, pdf, w, pn, nn, tri = back.brdf_trace(sc, rows)
    return {"pos": rows["pos"], "pos_next": np.asarray(pn, F32), "nrm_next": np.asarray(nn, F32), "wi": np.asarray(wi, F32), "tri_next": np.asarray(tri, np.int64).reshape(-1),
            "pdf": np.asarray(pdf, F32).reshape(-1), "weight": np.asarray(w, F32)}


def _finish_compare(name, got, ref, Cc):
    coef2, const2, e2, vn = (np.asarray(x) for x in got)
    f2, fc, re2, rvn, br, und = ref
    dec = ~und
    assert np.array_equal(e2.reshape(-1)[dec], re2[dec]), f"{name}: e2 differs on rows {np.nonzero(dec & (e2.reshape(-1) != re2))[0][:5].tolist()}"
    assert np.array_equal(vn.reshape(-1).astype(bool)[dec], rvn[dec]), f"{name}: valid_next differs on rows {np.nonzero(dec & (vn.reshape(-1).astype(bool) != rvn))[0][:5].tolist()}"
    worst = 0.0
    for what, g_, f_ in (("coef2", coef2, f2), ("const2", const2, fc)):
        ok = same_class(g_, f_)
        assert ok[dec].all(), f"{name}: {what} non-finite values differ in kind on rows {np.nonzero(dec & ~ok.all(-1))[0][:5].tolist()}"
        with np.errstate(all="ignore"):
            tol = C_ROUND_FINISH * U * np.abs(f_) + FLOOR
        r, _ = ratio(g_, f_, np.where(np.isfinite(tol), tol, np.inf))
        out = np.nonzero(dec & (r > Cc).any(-1))[0]
        assert out.size == 0, f"{name}: {what} outside the envelope on {out.size} rows, first {out[:5].tolist()}: got {g_[out[:5]].tolist()} f64 {f_[out[:5]].tolist()}"
        worst = max(worst, float((r[dec] / Cc).max(initial=0.0)))
    return worst


def _finish_ratio(back, sc, a, rough_next, trace_rough, g_eps, use_slf):
    got = back.finish(sc, a, rough_next, trace_rough, g_eps, use_slf)
    f2, fc, _, _, _, und = finish_formula(sc, a, rough_next, trace_rough, g_eps, F64, use_slf)
    worst = 0.0
    for g_, f_ in ((got[0], f2), (got[1], fc)):
        with np.errstate(all="ignore"):
            tol = C_ROUND_FINISH * U * np.abs(f_) + FLOOR
        worst = max(worst, float(ratio(g_, f_, np.where(np.isfinite(tol), tol, np.inf))[0][~und].max(initial=0.0)))
    return worst


FINISH_OF = {"single": (0.0, F32(1e-6)), "indirect": (0.6, F32(1e-12))}      # (trace_roughness, g_eps) of path_tracing_single (:335, :397) and trace_indirect (:180, :478)


def check_brdf_stage(back, yard, scene_name, variant, n_rows=None, log=print):
    """the BRDF-sampling stage's outputs (taken as they are) through the finish stage"""
    sc = scene(scene_name)
    rows = head(sc["rows"], n_rows)
    tr, g_eps = FINISH_OF[variant]
    Cc = yard.C(("finish", scene_name, variant), lambda b: _finish_ratio(b, sc, _finish_args(b, sc, sc["rows"]), sc["rows"]["rough_next"], tr, g_eps, True))
    a = _finish_args(back, sc, rows)
    ref = finish_formula(sc, a, rows["rough_next"], tr, g_eps)
    name = f"brdf stage + finish[{back.name}, {scene_name}, {variant}, {len(a['pdf'])} rows]"
    worst = _finish_compare(name, back.finish(sc, a, rows["rough_next"], tr, g_eps), ref, Cc)
    log(f"{name}: worst |err| / (C tol) {worst:.3f} (C = {Cc:.2f}), excluded {{'threshold': {int(ref[5].sum())}}}")
    return {"undecided": {"threshold": int(ref[5].sum())}, "n": len(a["pdf"]), "branches": count_branches(ref[4], ~ref[5]), "worst": worst}


FINISH_TABLE_CASES = (("single", 0.0, "rough"), ("indirect", 0.6, "rough"), ("single", 0.0, "null"), ("indirect", 0.6, "null"), ("indirect", np.inf, "no-slf"))


def check_finish_table(back, yard, variant, trace_rough, mode, n_rows=None, log=print):
    """the finish stage on the synthetic table.  mode 'rough': roughness_next given; 'null': NULL, on a table whose every roughness exceeds trace_roughness (the
    kernel's documented precondition; the reference gets that roughness); 'no-slf': trace_roughness = +inf with a NULL cache"""
    sc = scene("open")
    a = head(finish_table(), n_rows)
    g_eps = FINISH_OF[variant][1]
    use_slf = mode != "no-slf"
    rn = a["rough_next"] if mode != "null" else None
    rn_ref = rn if rn is not None else np.full(len(a["pdf"]), 0.9, F32)
    full = finish_table()
    Cc = yard.C(("finish", "table", variant, float(trace_rough), mode),
                lambda b: _finish_ratio(b, sc, full, full["rough_next"] if mode != "null" else None, trace_rough, g_eps, use_slf))
    ref = finish_formula(sc, a, rn_ref, trace_rough, g_eps, F64, use_slf)
    name = f"finish table[{back.name}, {variant}, trace_roughness {trace_rough}, {mode}, {len(a['pdf'])} rows]"
    worst = _finish_compare(name, back.finish(sc, a, rn, trace_rough, g_eps, use_slf), ref, Cc)
    log(f"{name}: worst |err| / (C tol) {worst:.3f} (C = {Cc:.2f}), excluded {{'threshold': {int(ref[5].sum())}}}")
    return {"undecided": {"threshold": int(ref[5].sum())}, "n": len(a["pdf"]), "branches": count_branches(ref[4], ~ref[5]), "worst": worst}


def check_apply(back, nan_to_zero, drop, log=print):
    tb = apply_table()
    got = back.apply(tb, nan_to_zero, drop)
    if got is None:
        return None
    L, thr, tol = apply_formula(tb, nan_to_zero, drop)
    name = f"apply[{back.name}, nan_to_zero {nan_to_zero}, without {drop}]"
    ok = same_class(got[0], L)
    assert ok.all(), f"{name}: non-finite values differ in kind on rows {np.nonzero(~ok.all(-1))[0][:5].tolist()}"
    r, _ = ratio(got[0], L, tol)
    log(f"{name}: worst |err| / tol {float(r.max()):.3f}")
    assert (r <= 1.0).all(), f"{name}: rows {np.nonzero((r > 1).any(-1))[0][:5].tolist()} outside the bound"
    if thr is not None:
        ok = same_class(got[1], thr)
        with np.errstate(all="ignore"):
            d = np.abs(np.asarray(got[1], F64) - thr)
            assert ok.all() and (~np.isfinite(thr) | (d <= U * np.abs(thr) + FLOOR)).all(), f"{name}: throughput"
    if nan_to_zero:
        touched = np.arange(len(tb["coef"])) if drop == "rows" else tb["rows"]
        assert not np.isnan(np.asarray(got[0])[touched][~np.isnan(tb["L"][touched])]).any(), f"{name}: a NaN reached L"
    return float(r.max())
