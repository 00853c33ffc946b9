"""Helper (not a test): the BRDF samplers and the GGX evaluation (model/brdf.py:20-210, model/emitter.py:224-255, utils/ops.py:12-118) restated from their
formulas in numpy, in a chosen dtype, with the case tables and the checks that tests/test_brdf_ref64_cpu.py (oracle, both modes, and the float32 run of
this restatement) and tests/test_brdf_ref64.py (the HIP kernels) share.  No torch, and nothing taken from oracle/iris_oracle.c.

Two ideas make the comparison elementwise and tight.

Stage-wise continuation (directions).  The samplers' prefix is IEEE-exact float32 arithmetic -- sqrt(u0); c2 = (1 - u0) / (u0 (alpha^2 - 1) + 1) and its
sqrt; phi = f32(2 pi) u1 -- so it is computed in float32 by everybody, the reference included, and everything after it (the polar angle, its sin / cos, the
normalisations, the frame, to_world, the reflection about the half vector) in `dtype`.  dtype = float64 is the reference; dtype = float32 is "the
restatement in float32", one of the two runs that measure E, the reference arithmetic's own error.  (A closed form in float64 from u0 would not do: at
u0 = 1 - 2^-24 the float32 sqrt alone moves cos(theta) by 1e-4 -- the formula's conditioning, not a kernel's error.)

Perturbation envelope (pdf, brdf, g0, g1, weight).  They are evaluated in float64 on the direction the code under test returned, taken as exact: the
four cosines c = (NoL, NoV, VoH, NoH), then f(c) with the relu and the max(., 1e-4f) clamps in it.  Per element
    tol = 16 u |f| + sum_i max(|f(c + d e_i) - f|, |f(c - d e_i) - f|) + max(|f(den + 4 u) - f|, |f(den - 4 u) - f|),     u = 2^-24, d = 8 u:
a float32 normalise costs <= 3.5 u per component and a three-term dot of unit vectors <= 3 u more (d); the roundings of den = NoH^2 (alpha^2 - 1) + 1
are <= 4 u absolute (alpha^2 itself is formed in float32 here, as the prefix is); 16 u covers the roundings of the products and quotients after it.
The envelope widens by itself where f is ill conditioned (clamps, grazing angles, the peak of the r = 0.02 lobe) and is a few ulps elsewhere.
These constants are derived; a row outside its envelope is a finding, not a reason to widen them.  One such finding is part of the check now: the ends
of the box do not bound D_GGX on the few rows whose box contains its pole (den <= 20 u, r = 0.02 only); see envelope().
"""
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24
DELTA = 8 * U
PI_F = F32(np.pi)
TWO_PI_F = F32(2 * np.pi)
PIO2_F = F32(np.pi / 2)
TOP = F32(1.0 - 2.0 ** -24)                       # the largest value torch.rand returns
CLAMP = F32(1e-4)
F0 = F32(0.04)
ALPHA_T = F32                                     # the dtype alpha^2 = r^4 is formed in (float32: what everybody forms it in)
ROUGH_LEVELS = tuple(F32(r) for r in (0.02, 0.03, 0.05, 0.1, 0.216, 0.412, 0.608, 0.804, 1.0))
B = 1 << 15
GRID = (0.0, 2.0 ** -40, 2.0 ** -24, 0.125, float(np.nextafter(F32(0.25), F32(0))), 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, float(TOP))


# ============================================================================================================ the operations, in `dtype`
def _dot(a, b):
    return (a * b).sum(-1)


def _normalize(v, T):
    """NF.normalize(v, dim=-1) = v / max(|v|, 1e-12)"""
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    return v / np.maximum(n, T(1e-12))


def normal_space(n32, T):
    """utils/ops.py:12-30: tangent = normalize(cross(e, n)), e = (1,0,0) where |n.x| <= 0.1 (compared in float32) else (0,1,0); bitangent = cross(n, tangent)"""
    n = n32.astype(T)
    mask = np.abs(n32[:, 0]) <= F32(0.1)
    z = np.zeros_like(n[:, 0])
    t = np.where(mask[:, None], np.stack([z, -n[:, 2], n[:, 1]], -1), np.stack([n[:, 2], z, -n[:, 0]], -1))
    t = _normalize(t, T)
    return t, np.cross(n, t)


def angle2xyz(theta, phi, T):
    """utils/ops.py:32-44, theta and phi given in float32"""
    theta, phi = theta.astype(T), phi.astype(T)
    st = np.sin(theta)
    return _normalize(np.stack([st * np.cos(phi), st * np.sin(phi), np.cos(theta)], -1), T)


def _to_world(l, t, b, n):
    return l[:, 0:1] * t + l[:, 1:2] * b + l[:, 2:3] * n


def alpha2(rough32):
    """alpha^2 = r^4 of D_GGX and of the sampler, in the float32 products everybody forms it with"""
    r = np.asarray(rough32, ALPHA_T)
    a = r * r
    return a * a


def prefix_diffuse(u2):
    """(sqrt(u0), phi) in float32: the IEEE-exact prefix of diffuse_sampler"""
    return np.sqrt(u2[:, 0]), TWO_PI_F * u2[:, 1]


def prefix_specular(u2, rough32):
    """(sqrt(c2), phi) in float32: the IEEE-exact prefix of specular_sampler"""
    u0 = u2[:, 0]
    c2 = (F32(1) - u0) / (u0 * (alpha2(rough32) - F32(1)) + F32(1))
    return np.sqrt(c2), TWO_PI_F * u2[:, 1]


def diffuse_dir(u2, n32, T=np.float64):
    """model/brdf.py:20-34"""
    s, phi = prefix_diffuse(u2)
    t, b = normal_space(n32, T)
    l = angle2xyz(np.arcsin(s.astype(T)), phi.astype(T), T)
    return _to_world(l, t, b, n32.astype(T))


def specular_dir(u2, wo32, n32, rough32, T=np.float64):
    """model/brdf.py:36-59: the GGX half vector, and wo reflected about it"""
    s, phi = prefix_specular(u2, rough32)
    t, b = normal_space(n32, T)
    l = angle2xyz(np.arccos(s.astype(T)), phi.astype(T), T)
    wh = _to_world(l, t, b, n32.astype(T))
    wo = wo32.astype(T)
    return _normalize(T(2) * _dot(wo, wh)[:, None] * wh - wo, T)


def cosines(wi32, wo32, n32, T=np.float64):
    """(B, 4): NoL, NoV, VoH, NoH before the relu, h = normalize(wi + wo)"""
    wi, wo, n = wi32.astype(T), wo32.astype(T), n32.astype(T)
    h = _normalize(wi + wo, T)
    return np.stack([_dot(wi, n), _dot(wo, n), _dot(wo, h), _dot(n, h)], -1)


def ggx_den(c, rough32, T=np.float64):
    return np.maximum(c[:, 3], T(0)) ** 2 * (alpha2(rough32).astype(T) - T(1)) + T(1)


def _lobe(c, rough32, T, dden):
    """utils/ops.py:46-82 on relu(c): D_GGX (its denominator shifted by dden), the GGX pdf, G_Smith, (1 - VoH)^5"""
    c = np.maximum(c, T(0))
    NoL, NoV, VoH, NoH = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    r, a2, pi = np.asarray(rough32, ALPHA_T).astype(T), alpha2(rough32).astype(T), T(PI_F)
    den = NoH * NoH * (a2 - T(1)) + T(1) + np.asarray(dden, T)
    with np.errstate(divide="ignore", invalid="ignore"):       # (a float32 den can round to 0 at r = 0.02: D = inf, as in the reference)
        D = a2 / (pi * den * den)
    pdf_spec = D / (T(4) * np.maximum(VoH, T(CLAMP))) * NoH
    k = r + T(1)
    k = k * k / T(8)
    G = (T(1) / (NoL * (T(1) - k) + k)) * (T(1) / (NoV * (T(1) - k) + k))
    x1 = T(1) - VoH
    x2 = x1 * x1
    return D, pdf_spec, G, x2 * x2 * x1, NoL, VoH, NoH


def f_cos_pdf(c, T=np.float64, dden=0.0):
    """model/brdf.py:78-88: relu(n.wi) / pi; c is (B, 1)"""
    return np.maximum(c, T(0)) / T(PI_F)


def f_spec(c, rough32, T=np.float64, dden=0.0):
    """model/brdf.py:112-136 after the direction: (B, 3) = pdf, g0, g1"""
    D, pdf, G, x5, NoL, VoH, NoH = _lobe(c, rough32, T, dden)
    fac = G * VoH * NoL / np.maximum(NoH, T(CLAMP))
    return np.stack([pdf, (T(1) - x5) * fac, x5 * fac], -1)


def f_brdf(c, rough32, albedo32, metal32, T=np.float64, dden=0.0):
    """model/brdf.py:138-175: (B, 4) = pdf, brdf rgb (already multiplied by NoL)"""
    D, pdf_spec, G, x5, NoL, VoH, NoH = _lobe(c, rough32, T, dden)
    pi = T(PI_F)
    albedo, metal = albedo32.astype(T), metal32.astype(T)[:, None]
    om = T(1) - metal
    kd = albedo * om
    ks = T(F0) * om + albedo * metal
    pdf = T(0.5) * pdf_spec + T(0.5) * (NoL / pi)
    F = ks + (T(1) - ks) * x5[:, None]
    brdf = kd / pi * NoL[:, None] + (D * G)[:, None] * F / T(4) * NoL[:, None]
    return np.concatenate([pdf[:, None], brdf], -1)


def f_weight(c, rough32, albedo32, metal32, T=np.float64, dden=0.0):
    """model/brdf.py:205-208: (B, 3) = brdf / pdf where pdf > 0, else 0, NaN -> 0"""
    v = f_brdf(c, rough32, albedo32, metal32, T, dden)
    pdf = v[:, 0:1]
    w = np.where(pdf > 0, v[:, 1:] / np.where(pdf > 0, pdf, T(1)), T(0))
    return np.where(np.isnan(w), T(0), w)


def emitter_ordinal(cdf32, s1):
    """model/emitter.py:238: searchsorted(cdf, clamp_min(s1, 1e-12)), kept inside the table"""
    v = np.maximum(s1, F32(1e-12))
    return np.minimum(np.searchsorted(cdf32, v, side="left"), len(cdf32) - 1)


def emitter_dir(verts32, ordinal, s2, pos32, T=np.float64):
    """model/emitter.py:240-250: uniform point on the triangle (xi1 = sqrt(u0) is the float32 prefix), direction towards it"""
    xi1 = np.sqrt(s2[:, 0]).astype(T)
    u = T(1) - xi1
    v = xi1 * s2[:, 1].astype(T)
    w = (T(1) - u) - v
    p = verts32.astype(T)[ordinal]
    p1 = p[:, 0] * u[:, None] + p[:, 1] * v[:, None] + p[:, 2] * w[:, None]
    return _normalize(p1 - pos32.astype(T), T)


def lerp_plan(rough32, R):
    """utils/ops.py:107-115 in float32 (every operation exact IEEE): the two levels and the weight.  Outside [0.02, 1] the reference's gather raises;
    the kernels keep both indices inside the table, so the result there is the end level."""
    r = (rough32 - F32(0.02)) / F32(1.0 - 0.02) * F32(R - 1)
    fl = np.floor(r)
    w = r - fl
    r0 = np.clip(fl, 0, R - 1).astype(np.int64)
    r1 = np.clip(np.ceil(r), 0, R - 1).astype(np.int64)
    return r0, r1, w


def lerp_specular(spec32, rough32, T=np.float64):
    """-> (blend (B, 3) in T, tolerance 3 u (|a| (1 - w) + |b| w))"""
    R = spec32.shape[1]
    r0, r1, w = lerp_plan(rough32, R)
    i = np.arange(spec32.shape[0])
    a, b, w = spec32[i, r0].astype(T), spec32[i, r1].astype(T), w.astype(T)[:, None]
    return a * (T(1) - w) + b * w, 3 * U * (np.abs(a).astype(np.float64) * (1 - w) + np.abs(b) * w)


class float64_constants:
    """with float64_constants(): the formulas above with pi, 0.04, the 1e-4 clamp and alpha^2 in double -- what the reference's own Python computes when it
    is run in float64 (tests/test_pt_stage_ref64_cpu.py holds the restatement to such a run); outside it they are the float32 constants of a float32 run"""

    def __enter__(self):
        global PI_F, CLAMP, F0, ALPHA_T
        self.prev = (PI_F, CLAMP, F0, ALPHA_T)
        PI_F, CLAMP, F0, ALPHA_T = np.pi, 1e-4, 0.04, np.float64

    def __exit__(self, *a):
        global PI_F, CLAMP, F0, ALPHA_T
        PI_F, CLAMP, F0, ALPHA_T = self.prev


# ============================================================================================================ the float32 run of the restatement
class Numpy32:
    """The restatement above in float32, behind the same call surface as the oracle and the HIP backends."""
    name = "numpy-f32"
    T = F32

    def sample_diffuse(self, u2, n):
        wi = diffuse_dir(u2, n, F32)
        return wi, f_cos_pdf(_dot(n, wi)[:, None], F32), np.ones_like(wi)

    def sample_specular(self, u2, wo, n, rough):
        wi = specular_dir(u2, wo, n, rough, F32)
        v = f_spec(cosines(wi, wo, n, F32), rough, F32)
        return wi, v[:, 0:1], v[:, 1:2], v[:, 2:3]

    sample_specular_v = sample_specular

    def eval_brdf(self, wi, wo, n, albedo, rough, metal):
        v = f_brdf(cosines(wi, wo, n, F32), rough, albedo, metal, F32)
        return v[:, 1:], v[:, 0:1]

    def sample_brdf(self, s1, u2, wo, n, albedo, rough, metal):
        wi = np.where((s1 > F32(0.5))[:, None], diffuse_dir(u2, n, F32), specular_dir(u2, wo, n, rough, F32))
        c = cosines(wi, wo, n, F32)
        with np.errstate(all="ignore"):
            return wi, f_brdf(c, rough, albedo, metal, F32)[:, 0:1], f_weight(c, rough, albedo, metal, F32)

    def sample_emitter(self, em, s1, s2, pos):
        o = emitter_ordinal(em["cdf"], s1)
        pdf = em["emitter_pdf"] / np.maximum(em["area"][o], F32(1e-12))
        return emitter_dir(em["verts"], o, s2, pos, F32), pdf[:, None], em["triangle_idx"][o]

    def angle2xyz(self, theta, phi):
        return angle2xyz(theta, phi, F32)

    def get_normal_space(self, n):
        t, b = normal_space(n, F32)
        return np.stack([t, b, n], -1)

    def lerp_specular(self, spec, rough):
        return lerp_specular(spec, rough, F32)[0]


class Oracle:
    """oracle/ in one of its two modes (0: libm, 1: the kernels' arithmetic), behind the same call surface."""

    def __init__(self, oracle_mod, mode):
        self.o, self.mode, self.name = oracle_mod, int(mode), ("libm", "device-arithmetic")[int(mode)]
        self._em = {}

    def _run(self, fn, *a):
        prev = self.o.get_mode()
        self.o.set_mode(self.mode)
        try:
            return fn(*a)
        finally:
            self.o.set_mode(prev)

    def sample_diffuse(self, u2, n):
        return self._run(self.o.sample_diffuse, u2, n)

    def sample_specular(self, u2, wo, n, rough):
        return self._run(self.o.sample_specular, u2, wo, n, rough)

    def sample_specular_v(self, u2, wo, n, rough):
        """(the oracle has the scalar form only: one call per roughness value)"""
        outs = [np.empty((len(u2), k), F32) for k in (3, 1, 1, 1)]
        for r in np.unique(rough):
            m = rough == r
            for dst, src in zip(outs, self._run(self.o.sample_specular, u2[m], wo[m], n[m], r)):
                dst[m] = src
        return tuple(outs)

    @staticmethod
    def _mat(albedo, rough, metal):
        return {"albedo": albedo, "roughness": rough, "metallic": metal}

    def eval_brdf(self, wi, wo, n, albedo, rough, metal):
        return self._run(self.o.eval_brdf, wi, wo, n, self._mat(albedo, rough, metal))

    def sample_brdf(self, s1, u2, wo, n, albedo, rough, metal):
        return self._run(self.o.sample_brdf, s1, u2, wo, n, self._mat(albedo, rough, metal))

    def sample_emitter(self, em, s1, s2, pos):
        e = self._em.get(em["key"])
        if e is None:
            e = self._em[em["key"]] = self.o.SLFEmitter(em["is_emitter"], np.zeros((len(em["area"]), 3), F32), em["area"], None, em["verts"], em["cdf"])
        return self._run(e.sample_emitter, s1, s2, pos)

    def angle2xyz(self, theta, phi):
        return self._run(self.o.angle2xyz, theta, phi)

    def get_normal_space(self, n):
        return self._run(self.o.get_normal_space, n)

    def lerp_specular(self, spec, rough):
        return self._run(self.o.lerp_specular, spec, rough)


# ============================================================================================================ case tables (seeded, built once, read-only)
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _near(x, k):
    """the 2k + 1 float32 values around x, ascending"""
    x = F32(x)
    lo, hi = [x], [x]
    for _ in range(k):
        lo.append(np.nextafter(lo[-1], F32(-np.inf)))
        hi.append(np.nextafter(hi[-1], F32(np.inf)))
    return np.array(lo[:0:-1] + hi, F32)


def _hitting(fn, guess, targets, span, lo=0.0, hi=float(TOP)):
    """float32 arguments within `span` ulps of `guess` (and inside [lo, hi]) that fn maps onto one of `targets`, at most two per target"""
    x = _near(guess, span)
    x = x[(x >= F32(lo)) & (x <= F32(hi))]
    y = fn(x)
    out = []
    for t in targets:
        out += list(x[y == F32(t)][:2])
    return out


HALF3 = tuple(_near(0.5, 1))


def u0_for_sqrt_half():
    """u0 whose float32 sqrt is 0.5 or one of its neighbours: the branch of the asin"""
    return np.array(_hitting(np.sqrt, 0.25, HALF3, 8), F32)


def u0_for_c2_half(rough32):
    """u0 around the branch of the acos, sqrt(c2) = 0.5, at this roughness: the seven float32 values about the solution of c2(u0) = 0.25 (u0's grid is
    coarser than sqrt(c2)'s there, so 0.5 and its neighbours are not all attainable: these are the closest arguments there are), and whichever u0 nearby do
    give 0.5 or a neighbour exactly.  At r = 0.02 the solution lies above 1 - 2^-24: sqrt(c2) >= 0.52 for every u0 a draw can take."""
    a2 = float(alpha2(rough32))
    guess = 0.75 / (1.0 + 0.25 * (a2 - 1.0))
    fn = lambda x: prefix_specular(np.stack([x, x], -1), rough32)[0]
    x = _near(min(guess, float(TOP)), 3)
    return np.unique(np.array(list(x[x <= TOP]) + _hitting(fn, guess, HALF3, 256), F32))


def phi_specials():
    """float32(k pi / 4), k = 0..8, and their neighbours: the multiples of pi/2 and the angles at which the sincos changes quadrant"""
    out = [F32(0)]
    for k in range(1, 9):
        out += list(_near(F32(k * np.pi / 4), 1))
    out = np.array(out, F32)
    return out[out <= TWO_PI_F]


def u1_for_phi_specials():
    """u1 < 1 whose phi = f32(2 pi) u1 is one of phi_specials() where one exists, and the seven u1 about every k / 8 (phi's grid is coarser than u1's
    image there: the closest azimuths there are on both sides of every multiple of pi / 4); plus 0 and the smallest float32 values"""
    out = [F32(0), F32(2.0 ** -149), F32(2.0 ** -126)]
    for p in phi_specials()[1:]:
        out += _hitting(lambda x: TWO_PI_F * x, float(p) / float(TWO_PI_F), (p,), 8)
    for k in range(1, 9):
        x = _near(F32(k / 8), 3)
        out += list(x[x <= TOP])
    return np.unique(np.array(out, F32))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def normals_table(rng, n_rows):
    n = _unit(rng.normal(size=(n_rows, 3)))
    n[: n_rows // 4] = (0.0, 0.0, 1.0)
    fixed = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1)]
    o = n_rows // 4
    for v in fixed:
        n[o:o + 16] = v
        o += 16
    n32 = n.astype(F32)
    for x in _near(0.1, 1):                                     # |n.x| at the frame's threshold 0.1f and its neighbours, renormalised through y and z
        for sgn in (1.0, -1.0):
            a = rng.uniform(0, 2 * np.pi, 32)
            s = np.sqrt(1.0 - float(x) ** 2)
            n32[o:o + 32] = np.stack([np.full(32, sgn * float(x)), s * np.cos(a), s * np.sin(a)], -1).astype(F32)
            n32[o:o + 32, 0] = F32(sgn) * x
            o += 32
    return n32[rng.permutation(n_rows)]


def directions_about(rng, n32):
    """normalize(n + 0.8 N(0,1)) (about 11 % below the horizon); 256 rows equal to n; 128 rows each with n.d = 1e-3, 1e-4, 0"""
    n = n32.astype(np.float64)
    B_ = len(n)
    d = _unit(n + 0.8 * rng.normal(size=(B_, 3)))
    rows = rng.permutation(B_)
    d[rows[:256]] = n[rows[:256]]
    o = 256
    for c in (1e-3, 1e-4, 0.0):
        i = rows[o:o + 128]
        t = _unit(np.cross(n[i], rng.normal(size=(128, 3))))
        d[i] = np.sqrt(1 - c * c) * t + c * n[i]
        o += 128
    return d.astype(F32)


def uniforms_table(rng, n_rows, rough=None):
    """-> u2 (n_rows, 2), level (n_rows) index into ROUGH_LEVELS.  rough: one level (every row gets it) or None (one per row, the rows that plant
    sqrt(c2) = 0.5 getting the level they were solved for)."""
    levels = list(range(len(ROUGH_LEVELS))) if rough is None else [ROUGH_LEVELS.index(F32(rough))]
    u2 = rng.random((n_rows, 2), dtype=F32)
    level = rng.choice(levels, n_rows)
    o = 0
    g = np.array(GRID, F32)
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    for _ in range(8):                                          # the full grid, eight times (so that every pair meets several normals)
        u2[o:o + len(grid)] = grid
        o += len(grid)
    u1s = u1_for_phi_specials()
    for lv in [None] + levels:
        u0s = u0_for_sqrt_half() if lv is None else u0_for_c2_half(ROUGH_LEVELS[lv])
        for u0 in u0s:
            k = 8
            u2[o:o + k, 0] = u0
            u2[o + 4:o + k, 1] = rng.choice(u1s, 4)
            if lv is not None:
                level[o:o + k] = lv
            o += k
    for u1 in u1s:
        u2[o:o + 8, 1] = u1
        u2[o + 4:o + 8, 0] = rng.choice(g, 4)
        o += 8
    assert o < n_rows // 2
    p = rng.permutation(n_rows)
    return u2[p], level[p]


@functools.lru_cache(maxsize=None)
def sampler_case(rough=None, seed=0):
    """u2, normal, wo and the per-row roughness for the samplers; rough: a level (scalar calls) or None (one level per row)"""
    rng = np.random.default_rng([seed, 0 if rough is None else 1 + ROUGH_LEVELS.index(F32(rough))])
    u2, level = uniforms_table(rng, B, rough)
    n = normals_table(rng, B)
    return _frozen({"u2": u2, "normal": n, "wo": directions_about(rng, n), "rough": np.array(ROUGH_LEVELS, F32)[level], "level": level})


def _materials(rng, n_rows):
    albedo = rng.random((n_rows, 3), dtype=F32)
    metal = rng.random(n_rows, dtype=F32)
    which = rng.integers(0, 4, n_rows)
    metal[which == 0] = 0.0
    metal[which == 1] = 1.0
    return albedo, metal


@functools.lru_cache(maxsize=None)
def eval_case(seed=1):
    rng = np.random.default_rng([seed, 100])
    n = normals_table(rng, B)
    wo = directions_about(rng, n)
    wi = directions_about(rng, n)
    n64, wo64 = n.astype(np.float64), wo.astype(np.float64)
    mirror = 2 * _dot(n64, wo64)[:, None] * n64 - wo64
    rows = rng.permutation(B)[: B // 4]                          # a quarter near the mirror direction, 64 of them exactly on it
    near = _unit(mirror[rows] + rng.normal(size=(len(rows), 3)) * np.exp(rng.uniform(-12, -1, (len(rows), 1))))
    near[:64] = mirror[rows[:64]]
    wi[rows] = near.astype(F32)
    level = rng.integers(0, len(ROUGH_LEVELS), B)
    albedo, metal = _materials(rng, B)
    return _frozen({"wi": wi, "wo": wo, "normal": n, "rough": np.array(ROUGH_LEVELS, F32)[level], "level": level, "albedo": albedo, "metal": metal})


S1_SPECIALS = (F32(0), HALF3[0], HALF3[1], HALF3[2], TOP)


@functools.lru_cache(maxsize=None)
def brdf_sample_case(seed=2):
    c = dict(sampler_case(None, seed))
    rng = np.random.default_rng([seed, 200])
    s1 = rng.random(B, dtype=F32)
    for k, v in enumerate(S1_SPECIALS):
        s1[k * 1024:(k + 1) * 1024] = v
    c["s1"] = s1
    c["albedo"], c["metal"] = _materials(rng, B)
    return _frozen(c)


EMITTER_CONFIGS = ((1, None), (1, 0), (2, 0), (3, 1), (7, 3))        # (K emitters, which one has area 0)


def emitter_tables(K, zero, seed=3):
    """Everything but the cdf, which the tests take from the model (emitter_pdf.cumsum): emitters are the odd faces of 2K + 1"""
    rng = np.random.default_rng([seed, 300, K, K if zero is None else zero])
    verts = rng.uniform(-1, 1, (K, 1, 3)) + rng.uniform(-0.5, 0.5, (K, 3, 3))
    if zero is not None:
        verts[zero, 2] = 0.5 * (verts[zero, 0] + verts[zero, 1])
    verts = verts.astype(F32)
    v = verts.astype(np.float64)
    area = (0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=-1)).astype(F32)
    if zero is not None:
        area[zero] = 0.0
    is_emitter = np.zeros(2 * K + 1, bool)
    is_emitter[1::2] = True
    return {"key": (K, zero), "K": K, "verts": verts, "area": area, "is_emitter": is_emitter, "triangle_idx": np.nonzero(is_emitter)[0].astype(np.int64),
            "emitter_pdf": F32(1) / F32(K)}


def emitter_case(em, seed=3):
    """em: emitter_tables(...) with em['cdf'] filled in.  s1: 0, every cdf entry and its two neighbours, 1 - 2^-24, and random draws."""
    K = em["K"]
    rng = np.random.default_rng([seed, 301, K])
    s1 = rng.random(B, dtype=F32)
    sp = [F32(0), TOP] + [x for c in em["cdf"] for x in _near(c, 1)]
    sp = np.array([x for x in sp if 0 <= x <= TOP], F32)
    s1[: len(sp) * 64] = np.repeat(sp, 64)
    s2 = uniforms_table(rng, B)[0]
    pos = (_unit(rng.normal(size=(B, 3))) * rng.uniform(4, 6, (B, 1))).astype(F32)
    return _frozen({"s1": s1, "s2": s2, "position": pos})


@functools.lru_cache(maxsize=None)
def frame_case(seed=4):
    rng = np.random.default_rng([seed, 400])
    n = normals_table(rng, B).copy()
    n[:8] = 0.0                                                 # the zero normal: finite output
    return _frozen({"normal": n})


@functools.lru_cache(maxsize=None)
def lerp_case(R, seed=5):
    rng = np.random.default_rng([seed, 500, R])
    spec = (rng.normal(size=(B, R, 3)) * np.exp(rng.uniform(-3, 6, (B, R, 1)))).astype(F32)
    rough = rng.uniform(0.02, 1.0, B).astype(F32)
    sp = [F32(0.02)] + list(_near(0.02, 2)) + [F32(0), F32(0.01), F32(-0.5), F32(-7.3), np.nextafter(F32(1), F32(2)), F32(1.5), F32(3), F32(40.25)]
    for k in range(R if R > 1 else 0):
        sp += list(_near(F32(0.02 + k * 0.98 / (R - 1)), 2))
    sp = np.array(sp, F32)
    rough[: len(sp) * 32] = np.repeat(sp, 32)
    return _frozen({"spec": spec, "rough": rough})


@functools.lru_cache(maxsize=None)
def angle_case(seed=6):
    rng = np.random.default_rng([seed, 600])
    theta = np.minimum((rng.random(B, dtype=F32) * PIO2_F), PIO2_F)
    phi = np.minimum(rng.random(B, dtype=F32) * TWO_PI_F, TWO_PI_F)
    tsp = np.array([F32(0), PIO2_F, np.nextafter(PIO2_F, F32(0)), F32(2.0 ** -149), F32(2.0 ** -126), F32(1e-4)] + list(_near(F32(np.pi / 4), 2)), F32)
    psp = phi_specials()
    theta[: len(tsp) * 64] = np.repeat(tsp, 64)
    phi[: len(psp) * 64] = np.tile(psp, 64)
    theta = theta[rng.permutation(B)]
    theta[-len(psp) * len(tsp):] = np.repeat(tsp, len(psp))           # every special polar angle with every special azimuth
    phi[-len(psp) * len(tsp):] = np.tile(psp, len(tsp))
    return _frozen({"theta": theta, "phi": phi})


# ============================================================================================================ the checks
def envelope(fn, c, den=None, rising=()):
    """fn(c, dden=...) -> (B, M) in float64.  Returns (f, tol, open_above), all (B, M).

    den (B): the GGX denominator of the rows, for functions that carry D_GGX.  The formula above takes the ends of the perturbation box, which bound f
    over the box only while f is monotone on it.  D has a pole at den = 0, and on a row whose box reaches it -- den <= 2 NoH d + 4 u, about
    20 u: only at r = 0.02, alpha^2 = 2.7 u -- the float32 denominator may land anywhere in [0, den + ...], so the supremum of D over the box is unbounded,
    whatever the ends give.  (Evidence, sample_specular at r = 0.02, u2 = (0.65209824, 0.5178346): float64 NoH = 0.99999983, den = 8.3 u, pdf 6.58e4; the
    libm oracle, the device-arithmetic oracle and the float32 restatement all form NoH = 1.0f, 2.8 u off and inside d, hence den = 3 u and pdf 5.05e5, while the
    box's ends give tol = 2.4e5.)  On such rows the columns listed in `rising` (those that grow with D) are open above: the value may exceed f by any
    amount but must not fall below f - tol; the other columns get the far end of the box, den -> 0+, as one more term of tol."""
    with np.errstate(all="ignore"):
        f = fn(c, dden=0.0)
        tol = 16 * U * np.abs(f)
        for i in range(c.shape[1]):
            e = np.zeros(c.shape[1])
            e[i] = DELTA
            tol = tol + np.maximum(np.abs(fn(c + e, dden=0.0) - f), np.abs(fn(c - e, dden=0.0) - f))
        tol = tol + np.maximum(np.abs(fn(c, dden=4 * U) - f), np.abs(fn(c, dden=-4 * U) - f))
        open_above = np.zeros(f.shape, bool)
        if den is not None:
            pole = den - (2 * np.maximum(c[:, 3], 0) * DELTA + 4 * U) <= 0
            if pole.any():
                far = np.abs(fn(c, dden=np.where(pole, 1e-30 - den, 0.0)) - f)
                cols = np.zeros(f.shape[1], bool)
                cols[list(rising)] = True
                open_above = pole[:, None] & cols[None, :]
                tol = tol + np.where(pole[:, None] & ~cols[None, :], far, 0.0)
    return f, np.where(np.isfinite(tol), tol, np.inf), open_above


def envelope_report(got, f, tol, open_above=None):
    """-> (rows outside the envelope (finite values only), worst |err| / tol, uninformative (B, M) mask: tol > 1e-3 |f| + 1e-6 or open above)"""
    got = np.asarray(got, np.float64).reshape(f.shape)
    open_above = np.zeros(f.shape, bool) if open_above is None else open_above
    fin = np.isfinite(got)
    with np.errstate(all="ignore"):
        err = np.abs(got - f)
        ok = (err <= tol) | (open_above & (got >= f))
        bad = fin & ~ok
        ratio = np.where(fin & (tol > 0) & np.isfinite(tol) & ~(open_above & (got >= f)), err / np.where(tol > 0, tol, 1.0), 0.0)
    return bad, float(ratio.max()) if ratio.size else 0.0, (tol > 1e-3 * np.abs(f) + 1e-6) | open_above


def assert_inside(name, got, f, tol, open_above=None, log=None):
    bad, worst, uninf = envelope_report(got, f, tol, open_above)
    if log is not None:
        log(f"{name}: rows outside the envelope {int(bad.any(-1).sum())} of {len(f)}, worst |err|/tol {worst:.3f}, "
            f"uninformative {100.0 * uninf.any(-1).mean():.2f} %")
    rows = np.nonzero(bad.any(-1))[0]
    assert rows.size == 0, (f"{name}: {rows.size} rows outside the envelope, first {rows[:5].tolist()}: got "
                            f"{np.asarray(got, np.float64).reshape(f.shape)[rows[:5]].tolist()} f64 {f[rows[:5]].tolist()} tol {tol[rows[:5]].tolist()}")
    return uninf


def assert_nonfinite_rule(name, got, c, rough32, level):
    """Non-finite values only at r = 0.02, only where the float64 den = NoH^2 (alpha^2 - 1) + 1 <= 24 u (the float32 denominator can round to 0 there; the
    reference's own outputs hold inf on such rows), and on at most 1 % of that level's rows."""
    nf = ~np.isfinite(np.asarray(got, np.float64).reshape(len(c), -1)).all(-1)
    if not nf.any():
        return 0
    allowed = (np.asarray(rough32, F32) == ROUGH_LEVELS[0]) & (ggx_den(c, rough32) <= 24 * U)
    allowed = np.broadcast_to(allowed, nf.shape)
    assert not (nf & ~allowed).any(), f"{name}: non-finite values on rows {np.nonzero(nf & ~allowed)[0][:8].tolist()} where the GGX denominator is not degenerate"
    n_level = int((np.broadcast_to(level, nf.shape) == 0).sum())
    assert nf.sum() <= 0.01 * n_level, f"{name}: {int(nf.sum())} non-finite rows of {n_level} at r = 0.02"
    return int(nf.sum())


def assert_cap(name, uninf, level, cap):
    """at most `cap` of every roughness level's rows may be uninformative"""
    level = np.broadcast_to(level, uninf.shape[:1])
    for lv in np.unique(level):
        frac = uninf[level == lv].any(-1).mean()
        assert frac <= cap, f"{name}: {100 * frac:.2f} % of the rows at r = {ROUGH_LEVELS[lv]} are uninformative (cap {100 * cap:.1f} %)"


def direction_error(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max())


def assert_unit(name, wi):
    n = np.linalg.norm(np.asarray(wi, np.float64), axis=-1)
    assert np.abs(n - 1).max() <= 4 * U, f"{name}: | |wi| - 1 | = {np.abs(n - 1).max() / U:.2f} u"


class Bounds:
    """E of a case: the largest direction error, against the float64 reference, of the libm oracle and of the float32 run of the restatement on that
    case's table.  The code under test must stay within 2 E: its asin / sincos may differ from libm's by an ulp of the angle, and the angle and the
    trigonometric result each contribute at most that much again."""
    E_MAX = 1e-6      # a guard on the yardstick itself (observed: <= 6.0e-7); E is a property of float32, not of the code under test

    def __init__(self, oracle_mod):
        self.backs = (Oracle(oracle_mod, 0), Numpy32())
        self.E = {}

    def measure(self, key, run, ref):
        """run(backend) -> directions; ref: the float64 reference.  Cached per key."""
        if key not in self.E:
            e = max(direction_error(run(b), ref) for b in self.backs)
            assert 0 < e <= self.E_MAX, f"E[{key}] = {e:.3g}: the yardstick itself is off"
            self.E[key] = e
        return self.E[key]


# ---------------------------------------------------------------------------------------------------- one function per operation under test
def check_sample_diffuse(back, bounds, log=print):
    c = sampler_case(ROUGH_LEVELS[0], seed=10)
    run = lambda b: b.sample_diffuse(c["u2"], c["normal"])[0]
    ref = diffuse_dir(c["u2"], c["normal"])
    assert np.isfinite(ref).all()
    E = bounds.measure("sample_diffuse", run, ref)
    wi, pdf, w = back.sample_diffuse(c["u2"], c["normal"])
    err = direction_error(wi, ref)
    log(f"sample_diffuse[{back.name}]: direction error {err:.3g}, E {E:.3g}")
    assert err <= 2 * E
    assert_unit("sample_diffuse", wi)
    f, tol, _ = envelope(lambda x, dden: f_cos_pdf(x), _dot(c["normal"].astype(np.float64), wi.astype(np.float64))[:, None])
    uninf = assert_inside(f"sample_diffuse pdf[{back.name}]", pdf, f, tol, log=log)
    assert uninf.mean() <= 0.005
    assert np.array_equal(np.asarray(w), np.ones((B, 3), F32))
    return E


def _check_spec_outputs(name, c, rough, wi, pdf, g0, g1, log):
    cs = cosines(wi, c["wo"], c["normal"])
    f, tol, above = envelope(lambda x, dden: f_spec(x, rough, dden=dden), cs, ggx_den(cs, rough), rising=(0,))
    got = np.concatenate([np.asarray(a, F32).reshape(-1, 1) for a in (pdf, g0, g1)], -1)
    n_nf = assert_nonfinite_rule(name, got, cs, rough, c["level"])
    uninf = assert_inside(name, got, f, tol, above, log)
    assert_cap(name + " g0/g1", uninf[:, 1:], c["level"], 0.005)         # (the pdf of the sampled lobe sits on its peak: no cap, eval_brdf carries that)
    return n_nf


def check_sample_specular(back, bounds, rough, log=print):
    c = sampler_case(rough, seed=11)
    run = lambda b: b.sample_specular(c["u2"], c["wo"], c["normal"], rough)[0]
    ref = specular_dir(c["u2"], c["wo"], c["normal"], rough)
    assert np.isfinite(ref).all()
    E = bounds.measure(("sample_specular", float(rough)), run, ref)
    wi, pdf, g0, g1 = back.sample_specular(c["u2"], c["wo"], c["normal"], rough)
    err = direction_error(wi, ref)
    log(f"sample_specular[{back.name}, r = {rough}]: direction error {err:.3g}, E {E:.3g}")
    assert err <= 2 * E
    assert_unit("sample_specular", wi)
    _check_spec_outputs(f"sample_specular[{back.name}, r = {rough}]", c, rough, wi, pdf, g0, g1, log)
    return E


def check_sample_specular_rows(back, bounds, log=print):
    c = sampler_case(None, seed=12)
    run = lambda b: b.sample_specular_v(c["u2"], c["wo"], c["normal"], c["rough"])[0]
    ref = specular_dir(c["u2"], c["wo"], c["normal"], c["rough"])
    E = bounds.measure("sample_specular_v", run, ref)
    wi, pdf, g0, g1 = back.sample_specular_v(c["u2"], c["wo"], c["normal"], c["rough"])
    err = direction_error(wi, ref)
    log(f"sample_specular_v[{back.name}]: direction error {err:.3g}, E {E:.3g}")
    assert err <= 2 * E
    assert_unit("sample_specular_v", wi)
    _check_spec_outputs(f"sample_specular_v[{back.name}]", c, c["rough"], wi, pdf, g0, g1, log)
    return E


def check_eval_brdf(back, log=print):
    c = eval_case()
    brdf, pdf = back.eval_brdf(c["wi"], c["wo"], c["normal"], c["albedo"], c["rough"], c["metal"])
    cs = cosines(c["wi"], c["wo"], c["normal"])
    f, tol, above = envelope(lambda x, dden: f_brdf(x, c["rough"], c["albedo"], c["metal"], dden=dden), cs, ggx_den(cs, c["rough"]), rising=(0, 1, 2, 3))
    got = np.concatenate([np.asarray(pdf, F32).reshape(-1, 1), np.asarray(brdf, F32).reshape(-1, 3)], -1)
    name = f"eval_brdf[{back.name}]"
    assert_nonfinite_rule(name, got, cs, c["rough"], c["level"])
    uninf = assert_inside(name, got, f, tol, above, log)
    assert_cap(name + " pdf", uninf[:, :1], c["level"], 0.25)
    assert_cap(name + " brdf", uninf[:, 1:], c["level"], 0.25)


def check_sample_brdf(back, bounds, log=print):
    c = brdf_sample_case()
    args = (c["s1"], c["u2"], c["wo"], c["normal"], c["albedo"], c["rough"], c["metal"])
    diffuse = c["s1"] > F32(0.5)                                  # 0.5 itself takes the specular lobe, the next value up the diffuse one
    assert not diffuse[c["s1"] == HALF3[1]].any() and diffuse[c["s1"] == HALF3[2]].all() and (c["s1"] == HALF3[1]).sum() >= 1024
    ref = np.where(diffuse[:, None], diffuse_dir(c["u2"], c["normal"]), specular_dir(c["u2"], c["wo"], c["normal"], c["rough"]))
    E = bounds.measure("sample_brdf", lambda b: b.sample_brdf(*args)[0], ref)
    wi, pdf, w = back.sample_brdf(*args)
    name = f"sample_brdf[{back.name}]"
    wi, pdf, w = np.asarray(wi, F32), np.asarray(pdf, F32).reshape(-1, 1), np.asarray(w, F32)
    # which lobe: a row that took the other lobe is off by the distance between the two directions, which is above 1e-3 on all but a few rows
    err_rows = np.abs(wi.astype(np.float64) - ref).max(-1)
    other = np.where(diffuse[:, None], specular_dir(c["u2"], c["wo"], c["normal"], c["rough"]), diffuse_dir(c["u2"], c["normal"]))
    apart = np.abs(other - ref).max(-1) > 1e-3
    for v in S1_SPECIALS:
        assert apart[c["s1"] == v].sum() >= 900
    assert (err_rows[apart] <= 2 * E).all(), f"{name}: rows {np.nonzero(apart & (err_rows > 2 * E))[0][:8].tolist()} took the other lobe"
    err = float(err_rows.max())
    log(f"{name}: direction error {err:.3g}, E {E:.3g}")
    assert err <= 2 * E
    assert_unit(name, wi)
    cs = cosines(wi, c["wo"], c["normal"])
    den = ggx_den(cs, c["rough"])
    f, tol, above = envelope(lambda x, dden: f_brdf(x, c["rough"], c["albedo"], c["metal"], dden=dden)[:, :1], cs, den, rising=(0,))
    assert_nonfinite_rule(name + " pdf", pdf, cs, c["rough"], c["level"])
    assert_inside(name + " pdf", pdf, f, tol, above, log)
    assert not np.isnan(w).any(), f"{name}: NaN weight"
    zero = (pdf[:, 0] == 0)
    assert (w[zero] == 0).all(), f"{name}: weight != 0 where the returned pdf is 0"
    live = ~zero & np.isfinite(pdf[:, 0])
    f, tol, _ = envelope(lambda x, dden: f_weight(x, c["rough"], c["albedo"], c["metal"], dden=dden), cs, den)
    assert_inside(name + " weight", w[live], f[live], tol[live], log=log)
    return E


def check_sample_emitter(back, bounds, em, log=print):
    c = emitter_case(em)
    K = em["K"]
    o = emitter_ordinal(em["cdf"], c["s1"])
    assert set(o.tolist()) == set(range(K))
    ref = emitter_dir(em["verts"], o, c["s2"], c["position"])
    run = lambda b: b.sample_emitter(em, c["s1"], c["s2"], c["position"])
    E = bounds.measure(("sample_emitter",) + em["key"], lambda b: run(b)[0], ref)
    wi, pdf, tri = run(back)
    name = f"sample_emitter[{back.name}, K = {K}, area-0 emitter {em['key'][1]}]"
    np.testing.assert_array_equal(np.asarray(tri).reshape(-1), em["triangle_idx"][o], err_msg=name)
    err = direction_error(wi, ref)
    log(f"{name}: direction error {err:.3g}, E {E:.3g}")
    assert err <= 2 * E
    assert_unit(name, wi)
    want = float(em["emitter_pdf"]) / np.maximum(em["area"][o].astype(np.float64), float(F32(1e-12)))
    assert (np.abs(np.asarray(pdf, np.float64).reshape(-1) - want) <= 2 * U * want).all(), name + " pdf"
    return E


def check_get_normal_space(back, log=print):
    c = frame_case()
    n32 = c["normal"]
    fr = np.asarray(back.get_normal_space(n32), F32)
    name = f"get_normal_space[{back.name}]"
    assert np.isfinite(fr).all(), name
    np.testing.assert_array_equal(fr[:, :, 2], n32)
    t, b, n = fr[8:, :, 0].astype(np.float64), fr[8:, :, 1].astype(np.float64), n32[8:].astype(np.float64)
    small = np.abs(n32[8:, 0]) <= F32(0.1)                      # the branch: cross((1,0,0), n) has no x, cross((0,1,0), n) no y
    assert small[n32[8:, 0] == F32(0.1)].all() and not small[n32[8:, 0] == np.nextafter(F32(0.1), F32(1))].any() and (n32[8:, 0] == F32(0.1)).sum() >= 32
    assert (t[small, 0] == 0).all() and (t[~small, 1] == 0).all(), name + ": wrong branch"
    worst = max(np.abs(np.linalg.norm(t, axis=-1) - 1).max(), np.abs(np.linalg.norm(b, axis=-1) - 1).max(),
                np.abs(_dot(t, n)).max(), np.abs(_dot(t, b)).max(), np.abs(_dot(b, n)).max())
    log(f"{name}: worst departure from an orthonormal frame {worst / U:.2f} u")
    assert worst <= 8 * U
    assert np.abs(b - np.cross(n, t)).max() <= 2 * U, name + ": b != n x t"
    t64, _ = normal_space(n32[8:], np.float64)
    assert np.abs(t - t64).max() <= 4 * U, name + ": tangent"


def check_lerp_specular(back, R, log=print):
    c = lerp_case(R)
    ref, tol = lerp_specular(c["spec"], c["rough"])
    r0, r1, w = lerp_plan(c["rough"], R)
    assert set(r0.tolist()) == set(range(R)) and set(r1.tolist()) == set(range(R)) and (w == 0).sum() >= 32
    got = np.asarray(back.lerp_specular(c["spec"], c["rough"]), np.float64)
    bad = ~(np.abs(got - ref) <= tol)
    log(f"lerp_specular[{back.name}, R = {R}]: worst |err|/tol {float((np.abs(got - ref) / np.maximum(tol, 1e-300)).max()):.3f}")
    assert not bad.any(), f"lerp_specular[{back.name}, R = {R}]: rows {np.nonzero(bad.any(-1))[0][:8].tolist()}, roughness {c['rough'][bad.any(-1)][:8].tolist()}"


def check_angle2xyz(back, bounds, log=print):
    c = angle_case()
    ref = angle2xyz(c["theta"], c["phi"], np.float64)
    E = bounds.measure("angle2xyz", lambda b: b.angle2xyz(c["theta"], c["phi"]), ref)
    got = back.angle2xyz(c["theta"], c["phi"])
    err = direction_error(got, ref)
    log(f"angle2xyz[{back.name}]: direction error {err:.3g}, E {E:.3g}")
    assert err <= 2 * E
    assert_unit("angle2xyz", got)
    return E


# ============================================================================================================ the reference checks itself
def _gauss(a, b, n=48):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (b - a) * x + 0.5 * (a + b), 0.5 * (b - a) * w


def _panels(hi, first):
    """[0, hi] cut into panels that double from `first`: the GGX peak at r = 0.02 is 4e-4 rad wide"""
    edges = [0.0]
    e = first
    while e < hi:
        edges.append(e)
        e *= 2
    return edges + [hi]


def ggx_cdf(theta, rough):
    """integral of D(h) (n.h) over the cap of half angle theta, by Gauss-Legendre quadrature (float64, alpha^2 = r^4)"""
    a2 = float(rough) ** 4
    total = 0.0
    ed = _panels(float(theta), a2 ** 0.5 / 8)
    for a, b in zip(ed[:-1], ed[1:]):
        x, w = _gauss(a, b)
        mu = np.cos(x)
        D = a2 / (np.pi * (np.sin(x) ** 2 + a2 * mu * mu) ** 2)               # mu^2 (a2 - 1) + 1 without its cancellation
        total += float((w * D * mu * np.sin(x) * 2 * np.pi).sum())
    return total


def cosine_pdf_integral():
    x, w = _gauss(0.0, np.pi / 2)
    return float((w * (np.cos(x) / np.pi) * np.sin(x) * 2 * np.pi).sum())
