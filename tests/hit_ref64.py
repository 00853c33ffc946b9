"""The closest hit against exact geometry (numpy only: no oracle, no HIP).  Shared by tests/test_hit_ref64_cpu.py (the oracle, BVH and brute force, and
the float32 run of the restatement below) and tests/test_hit_ref64.py (the HIP traversal in both node layouts).

exact_hits      float64 Moeller-Trumbore in Pluecker form (five K = 3 matrix products per block of rays) over ALL triangles: the ray-plane
                parameter t* and the barycentrics b* of every (ray, triangle) pair.  The float32 inputs are exact in float64; coordinates are
                taken relative to a float32 centre of the scene, so an offset of 1024 costs nothing.  It is not the Woop test of DESIGN.md section 2
                and shares no step with it.  exact_one is the same quantity for ONE triangle per ray by plain cross products relative to the
                ray's origin (test_reference_checks_itself holds the two together).
restated_hit    DESIGN.md section 2 operation by operation, brute force, in float32 or float64.  Nothing is asserted equal to it: its float32 run
                against exact_hits is the rounding floor E of each quantity, and the constants of every bound are C = 4 E (measure_E, constants).
check_hits      soundness of every reported hit, completeness of every ray, the tie rule, and the shares of rows for which a bound says nothing.

Per-row units, all from the float64 geometry of the triangle k in question and the ray (u = 2^-24):
    R = max_i |P_i - o|_inf       L = longest edge       h = |N.d| / L  (the height of the triangle as the ray sees it)       M_p = max_i |P_i|_inf
    unit_b = u R / h     unit_t = u R L / h     unit_p = u (M_p + R L / h)     unit_plane = u M_p     unit_n = u L^2 / |N|
unit_n is not a bare u: float32 edges p1 - p0, p2 - p0 carry u L each, so their cross product turns by u L^2 / |N|, which is
1.2 u for an equilateral triangle and 10^4 u for the needles (p2 within 1e-4 of p1) of the soups; in the bare unit E_n was 1.5e4 on that input.

E, measured when the tests run (numpy's float32 arithmetic is IEEE, so these should not move), max over the inputs of INPUTS below:
    E_t = 3.93   E_b = 1.77   E_p = 2.35   E_plane = 2.62   E_n = 1.49          =>  C = 4 E
"""
import functools

import numpy as np

U = 2.0 ** -24
VACUOUS = 2.0 ** -10            # rows with unit_t > VACUOUS * R (L / h > 2^14: degenerate or edge-on) make the t, uv and min(b) bounds vacuous
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------ exact geometry, float64
class Geometry:
    """per-triangle float64 quantities; coordinates relative to a float32 centre (P - c is exact in float64)"""

    def __init__(self, verts, faces):
        assert verts.dtype == F32
        self.verts, self.faces = verts, np.asarray(faces, np.int64).reshape(-1, 3)
        self.c = (0.5 * (verts.min(0) + verts.max(0))).astype(F32).astype(F64) if len(verts) else np.zeros(3)
        self.Pabs = verts.astype(F64)[self.faces]                               # (T, 3 vertices, 3)
        self.P = self.Pabs - self.c
        self.e1, self.e2 = self.P[:, 1] - self.P[:, 0], self.P[:, 2] - self.P[:, 0]
        self.N = np.cross(self.e1, self.e2)
        self.Nlen = np.linalg.norm(self.N, axis=-1)
        e3 = self.P[:, 2] - self.P[:, 1]
        self.L = np.sqrt(np.maximum(np.maximum((self.e1 ** 2).sum(-1), (self.e2 ** 2).sum(-1)), (e3 ** 2).sum(-1)))
        self.Mp = np.abs(self.Pabs).max((1, 2)) if len(self.faces) else np.zeros(0)
        bits = np.ascontiguousarray(verts[self.faces].reshape(-1, 9)).view(np.uint32)
        if len(bits):                                                            # the smallest index among the bitwise duplicates of each triangle
            _, first, inv = np.unique(bits, axis=0, return_index=True, return_inverse=True)
            self.first_dup = first[inv.reshape(-1)]
        else:
            self.first_dup = np.zeros(0, np.int64)


def exact_hits(verts, faces, o, d, geom=None):
    """t* (B, T), b* (3, B, T) and the unnormalised plane normals N (T, 3) of every ray against every triangle; inf / nan where N.d = 0"""
    g = geom or Geometry(verts, faces)
    oc, dd = o.astype(F64) - g.c, d.astype(F64)
    m = np.cross(oc, dd)                                                         # the ray's moment
    P0 = g.P[:, 0]
    with np.errstate(all="ignore"):
        det = -(dd @ g.N.T)                                                      # e1 . (d x e2)
        t = (oc @ g.N.T - (P0 * g.N).sum(-1)) / det
        b1 = (m @ g.e2.T - (dd @ np.cross(g.e2, P0).T)) / det
        b2 = ((dd @ np.cross(g.e1, P0).T) - m @ g.e1.T) / det
    return t, np.stack([(1.0 - b1) - b2, b1, b2]), g.N


def exact_one(g, o, d, k):
    """t*, b* (3, B) of triangle k[i] for ray i, by cross products relative to the ray's origin"""
    o64, d64 = o.astype(F64), d.astype(F64)
    A = g.Pabs[k] - o64[:, None, :]                                              # exact: float32 - float32 in float64
    e1, e2 = A[:, 1] - A[:, 0], A[:, 2] - A[:, 0]
    pv = np.cross(d64, e2)
    with np.errstate(all="ignore"):
        det = (e1 * pv).sum(-1)
        tv = -A[:, 0]
        b1 = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        b2 = (d64 * qv).sum(-1) / det
        t = (e2 * qv).sum(-1) / det
    return t, np.stack([(1.0 - b1) - b2, b1, b2])


def units(g, o, d, k):
    """the per-row units of triangle k[i] for ray i"""
    o64, d64 = o.astype(F64), d.astype(F64)
    R = np.abs(g.Pabs[k] - o64[:, None, :]).max((1, 2))
    with np.errstate(all="ignore"):
        h = np.abs((g.N[k] * d64).sum(-1)) / g.L[k]
        Loh = g.L[k] / h
        un = U * g.L[k] ** 2 / g.Nlen[k]
        return dict(R=R, b=U * R / h, t=U * R * Loh, p=U * (g.Mp[k] + R * Loh), plane=U * g.Mp[k], n=un)


# ------------------------------------------------------------------------------------------------------------------ DESIGN.md section 2, restated
def _fma(a, b, c, dt):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(dt)           # float32: exact product, the sum rounded to double, then once more


def restated_hit(verts, faces, o, d, dtype=F32, chunk=256):
    """brute-force closest hit by the contract of DESIGN.md section 2 in `dtype`; returns dict(idx, valid, t, uv, p, n) as ray_intersect does"""
    dt = np.dtype(dtype).type
    wide = F64 if dt is F32 else np.longdouble                                   # the re-evaluation of the edge functions where one is 0
    B, T = len(o), len(faces)
    V, Fc, o_, d_ = verts.astype(dt), np.asarray(faces, np.int64).reshape(-1, 3), o.astype(dt), d.astype(dt)
    idx, t_out = np.full(B, -1, np.int64), np.full(B, np.inf, dt)
    uv, p, n = np.zeros((B, 2), dt), np.zeros((B, 3), dt), np.zeros((B, 3), dt)
    if T and B:
        P = V[Fc]                                                                # (T, 3 vertices, 3)
        ad = np.abs(d_)
        kz_all = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
        for kz in range(3):
            kx = (kz + 1) % 3; ky = (kx + 1) % 3
            rows_k = np.nonzero(kz_all == kz)[0]
            for s in range(0, len(rows_k), chunk):
                r = rows_k[s:s + chunk]
                with np.errstate(all="ignore"):
                    sz = (dt(1) / d_[r, kz])[:, None]
                    sx, sy = d_[r, kx][:, None] * sz, d_[r, ky][:, None] * sz
                    xy = []
                    zs = []
                    for i in range(3):
                        z = P[None, :, i, kz] - o_[r, kz][:, None]
                        xy.append((_fma(-sx, z, P[None, :, i, kx] - o_[r, kx][:, None], dt), _fma(-sy, z, P[None, :, i, ky] - o_[r, ky][:, None], dt)))
                        zs.append(z)
                    (Ax, Ay), (Bx, By), (Cx, Cy) = xy
                    Uu, Vv, Ww = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
                    zero = np.minimum(np.minimum(np.abs(Uu), np.abs(Vv)), np.abs(Ww)) == 0
                    if zero.any():
                        w = lambda a: a[zero].astype(wide)
                        Uu[zero] = (w(Cx) * w(By) - w(Cy) * w(Bx)).astype(dt)
                        Vv[zero] = (w(Ax) * w(Cy) - w(Ay) * w(Cx)).astype(dt)
                        Ww[zero] = (w(Bx) * w(Ay) - w(By) * w(Ax)).astype(dt)
                    det = (Uu + Vv) + Ww
                    inv = dt(1) / det
                    t = (_fma(Uu, zs[0], _fma(Vv, zs[1], Ww * zs[2], dt), dt) * sz) * inv
                    mn, mx = np.minimum(np.minimum(Uu, Vv), Ww), np.maximum(np.maximum(Uu, Vv), Ww)
                    ok = ~((mn < 0) & (mx > 0)) & (t >= 0) & (t < np.inf)
                    tt = np.where(ok, t, np.inf)
                    j = tt.argmin(1)                                             # the first minimum: lexicographic (t, id)
                    hit = ok[np.arange(len(r)), j]
                    rr, jj = r[hit], j[hit]
                    ar = np.arange(len(r))[hit]
                    idx[rr], t_out[rr] = jj, t[ar, jj]
                    uv[rr, 0], uv[rr, 1] = (Vv * inv)[ar, jj], (Ww * inv)[ar, jj]
        hit = idx >= 0
        k = idx[hit]
        with np.errstate(all="ignore"):
            b1, b2 = uv[hit, 0:1], uv[hit, 1:2]
            b0 = (dt(1) - b1) - b2
            p0, p1, p2 = P[k, 0], P[k, 1], P[k, 2]
            p[hit] = _fma(p0, b0, _fma(p1, b1, p2 * b2, dt), dt)
            a, b = p1 - p0, p2 - p0
            c = np.stack([_fma(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1]), dt), _fma(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2]), dt),
                          _fma(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]), dt)], -1)
            ln = np.sqrt(_fma(c[:, 2], c[:, 2], _fma(c[:, 1], c[:, 1], c[:, 0] * c[:, 0], dt), dt))
            c = c / ln[:, None]                                                  # si.n = normalize(cross)
            ln = np.maximum(np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]), dt(1e-12))
            c = c / ln[:, None]                                                  # the call site normalises once more
            md = -d_[hit]
            flip = ((c[:, 0] * md[:, 0] + c[:, 1] * md[:, 1]) + c[:, 2] * md[:, 2]) < 0
            n[hit] = np.where(flip[:, None], -c, c)
    return dict(idx=idx, valid=idx >= 0, t=t_out, uv=uv, p=p, n=n)


# ------------------------------------------------------------------------------------------------------------------ the checks
QUANT = ("t", "b", "p", "plane", "n")


def residuals(g, o, d, res):
    """residuals of the reported hits against the exact geometry of the reported triangle, each in its unit: dict of (n_hit,) arrays + `vacuous`,
    `rows` (the indices of the hit rows).  `t` is absent where the caller has none (the HIP entry point returns no t)."""
    rows = np.nonzero(res["idx"] >= 0)[0]
    k = res["idx"][rows]
    oo, dd = o[rows], d[rows]
    ts, bs = exact_one(g, oo, dd, k)
    un = units(g, oo, dd, k)
    with np.errstate(all="ignore"):
        vac = ~(un["t"] <= VACUOUS * un["R"])
        out = dict(rows=rows, vacuous=vac, units=un, tstar=ts)
        if res.get("t") is not None:
            out["t"] = np.abs(res["t"][rows].astype(F64) - ts) / un["t"]
        uvr = np.abs(res["uv"][rows].astype(F64) - bs[1:].T).max(-1)
        out["b"] = np.maximum(uvr, np.maximum(0.0, -bs.min(0))) / un["b"]
        pstar = (bs.T[:, :, None] * g.Pabs[k]).sum(1)
        p64 = res["p"][rows].astype(F64)
        out["p"] = np.abs(p64 - pstar).max(-1) / un["p"]
        Nh = g.N[k] / g.Nlen[k][:, None]
        out["plane"] = np.abs(((p64 - g.Pabs[k, 0]) * Nh).sum(-1)) / un["plane"]
        n64 = res["n"][rows].astype(F64)
        out["n"] = np.minimum(np.abs(n64 - Nh).max(-1), np.abs(n64 + Nh).max(-1)) / un["n"]
        out["n_dot_d"] = (n64 * dd.astype(F64)).sum(-1)
    return out


def measure_E(g, o, d, res):
    """the largest residual of each quantity, vacuous rows left out of t and b"""
    r = residuals(g, o, d, res)
    E = {}
    for q in QUANT:
        v = r[q][~r["vacuous"]] if q in ("t", "b") else r[q]
        E[q] = float(np.nanmax(v)) if len(v) else 0.0
        assert not np.isnan(v).any(), q
    return E


def constants(Es):
    """C = 4 E over a list of per-input E dicts; an E above 16 means the unit is wrong for some input"""
    E = {q: max(e[q] for e in Es) for q in QUANT}
    for q in QUANT:
        assert 0 < E[q] <= 16, (q, E[q], "the unit does not fit some input")
    return {q: 4.0 * E[q] for q in QUANT}, E


def completeness_table(verts, faces, o, d, C, geom=None, chunk=1024):
    """what completeness needs of every ray, independent of the result: lim = min over the robustly crossed j of t*_j + C_t unit_t(j) (inf: none),
    and whether the exact closest crossing is robust"""
    g = geom or Geometry(verts, faces)
    B, T = len(o), len(g.faces)
    lim, nonrobust, crossed = np.full(B, np.inf), np.zeros(B, bool), np.zeros(B, bool)
    if T == 0:
        return dict(lim=lim, nonrobust=nonrobust, crossed=crossed)
    for s in range(0, B, chunk):
        oo, dd = o[s:s + chunk], d[s:s + chunk]
        t, b, _ = exact_hits(verts, faces, oo, dd, g)
        o64, d64 = oo.astype(F64), dd.astype(F64)
        R = np.zeros(t.shape)
        for i in range(3):
            for a in range(3):
                np.maximum(R, np.abs(g.Pabs[None, :, i, a] - o64[:, None, a]), out=R)
        with np.errstate(all="ignore"):
            h = np.abs(d64 @ g.N.T) / g.L[None, :]
            ub, ut = U * R / h, U * R * g.L[None, :] / h
            bmin = b.min(0)
            robust = (bmin >= C["b"] * ub) & (t >= C["t"] * ut)                  # nan / inf units compare false
            lim[s:s + chunk] = np.where(robust, t + C["t"] * ut, np.inf).min(1)
            ex = (bmin >= 0) & (t >= 0) & np.isfinite(t)
            te = np.where(ex, t, np.inf)
            j = te.argmin(1)
            ar = np.arange(len(oo))
            crossed[s:s + chunk] = ex[ar, j]
            nonrobust[s:s + chunk] = ex[ar, j] & ~robust[ar, j]
    return dict(lim=lim, nonrobust=nonrobust, crossed=crossed)


def check_hits(verts, faces, o, d, res, C, geom=None, table=None, complete=True, name=""):
    """Soundness of every reported hit, completeness of every ray, the tie rule.  res: dict(idx, valid, uv, p, n, t or None).  Without a t (the HIP
    entry point) the t of the reported triangle's plane, t*_k, stands in for it in the completeness bound, and p and uv carry the soundness of t.
    Returns the worst residual / bound of each quantity and the shares of vacuous rows (of the hits) and of non-robust rays (of the rays)."""
    g = geom or Geometry(verts, faces)
    idx, valid = np.asarray(res["idx"]), np.asarray(res["valid"]).astype(bool)
    B = len(o)
    assert idx.shape == (B,) and ((idx >= 0) == valid).all() and (idx >= -1).all() and (idx < len(g.faces)).all(), name
    miss = ~valid
    if res.get("t") is not None:
        assert np.isposinf(res["t"][miss]).all() and np.isfinite(res["t"][valid]).all() and (res["t"][valid] >= 0).all(), name
    r = residuals(g, o, d, res)
    rows, vac = r["rows"], r["vacuous"]
    worst = {}
    for q in QUANT:
        if q not in r:
            continue
        v = r[q][~vac] if q in ("t", "b") else r[q]
        worst[q] = float(v.max()) / C[q] if len(v) else 0.0
        bad = np.nonzero(~(v <= C[q]))[0]
        assert len(bad) == 0, f"{name}: {q} of {len(bad)} of {len(v)} hits beyond C = {C[q]:.3g} units, worst {np.nanmax(v):.4g} (first row {rows[~vac][bad[0]] if q in ('t', 'b') else rows[bad[0]]})"
    assert (r["n_dot_d"] <= 0).all(), f"{name}: {(r['n_dot_d'] > 0).sum()} normals not face-forwarded"
    nn = np.linalg.norm(res["n"][rows].astype(F64), axis=-1)
    assert (np.abs(nn - 1) <= 4 * U).all(), name                                 # a float32 quotient by a float32 length: 1.5 u of the length, 0.5 u each component
    k = idx[rows]
    assert (g.first_dup[k] == k).all(), f"{name}: {(g.first_dup[k] != k).sum()} hits report a duplicate that is not the smallest index"
    out = dict(worst=worst, vacuous=float(vac.mean()) if len(vac) else 0.0, n_hit=len(rows))
    if complete:
        tb = table or completeness_table(verts, faces, o, d, C, g)
        trep = np.full(B, np.inf)
        trep[rows] = res["t"][rows].astype(F64) if res.get("t") is not None else r["tstar"]
        slack = np.zeros(B)
        slack[rows] = C["t"] * np.where(np.isfinite(r["units"]["t"]), r["units"]["t"], np.inf)
        bad = np.nonzero(~(trep <= tb["lim"] + slack))[0]
        assert len(bad) == 0, f"{name}: {len(bad)} rays report a hit behind a robustly crossed triangle, or miss one (first row {bad[0]}, t {trep[bad[0]]}, limit {tb['lim'][bad[0]]})"
        out["nonrobust"] = float(tb["nonrobust"].mean())
        out["crossed"] = float(tb["crossed"].mean())
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
def _soup(kind, n=1500, m=6000, seed=0):
    """the recipes of tests/test_bvh_fuzz.py::soups at a fixed size, the degenerate f[0] = [0, 0, 1] included.  Random rays meet a needle of width 1e-4 a few
    times in 6 000, too few rows to say anything, and edge-on or thinner than L / 2^14 the bounds are vacuous: half of the needles' rays are aimed at the
    inside of the needles that are no thinner than L / 2^12, from within some 30 degrees of their normals"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, size=(n, 1, 3))
    t = c + rng.normal(scale=0.02 if kind == "long" else 0.3, size=(n, 3, 3))
    if kind == "long":
        k = n // 50
        t[:k] = rng.uniform(-1.2, 1.2, size=(k, 3, 3))
        t[1, :, 2] = -0.5
    if kind == "needles":
        t[:, 2] = t[:, 1] + 1e-4 * rng.normal(size=(n, 3))
    if kind == "duplicates":
        t[n // 2:] = t[: n - n // 2]
    v = t.reshape(-1, 3).astype(F32)
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    f[0] = [0, 0, 1]
    o = rng.uniform(-1.5, 1.5, size=(m, 3)).astype(F32)
    dd = rng.normal(size=(m, 3))
    if kind == "needles":
        e = t[:, [1, 2, 2]] - t[:, [0, 0, 1]]
        nrm = np.cross(e[:, 0], e[:, 1])
        fat = np.nonzero(((e ** 2).sum(-1).max(-1) <= 4096 * np.linalg.norm(nrm, axis=-1)) & (np.arange(n) > 0))[0]      # L / width <= 2^12
        j = fat[rng.integers(0, len(fat), m // 2)]
        tg = (rng.dirichlet([3.0, 3.0, 3.0], m // 2)[:, :, None] * t[j]).sum(1)
        nj = nrm[j] / np.linalg.norm(nrm[j], axis=-1, keepdims=True)
        o[: m // 2] = (tg + rng.choice([-1.0, 1.0], (m // 2, 1)) * rng.uniform(0.3, 1.0, (m // 2, 1)) * (nj + 0.2 * rng.normal(size=(m // 2, 3)))).astype(F32)
        dd[: m // 2] = tg - o[: m // 2]
    dd = (dd / np.linalg.norm(dd, axis=-1, keepdims=True)).astype(F32)
    return v, f, np.ascontiguousarray(o), np.ascontiguousarray(dd)


def _grazing_grid(n=24, m=6000, seed=21):
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(s, s, indexing="ij")
    Z = 0.02 * np.sin(9.0 * X) * np.cos(7.0 * Y) + 0.002 * rng.standard_normal(X.shape)
    v = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(F32)
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    a, b, c, e = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, e], -1).reshape(-1, 3)]).astype(np.int32)
    o = np.stack([rng.uniform(-1.0, 2.0, m), rng.uniform(-1.0, 2.0, m), 0.03 + np.exp(rng.uniform(np.log(0.01), np.log(0.2), m))], -1).astype(F32)
    tg = np.stack([rng.uniform(0.05, 0.95, m), rng.uniform(0.05, 0.95, m), np.zeros(m)], -1)
    dd = tg - o
    dd = (dd / np.linalg.norm(dd, axis=-1, keepdims=True)).astype(F32)
    return v, f, np.ascontiguousarray(o), np.ascontiguousarray(dd)


def _closed(offset=0.0, outside=False):
    import test_watertight as W
    v, f = W._icosphere(subdiv=3)
    if outside:
        rng = np.random.default_rng(17)
        centre, ext = np.array([0.3, -0.2, 0.9]), float((v.max(0) - v.min(0)).max())
        u = rng.standard_normal((4000, 3)); u /= np.linalg.norm(u, axis=-1, keepdims=True)
        o = (centre + 4.0 * ext * u).astype(F32)
        w = rng.dirichlet([1.0, 1.0, 1.0], 4000)
        tg = (w[:, :, None] * v[f[rng.integers(0, len(f), 4000)]].astype(F64)).sum(1)
        d = tg - o
        d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)
    else:
        o, d = W._interior_rays(20000)
    if offset:
        v, o = (v + F32(offset)).astype(F32), (o + F32(offset)).astype(F32)     # re-rounded: the reference sees the rounded values
    return np.ascontiguousarray(v), f, np.ascontiguousarray(o), np.ascontiguousarray(d)


def _cracks():
    import test_watertight as W
    v, f, n = W._patch(n=16)
    o, d = W._rays(W._targets(v, f, n))
    return v, f, o, d


def _single():
    v = np.array([[0, 0, 1], [1, 0, 1.25], [0, 1, 1.5]], F32)
    return v, np.array([[0, 1, 2]], np.int32), np.array([[0.25, 0.25, 0.0]], F32), np.array([[0.0, 0.0, 1.0]], F32)


def _empty():
    return np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), np.array([[0.25, 0.25, 0.0]], F32), np.array([[0.0, 0.0, 1.0]], F32)


INPUTS = {
    "closed": lambda: _closed(), "closed+64": lambda: _closed(64.0), "closed+1024": lambda: _closed(1024.0), "closed-from-outside": lambda: _closed(outside=True),
    "soup-random": lambda: _soup("random", seed=1), "soup-needles": lambda: _soup("needles", seed=2), "soup-duplicates": lambda: _soup("duplicates", seed=3),
    "soup-long": lambda: _soup("long", seed=4), "grazing-grid": _grazing_grid, "cracks": _cracks, "single": _single, "empty": _empty,
}
# completeness and its cap are not asked of the set aimed at edges and vertices: nearly every one of its rays is non-robust by construction
NO_COMPLETENESS = ("cracks",)
NEVER_MISSES = ("closed", "closed+64", "closed+1024", "closed-from-outside", "cracks", "single")
SYMMETRY_INPUTS = ("closed", "soup-random", "soup-long")
CAP_VACUOUS, CAP_NONROBUST = 0.005, 0.01


@functools.lru_cache(maxsize=None)
def scene(name):
    v, f, o, d = INPUTS[name]()
    for a in (v, f, o, d):
        a.setflags(write=False)
    return v, f, o, d, Geometry(v, f)


@functools.lru_cache(maxsize=None)
def restated32(name):
    v, f, o, d, _ = scene(name)
    return restated_hit(v, f, o, d, F32)


@functools.lru_cache(maxsize=None)
def measured():
    """(C, E): the constants of every bound, from the float32 restatement against the exact geometry over all inputs"""
    return constants([measure_E(scene(nm)[4], scene(nm)[2], scene(nm)[3], restated32(nm)) for nm in INPUTS if nm != "empty"])


@functools.lru_cache(maxsize=None)
def table(name):
    v, f, o, d, g = scene(name)
    return completeness_table(v, f, o, d, measured()[0], g)


def check_input(name, res):
    """every check of this module on one input; the caps included"""
    v, f, o, d, g = scene(name)
    C = measured()[0]
    complete = name not in NO_COMPLETENESS
    out = check_hits(v, f, o, d, res, C, g, table(name) if complete else None, complete, name)
    assert out["vacuous"] <= CAP_VACUOUS, (name, out)
    if complete:
        assert out["nonrobust"] <= CAP_NONROBUST, (name, out)
    if name in NEVER_MISSES:
        assert np.asarray(res["valid"]).all(), f"{name}: {(~np.asarray(res['valid'])).sum()} rays miss a closed surface"
    return out


# ------------------------------------------------------------------------------------------------------------------ exact signs of the edge functions
def exact_sign_cases(kz, n=96, seed=31):
    """One triangle and one axis-parallel ray per case, in one scene (the cases 16 apart: a ray meets only its own triangle).  The ray's origin lies
    within 2^-26 of the line through B and C: the float32 products of the edge function U = Cx By - Cy Bx round to the same value although the exact
    U is +-2^-26, while V and W are far from 0.  The contract evaluates U, V, W again in double when one of them is 0, so the decision is that of
    the exact signs: a hit where U has the sign of V and W, a miss where it has not.  All coordinates are multiples of 2^-13 below 2^9 and the
    ray is parallel to an axis, so the sheared vertices P - o are exact and the expected decision below is integer arithmetic.
    Returns verts, faces, o, d, expected valid."""
    import math
    rng = np.random.default_rng(seed + kz)
    kx = (kz + 1) % 3; ky = (kx + 1) % 3
    V, O, D, want = [], [], [], []
    while len(want) < n:
        m1, m2 = (int(x) for x in rng.integers(2 ** 11, 2 ** 13, 2))
        if math.gcd(m1, m2) != 1:
            continue
        sgn, k = int(rng.choice([-1, 1])), int(rng.integers(2, 4))
        s3 = (sgn * pow(m2, -1, m1)) % m1                                        # s3 m2 - s4 m1 = sgn
        s4 = (s3 * m2 - sgn) // m1
        A, Bv, Cv = (-m2, m1), (m1, m2), (-k * m1 + s3, -k * m2 + s4)
        if rng.integers(0, 2):
            Bv, Cv = Cv, Bv                                                      # the other winding: every sign flips
        Uu, Vv, Ww = Cv[0] * Bv[1] - Cv[1] * Bv[0], A[0] * Cv[1] - A[1] * Cv[0], Bv[0] * A[1] - Bv[1] * A[0]
        assert abs(Uu) == 1 and min(abs(Vv), abs(Ww)) > 2 ** 22
        f = lambda m: F32(m * 2.0 ** -13)
        if f(Cv[0]) * f(Bv[1]) != f(Cv[1]) * f(Bv[0]):                           # the float32 edge function must cancel to 0
            continue
        i = len(want)
        X, Y, up = 16.0 * (i % 8 + 1), 16.0 * (i // 8 + 1), 1.0 if i % 2 else -1.0
        for q, (mx, my) in enumerate((A, Bv, Cv)):
            P = np.zeros(3)
            P[kx], P[ky], P[kz] = X + mx * 2.0 ** -13, Y + my * 2.0 ** -13, up * (3.0 + 0.25 * q)
            V.append(P)
        oo, dd = np.zeros(3), np.zeros(3)
        oo[kx], oo[ky], dd[kz] = X, Y, up
        O.append(oo); D.append(dd)
        want.append(not (min(Uu, Vv, Ww) < 0 < max(Uu, Vv, Ww)))
    v = np.asarray(V)
    assert (v.astype(F32) == v).all()
    return v.astype(F32), np.arange(3 * n, dtype=np.int32).reshape(n, 3), np.asarray(O, F32), np.asarray(D, F32), np.asarray(want)


def check_exact_signs(res, want, name=""):
    np.testing.assert_array_equal(np.asarray(res["valid"]).astype(bool), want, err_msg=name)
    np.testing.assert_array_equal(res["idx"], np.where(want, np.arange(len(want)), -1), err_msg=name)
    assert 0.25 < want.mean() < 0.75


def boundary_cases(kz):
    """One triangle, whose vertices are the extremes of the scene's box, and axis-parallel rays through its vertices and edge midpoints exactly,
    from below and from above.  Every coordinate is a small multiple of 2^-6, so every step of the contract is exact: the edge functions that
    vanish are exact zeros, a zero belongs to the triangle, and uv and p are the vertex or the midpoint themselves.  A BVH whose boxes are not
    padded culls these rays: the slab of an axis in whose box face the ray lies is [-inf, 0], and the ray enters the slab of its own axis at t >= 3.
    Returns verts, faces, o, d, expected idx, uv, p."""
    kx = (kz + 1) % 3; ky = (kx + 1) % 3
    xy = np.array([[-40, -24], [56, -8], [-8, 64]], F64) / 64 + np.array([5.0, 7.0])
    bary = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]])
    tv = np.zeros((3, 3))
    tv[:, kx], tv[:, ky], tv[:, kz] = xy[:, 0], xy[:, 1], [3.0, 3.5, 4.25]
    O, D, P = [], [], []
    for start, up in ((0.0, 1.0), (8.0, -1.0)):
        for b in bary:
            pt = b @ tv
            oo, dd = pt.copy(), np.zeros(3)
            oo[kz], dd[kz] = start, up
            O.append(oo); D.append(dd); P.append(pt)
    assert (tv.astype(F32) == tv).all() and (np.asarray(P, F32) == np.asarray(P)).all()
    return (tv.astype(F32), np.arange(3, dtype=np.int32).reshape(1, 3), np.asarray(O, F32), np.asarray(D, F32), np.zeros(12, np.int64),
            np.tile(bary[:, 1:], (2, 1)).astype(F32), np.asarray(P, F32))


def check_boundary(res, idx, uv, p, name=""):
    np.testing.assert_array_equal(res["idx"], idx, err_msg=name)
    assert np.asarray(res["valid"]).all(), name
    np.testing.assert_array_equal(res["uv"], uv, err_msg=name)
    np.testing.assert_array_equal(res["p"], p, err_msg=name)


# ------------------------------------------------------------------------------------------------------------------ exact symmetries
SCALES = (-20, -7, 9, 20)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def scaled(v, o, k):
    s = F32(2.0 ** k)
    return np.ascontiguousarray(v * s), np.ascontiguousarray(o * s)            # exact: no float32 of the inputs leaves the normal range


def permuted(a):
    return np.ascontiguousarray(a[:, [1, 2, 0]])                                # (x, y, z) -> (y, z, x)


def mirrored(a):
    return np.ascontiguousarray(a * np.array([-1, 1, 1], F32))


def unique_major_axis(d):
    ad = np.sort(np.abs(d), axis=-1)
    return ad[:, 2] > ad[:, 1]


def assert_scaled(res, res_k, k, name=""):
    s = F32(2.0 ** k)
    np.testing.assert_array_equal(res_k["idx"], res["idx"], err_msg=name)
    np.testing.assert_array_equal(res_k["valid"], res["valid"], err_msg=name)
    np.testing.assert_array_equal(bits(res_k["uv"]), bits(res["uv"]), err_msg=name)
    np.testing.assert_array_equal(bits(res_k["n"]), bits(res["n"]), err_msg=name)
    np.testing.assert_array_equal(bits(res_k["p"]), bits(res["p"] * s), err_msg=name)
    if res.get("t") is not None:
        np.testing.assert_array_equal(bits(res_k["t"]), bits(res["t"] * s), err_msg=name)


def assert_isometry(res, res_x, rows, back, name=""):
    """res_x: the result on the transformed problem; back maps its p and n to the untransformed frame"""
    np.testing.assert_array_equal(res_x["idx"][rows], res["idx"][rows], err_msg=name)
    np.testing.assert_array_equal(bits(res_x["uv"])[rows], bits(res["uv"])[rows], err_msg=name)
    np.testing.assert_array_equal(back(res_x["p"])[rows], res["p"][rows], err_msg=name)        # by value: the mirror image of a miss's +0 is -0
    if res.get("t") is not None:
        np.testing.assert_array_equal(bits(res_x["t"])[rows], bits(res["t"])[rows], err_msg=name)
    dn = np.abs(back(res_x["n"]).astype(F64) - res["n"].astype(F64))[rows]
    assert dn.max(initial=0.0) <= 2 * U, (name, dn.max())
