"""Helper (not a test): the camera rays of real_ldr.get_direction / to_world (reference utils/dataset/real_ldr.py:49-83) and of
synthetic_ldr.get_ray_directions / get_rays (synthetic_ldr.py:21-57) restated from their formulas in numpy, in a chosen dtype, with the case table and
the checks that tests/test_raygen_ref64_cpu.py (the oracle in both modes and the float32 run of this restatement) and tests/test_raygen_ref64.py (the HIP
kernel through the public calls) share.  No torch, nothing taken from oracle/iris_oracle.c.

The reference, for pixel (x, y) of an H x W view, all in the dtype T on the float32 K / focal / c2w (R = c2w[:, :3]):
    real       dc = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1)          (linspace(0.5, W - 0.5, W) is x + 0.5 exactly)      real_ldr.py:54-60
    synthetic  dc = (-(x + 0.5 - W / 2) / focal, -(y + 0.5 - H / 2) / focal, 1)                                                synthetic_ldr.py:28-32
    d = dc @ R.T = dc0 R[:, 0] + dc1 R[:, 1] + R[:, 2];   o = c2w[:, 3]                                                        real_ldr.py:76-77, synthetic_ldr.py:43-45
    ray_diff:  d as it is, dxdu = (1 / fx) R[:, 0], dydv = (1 / fy) R[:, 1]   (fx = fy = focal for a synthetic view)            real_ldr.py:79-81, synthetic_ldr.py:50-51
    else:      d / max(|d|, 1e-12) (real: NF.normalize), d / |d| (synthetic: torch.norm)                                       real_ldr.py:83, synthetic_ldr.py:56

Tolerance (derived, not measured; u = 2^-24).  The float32 roundings on the longest path of one component of the un-normalised direction: the subtraction
x + 0.5 - cx (x + 0.5 itself is exact below 2^23), the quotient by fx, the two products dc0 R[j, 0] and dc1 R[j, 1] and the two sums -- six roundings, each
relative to a partial result no larger than S_j = |dc0 R[j, 0]| + |dc1 R[j, 1]| + |R[j, 2]|, so
    |d_j - ref_j| <= K_D u S_j,   K_D = 6
(a single term meets five of them; the sixth covers the second-order terms).  Normalised: with e_j = K_D u S_j / |d| the error each component brings, the
norm is off by at most sum_k |dhat_k| e_k relatively through its argument, by 2.5 u through its own arithmetic (three squares and two sums under the root:
(1 + u)^3, halved by the root, and the root's rounding) and the quotient adds 1 u:
    |dhat_j - ref_j| <= e_j + |ref_j| (sum_k |ref_k| e_k + K_N u),   K_N = 3.5
which is at most (6 + 6 sqrt 3 + 3.5) u < 20 u for a rotation (S_j <= |d| by Cauchy-Schwarz), the "k 2^-24 of a unit vector".
tests/test_raygen_ref64_cpu.py asserts that the oracle and the float32 run of this restatement stay inside the same bounds: that is what validates K_D, K_N.

Exact facts (bits): o = c2w[:, 3] in every row; dxdu = fl(fl(1 / fx) c2w[:, 0]) and dydv = fl(fl(1 / fy) c2w[:, 1]) in every row (the reference's matrix
product of (1 / fx, 0, 0) with R.T adds two exact zeros to that product).
"""
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24
K_D = 6
K_N = 3.5
ONE_PASS = 4096 * 256                        # launch1d(raygen_kernel, H * W, 4096, ...): 4096 blocks of 256 threads, then the grid-stride loop
LARGE = (1025, 1031)                         # 1 056 775 pixels: 8 199 of them belong to the second pass
SIZES = ((1, 1), (1, 65), (63, 1), (5, 7), (37, 53))
MUTATIONS = ("no_half", "swap_cx_cy", "c2w_transposed", "normalise_in_ray_diff", "fx_in_dydv", "pass_two_from_pass_one")


def _rot(axis, angle):
    """Rodrigues' rotation, float64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def _c2w(Rm, t):
    return np.concatenate([Rm, np.asarray(t, np.float64).reshape(3, 1)], 1).astype(F32)


@functools.lru_cache(maxsize=None)
def cameras():
    """name -> {'kind', 'K' | 'focal', 'c2w'} (float32).  Non-square pixels, a principal point well outside the image, a rotation with zero entries and
    a generic one, a translation of magnitude 1e3."""
    generic = _rot((0.3, -0.8, 0.52), 1.1)
    axis = _rot((0, 1, 0), 0.7)                                       # zero entries: R[0, 1] = R[1, 0] = R[1, 2] = R[2, 1] = 0
    K = lambda fx, fy, cx, cy: np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F32)
    cams = {
        "real-generic": dict(kind="real", K=K(31.7, 29.3, 26.4, 18.6), c2w=_c2w(generic, (0.3, -1.2, 2.5))),
        "real-zero-entries-far": dict(kind="real", K=K(811.3, 640.9, 515.7, 512.2), c2w=_c2w(axis, (1000.0, -1000.0, 1e3))),
        "real-centre-outside": dict(kind="real", K=K(12.5, 47.75, -503.3, 1207.1), c2w=_c2w(generic.T, (-3.0, 0.25, 7.0))),
        "synthetic-generic": dict(kind="synthetic", focal=41.37, c2w=_c2w(generic, (0.5, 0.1, -2.0))),
        "synthetic-zero-entries": dict(kind="synthetic", focal=3.25, c2w=_c2w(axis, (1e3, 2.0, -1e3))),
    }
    for c in cams.values():
        c["c2w"].setflags(write=False)
        if "K" in c:
            c["K"].setflags(write=False)
    return cams


def cases():
    """(camera name, H, W, ray_diff): every camera at every small size (odd and even H and W, 1 x N, N x 1), both modes; the size just past one pass with
    the far real camera, both modes"""
    out = [(n, H, W, rd) for n in cameras() for (H, W) in SIZES + ((6, 8),) for rd in (False, True)]
    return out + [("real-zero-entries-far",) + LARGE + (rd,) for rd in (False, True)]


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-{'diff' if c[3] else 'unit'}"


def restate(cam, H, W, ray_diff, T=np.float64, mut=None):
    """-> (o, d, dxdu, dydv, tol_d) in T ((H W, 3) each; tol_d in float64), the formulas of the module docstring.  mut: one of MUTATIONS (the CPU twin's
    proof that the checks below see each of them)."""
    R = np.array(cam["c2w"][:, :3]).astype(T)
    if mut == "c2w_transposed":
        R = R.T.copy()
    half = T(0.0 if mut == "no_half" else 0.5)
    y, x = np.divmod(np.arange(H * W, dtype=np.int64), W)
    if mut == "pass_two_from_pass_one":
        late = np.arange(H * W) >= ONE_PASS
        y, x = np.where(late, np.divmod(np.arange(H * W) - ONE_PASS, W), (y, x))
    sx, sy = x.astype(T) + half, y.astype(T) + half
    if cam["kind"] == "real":
        Km = cam["K"].astype(T)
        fx, fy, cx, cy = Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]
        if mut == "swap_cx_cy":
            cx, cy = cy, cx
        dc0, dc1 = (sx - cx) / fx, (sy - cy) / fy
    else:
        fx = fy = T(F32(cam["focal"]))
        cx, cy = T(W / 2), T(H / 2)
        if mut == "swap_cx_cy":
            cx, cy = cy, cx
        dc0, dc1 = -(sx - cx) / fx, -(sy - cy) / fy
    t0, t1 = dc0[:, None] * R[None, :, 0], dc1[:, None] * R[None, :, 1]
    d = (t0 + t1) + R[None, :, 2]
    S = (np.abs(t0) + np.abs(t1) + np.abs(R[None, :, 2])).astype(np.float64)
    tol = K_D * U * S
    if (not ray_diff) or mut == "normalise_in_ray_diff":
        n = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))[:, None]
        if cam["kind"] == "real":
            n = np.maximum(n, T(1e-12))
        e = tol / n.astype(np.float64)
        d = d / n
        a = np.abs(d).astype(np.float64)
        tol = e + a * ((a * e).sum(-1, keepdims=True) + K_N * U)
    o = np.broadcast_to(np.array(cam["c2w"][:, 3]).astype(T), d.shape)
    ifx, ify = T(1) / fx, T(1) / (fx if mut == "fx_in_dydv" else fy)
    dxdu = np.broadcast_to(ifx * R[:, 0], d.shape)
    dydv = np.broadcast_to(ify * R[:, 1], d.shape)
    return o, d, dxdu, dydv, tol


class Numpy32:
    """the restatement run in float32 (and, with mut, one of its mutations)"""

    def __init__(self, mut=None):
        self.mut, self.name = mut, "numpy-f32" + (f"[{mut}]" if mut else "")

    def rays(self, cam, H, W, ray_diff):
        o, d, dx, dy, _ = restate(cam, H, W, ray_diff, F32, self.mut)
        return (o, d, dx, dy) if ray_diff else (o, d)


class Oracle:
    def __init__(self, oracle_mod, mode):
        self.o, self.mode, self.name = oracle_mod, mode, ("oracle-libm", "oracle-device-arithmetic")[mode]

    def rays(self, cam, H, W, ray_diff):
        prev = self.o.get_mode()
        self.o.set_mode(self.mode)
        try:
            if cam["kind"] == "real":
                return self.o.raygen_real(cam["K"], cam["c2w"], H, W, ray_diff)
            return self.o.raygen_synthetic(float(cam["focal"]), cam["c2w"], H, W, ray_diff)
        finally:
            self.o.set_mode(prev)


@functools.lru_cache(maxsize=4)
def reference(name, H, W, ray_diff):
    """the float64 run, computed once per case and shared (read-only)"""
    out = restate(cameras()[name], H, W, ray_diff)
    out = tuple(np.ascontiguousarray(a) for a in out)
    for a in out:
        a.setflags(write=False)
    return out


def exact_differentials(cam):
    """fl(fl(1 / fx) c2w[:, 0]), fl(fl(1 / fy) c2w[:, 1])"""
    fx, fy = (cam["K"][0, 0], cam["K"][1, 1]) if cam["kind"] == "real" else (F32(cam["focal"]),) * 2
    return (F32(1) / fx) * cam["c2w"][:, 0], (F32(1) / fy) * cam["c2w"][:, 1]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def check_view(back, case, log=print):
    """one case of cases() against the float64 run: d within the derived bound on every pixel, o and the differentials bit for bit.  Returns worst |err| / tol."""
    name, H, W, ray_diff = case
    cam = cameras()[name]
    _, d64, _, _, tol = reference(name, H, W, ray_diff)
    out = back.rays(cam, H, W, ray_diff)
    assert len(out) == (4 if ray_diff else 2)
    o, d = np.asarray(out[0]), np.asarray(out[1])
    assert o.shape == (H * W, 3) and d.shape == (H * W, 3) and o.dtype == F32 and d.dtype == F32
    assert (_bits(o) == _bits(cam["c2w"][:, 3])[None]).all(), f"{back.name} {case_id(case)}: rays_o is not c2w[:, 3]"
    err = np.abs(d.astype(np.float64) - d64)
    ratio = np.divide(err, tol, out=np.where(err > 0, np.inf, 0.0), where=tol > 0)           # (a component whose terms are all zero has tol = 0: it is exact)
    worst = float(ratio.max())
    log(f"raygen[{back.name}, {case_id(case)}]: worst |err| / tol {worst:.3f}")
    bad = ~(err <= tol)
    assert not bad.any(), f"{back.name} {case_id(case)}: pixels {np.nonzero(bad.any(-1))[0][:8].tolist()} outside the bound, worst |err| / tol {worst:.3g}"
    if ray_diff:
        ex, ey = exact_differentials(cam)
        for got, want, nm in ((out[2], ex, "dxdu"), (out[3], ey, "dydv")):
            got = np.asarray(got)
            assert got.shape == (H * W, 3) and (_bits(got) == _bits(want)[None]).all(), f"{back.name} {case_id(case)}: {nm} is not fl(fl(1 / f) c2w column)"
    else:
        n = np.linalg.norm(d.astype(np.float64), axis=-1)
        assert np.abs(n - 1).max() <= 4 * U, f"{back.name} {case_id(case)}: not unit length"
    return worst


def spread_ids(n_pixels, count=384, seed=3):
    """pixel ids spread over both passes of a view of n_pixels: the first and last of each pass, and random ones on either side of ONE_PASS"""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, ONE_PASS - 1, ONE_PASS, ONE_PASS + 1, n_pixels - 1]
    ids = np.concatenate([fixed, rng.integers(0, ONE_PASS, count // 2), rng.integers(ONE_PASS, n_pixels, count // 2)]).astype(np.int64)
    return ids[rng.permutation(len(ids))]
