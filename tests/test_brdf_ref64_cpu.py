"""The BRDF samplers and the GGX evaluation against the float64 reference of tests/brdf_ref64.py, on the CPU: the oracle in both of its modes (libm; the
HIP kernels' arithmetic, which tests/test_pt_single.py, test_hip_parity.py and test_refine.py show to be the kernels' bits) and the float32 run of the
restatement itself.  The float32 run and the libm oracle vouch for the case tables: every bound and cap below is met by the reference's own arithmetic,
and their direction errors are E, the yardstick of the direction checks here and in tests/test_brdf_ref64.py (the same tables on the GPU).

What is asserted (brdf_ref64.check_*): directions within 2 E of the float64 continuation of the float32 prefix and of unit length to 4 u; every finite
pdf / brdf / g0 / g1 / weight inside its perturbation envelope, on every row, the rows with wo below the horizon included; the share of rows whose
envelope says nothing (tol > 1e-3 |f| + 1e-6) capped per roughness level; non-finite values only where the GGX denominator is degenerate at r = 0.02;
the lobe sample_brdf takes at s1 = 0.5 and its neighbours; the emitter ordinal at every cdf entry and its neighbours; the frame's orthonormality and
branch at |n.x| = 0.1f; lerp_specular at every knot and outside [0.02, 1].

E is measured when the tests run, since numpy's float32 sin / cos are not the same on every CPU.  On the machine this was written on (max over the libm
oracle and the float32 restatement, B = 2^15 rows per table, edge rows no worse than random ones):
    sample_diffuse 2.7e-7;  sample_specular 3.1e-7, 3.8e-7, 4.2e-7, 6.0e-7, 3.6e-7, 4.0e-7, 4.6e-7, 5.5e-7, 5.7e-7 for r = 0.02 ... 1.0;
    sample_specular with one roughness per row 4.7e-7;  sample_brdf 4.6e-7;  sample_emitter 1.2e-7 ... 1.3e-7;  angle2xyz 1.2e-7.
The device-arithmetic oracle's own direction errors on the same tables are at or below the libm oracle's; the worst |err| / tol of any envelope is 0.50.
The direction checks cannot see a fraction of an ulp of the polar angle, so the specified asin / acos is also held directly to what iris_device.h states
of it (test_specified_asin_acos_is_within_one_ulp).

One row in 2^15 at r = 0.02 lies outside the envelope as the formula above gives it, in both oracle modes and in the float32 restatement alike: the box's
ends do not bound D_GGX where its pole lies inside the box.  brdf_ref64.envelope documents the row and treats such rows (den <= 20 u) as open above.

Found by these tests and fixed with them: the oracle's lerp_specular indexed outside the table for a roughness outside [0.02, 1] (the HIP kernel keeps
both indices inside); it clamps now, as the kernel does.

Mutations of the oracle's device-arithmetic code, each caught by this file in that mode (none is committed): a coefficient of spec_asin_poly changed in
its 6th digit; the k == 3 selects of spec_sincos swapped; `small != ACOS` turned into `==`; kPio2Lo dropped; `s1 > 0.5f` turned into `>=`; the
searchsorted loop using `<=`; ceilf for both lerp_specular indices.
"""
import functools

import numpy as np
import pytest
import torch

import brdf_ref64 as R


@pytest.fixture(scope="module")
def bounds(oracle_mod):
    return R.Bounds(oracle_mod)


@pytest.fixture(params=["libm", "device-arithmetic", "numpy-f32"])
def back(request, oracle_mod):
    if request.param == "numpy-f32":
        return R.Numpy32()
    return R.Oracle(oracle_mod, ("libm", "device-arithmetic").index(request.param))


def model_cdf(K):
    """emitter_pdf and emitter_cdf as the model builds them (model/emitter.py:168-170)"""
    pdf = torch.nn.functional.normalize(torch.ones(K), dim=-1, p=1)
    return pdf.cumsum(-1).numpy().copy()


@functools.lru_cache(maxsize=None)
def emitter(K, zero):
    em = R.emitter_tables(K, zero)
    em["cdf"] = model_cdf(K)
    return em


def test_reference_checks_itself():
    for r in R.ROUGH_LEVELS:
        assert abs(R.ggx_cdf(np.pi / 2, r) - 1.0) <= 1e-9, r                      # D(h) (n.h) integrates to 1
        for u0 in (0.0, 1e-3, 0.25, 0.5, 0.9, 1 - 2.0 ** -24):                    # the sampler's theta(u0) inverts the cdf
            a2 = float(r) ** 4
            den = u0 * (a2 - 1) + 1                                               # cos^2 = (1 - u0) / den, sin^2 = u0 a2 / den: no cancellation
            theta = np.arctan2(np.sqrt(u0 * a2 / den), np.sqrt((1 - u0) / den))
            assert abs(R.ggx_cdf(theta, r) - u0) <= 1e-9, (r, u0)
    assert abs(R.cosine_pdf_integral() - 1.0) <= 1e-12
    x = np.linspace(0.0, 1.0, 5)                                                  # the cosine sampler's theta(u0) inverts its cdf sin^2(theta)
    assert np.abs(np.sin(np.arcsin(np.sqrt(x))) ** 2 - x).max() <= 1e-15


def test_case_tables_hold_the_planted_edges():
    c = R.sampler_case(None, seed=12)
    u0, u1 = c["u2"][:, 0], c["u2"][:, 1]
    assert u0.min() == 0 and u0.max() == R.TOP and u1.min() == 0 and u1.max() == R.TOP
    for g in R.GRID:
        assert (u0 == R.F32(g)).sum() >= 8 and (u1 == R.F32(g)).sum() >= 8
    s = np.sqrt(u0)
    for h in R.HALF3:                                                             # the branch of the asin, x = 0.5, and both neighbours
        assert (s == h).any(), h
    for lv, r in enumerate(R.ROUGH_LEVELS):                                       # the branch of the acos: the closest u0 there are on both sides
        rows = c["level"] == lv
        sc = R.prefix_specular(c["u2"][rows], r)[0]
        assert sc.max() <= 1 and sc.min() >= 0
        planted = R.u0_for_c2_half(r)
        assert np.isin(planted, u0[rows]).all()
        sp = R.prefix_specular(np.stack([planted, planted], -1), r)[0]
        if lv > 0:
            assert sp.min() < 0.5 <= sp.max(), (r, sp)
        else:                                                                     # (r = 0.02: sqrt(c2) reaches 0.5 at the last draw there is, 1 - 2^-24, and never goes below)
            assert sp.min() == 0.5 and planted.max() == R.TOP
    phi = R.TWO_PI_F * u1
    assert (phi == 0).any()
    for k in range(1, 9):                                                         # both sides of every multiple of pi/4, within 4 ulps (u1 < 1 stops below 2 pi)
        t = R.F32(k * np.pi / 4)
        d = (phi.astype(np.float64) - float(t)) / float(np.spacing(t))
        assert ((d <= 0) & (d >= -4)).any() and (k == 8 or ((d > 0) & (d <= 4)).any()), k
    n = c["normal"]
    for x in R._near(0.1, 1):
        assert (n[:, 0] == x).sum() >= 32 and (n[:, 0] == -x).sum() >= 32
    assert ((n == (0, 0, 1)).all(-1)).mean() >= 0.25
    below = (R._dot(c["wo"].astype(np.float64), n.astype(np.float64)) < 0).mean()
    assert 0.05 <= below <= 0.2, below
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1).max() <= R.U


@pytest.mark.parametrize("acos", [False, True], ids=["asin", "acos"])
def test_specified_asin_acos_is_within_one_ulp(oracle_mod, acos):
    """iris_device.h states of spec_asin_acos, "exhaustively over the 2^24 Philox outputs u0: equal to the correctly rounded asin(sqrt u0) for 98.5 % of
    the inputs, never more than 1 ulp off".  Both halves are held here, over those 2^24 arguments, for the asin and for the acos that shares its code, against
    numpy's float64 functions rounded to float32.  (The direction checks cannot see an error of a fraction of an ulp of the angle; this can: a coefficient of
    the polynomial off in its 6th digit gives 96.1 %, the pi/2 tail dropped 54.7 %.  Measured: asin 98.45 %, acos 98.76 %, worst error 0.62 ulp.)"""
    x = np.sqrt((np.arange(1 << 24, dtype=np.float64) * 2.0 ** -24).astype(np.float32))
    x = np.concatenate([x, R._near(0.5, 4), R._near(1.0, 4)[:5], R._near(0.0, 4)[4:]])     # and the branch point, the ends and their neighbours
    got = oracle_mod.spec_asin_acos(x, acos)
    want = (np.arccos if acos else np.arcsin)(x.astype(np.float64)).astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(2.0 ** -126)))
    assert (np.abs(got.astype(np.float64) - want) <= ulp).all()
    exact = float((got == want).mean())
    print(f"spec_asin_acos[{'acos' if acos else 'asin'}]: correctly rounded on {100 * exact:.2f} %")
    assert exact >= 0.984
    for h in R.HALF3:                                                             # the branch point and its neighbours are among the arguments
        assert (x == h).any()


def test_sample_diffuse(back, bounds):
    R.check_sample_diffuse(back, bounds)


@pytest.mark.parametrize("rough", R.ROUGH_LEVELS, ids=[f"r{float(r):.3g}" for r in R.ROUGH_LEVELS])
def test_sample_specular(back, bounds, rough):
    R.check_sample_specular(back, bounds, rough)


def test_sample_specular_per_row_roughness(back, bounds):
    R.check_sample_specular_rows(back, bounds)


def test_eval_brdf(back):
    R.check_eval_brdf(back)


def test_sample_brdf(back, bounds):
    R.check_sample_brdf(back, bounds)


@pytest.mark.parametrize("K,zero", R.EMITTER_CONFIGS, ids=[f"K{k}" + ("" if z is None else "-area0") for k, z in R.EMITTER_CONFIGS])
def test_sample_emitter(back, bounds, K, zero):
    R.check_sample_emitter(back, bounds, emitter(K, zero))


def test_get_normal_space(back):
    R.check_get_normal_space(back)


@pytest.mark.parametrize("levels", [1, 2, 6])
def test_lerp_specular(back, levels):
    R.check_lerp_specular(back, levels)


def test_angle2xyz(back, bounds):
    R.check_angle2xyz(back, bounds)
