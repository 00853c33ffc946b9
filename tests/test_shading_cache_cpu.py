"""The BRDF trainer's shading combine and its gradients against the float64 closed form of tests/shade_ref64.py, on the CPU: the oracle's shade_cached
(both modes) and the float32 run of the restatement.  They vouch for the case tables and for the rounding counts behind the per-element bounds
(K_L = 10, K_A = 7, K_M = 10, K_R = 12; shade_ref64's docstring): the reference's own float32 arithmetic stays inside them on every row, at every level
knot, outside [0.02, 1], at metallic and albedo exactly 0 and 1.  tests/test_shading_cache.py runs the same tables on the GPU.

Worst |err| / tol on the machine this was written on, over R in {1, 2, 5, 6, 8} and all batches:
    oracle (both modes alike)   L 0.41   g_albedo 0.60   g_metallic 0.40   g_roughness 0.38
    float32 restatement         L 0.41   g_albedo 0.56   g_metallic 0.39   g_roughness 0.34

The mutations of shade_ref64.MUTATIONS are each refused by check_shade (test_mutation_is_caught).  `r1 = r0 + 1` is refused by one assertion alone,
g_roughness = 0 at a knot: its forward value and its other gradients are the unmutated ones.
"""
import numpy as np
import pytest

import brdf_ref64 as BR
import shade_ref64 as S


@pytest.fixture(params=["libm", "device-arithmetic", "numpy-f32"])
def back(request, oracle_mod):
    if request.param == "numpy-f32":
        return S.Numpy32()
    return S.Oracle(oracle_mod, ("libm", "device-arithmetic").index(request.param))


def test_closed_form_gradients_are_the_derivatives():
    """central differences of the float64 forward value, away from the knots (where L has a kink in the roughness)"""
    c = dict(S.case(6, 63, "permutation"))
    rough = c["rough"].reshape(-1)
    r0, r1, w = BR.lerp_plan(rough, 6)
    ref, _ = S.restate(c)
    g = c["gL"].astype(np.float64)
    h = 2.0 ** -10

    def slope(name, e):
        """(sum_c g L)(x + h e) - (...)(x - h e) over the step actually taken: the perturbed inputs are float32 numbers again"""
        hi, lo = dict(c), dict(c)
        hi[name], lo[name] = (c[name] + np.float32(h) * e).astype(np.float32), (c[name] - np.float32(h) * e).astype(np.float32)
        step = ((hi[name].astype(np.float64) - lo[name]) * e).sum(-1)
        return ((S.restate(hi)[0]["L"] - S.restate(lo)[0]["L"]) * g).sum(-1) / step

    smooth = (w > 0.01) & (w < 0.99) & (r0 != r1) & (rough > 0.03) & (rough < 0.99)
    assert smooth.sum() >= 5
    # (the weight is float32 arithmetic on the roughness: its own rounding, 2^-24 / h, is what the difference quotient is good to)
    assert np.allclose(slope("rough", np.ones((1, 1), np.float32))[smooth], ref["g_roughness"][smooth], rtol=1e-3, atol=0)
    # L is linear in the metallic and in each albedo channel, and float64 throughout: the quotient is exact up to float64
    scale = np.abs(g).sum(-1) * 1e3
    assert (np.abs(slope("metallic", np.ones((1, 1), np.float32)) - ref["g_metallic"]) <= 1e-9 * scale).all()
    for ch in range(3):
        e = np.zeros((1, 3), np.float32); e[0, ch] = 1
        assert (np.abs(slope("albedo", e) - ref["g_albedo"][:, ch]) <= 1e-9 * scale).all()


@pytest.mark.parametrize("batch", S.BATCHES, ids=S.batch_id)
@pytest.mark.parametrize("R", S.LEVELS)
def test_shade(back, R, batch):
    S.check_shade(back, R, batch)


@pytest.mark.parametrize("mut", S.MUTATIONS)
def test_mutation_is_caught(mut):
    with pytest.raises(AssertionError):
        S.check_shade(S.Numpy32(mut), 6, (1 << 15, "repeats"), log=lambda s: None)
    if mut == "r1_is_r0_plus_1":                                                  # ... by the knots alone: the same mutation with its knot rows' gradient zeroed passes
        class Masked(S.Numpy32):
            def shade(self, c):
                L, ga, gm, gr = super().shade(c)
                r0, r1, _ = BR.lerp_plan(c["rough"].reshape(-1), c["R"])
                return L, ga, gm, np.where(r0 == r1, np.float32(0), gr)
        S.check_shade(Masked(mut), 6, (1 << 15, "repeats"), log=lambda s: None)
