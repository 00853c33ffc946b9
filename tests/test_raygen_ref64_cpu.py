"""Ray generation against the float64 restatement of tests/raygen_ref64.py, on the CPU: the oracle in both of its modes and the float32 run of the
restatement itself.  They vouch for the case table and for the derived bound (K_D = 6 roundings on the un-normalised direction, K_N = 3.5 on top for the
unit vector; raygen_ref64's docstring): the reference's own float32 arithmetic stays inside it on every pixel of every case, the 1 056 775 pixels of the
1025 x 1031 view included.  tests/test_raygen_ref64.py runs the same cases on the GPU.

Worst |err| / tol on the machine this was written on, over all cases: 0.36 un-normalised, 0.25 normalised, for the oracle in both modes and for the
float32 restatement alike (every operation on the path is one IEEE operation: the three agree to the bit).

The mutations of the float32 restatement listed in raygen_ref64.MUTATIONS are each refused by check_view (test_mutation_is_caught): the list stays true.
"""
import numpy as np
import pytest

import raygen_ref64 as R


@pytest.fixture(params=["libm", "device-arithmetic", "numpy-f32"])
def back(request, oracle_mod):
    if request.param == "numpy-f32":
        return R.Numpy32()
    return R.Oracle(oracle_mod, ("libm", "device-arithmetic").index(request.param))


def test_case_table_holds_what_it_should():
    cams = R.cameras()
    K = cams["real-generic"]["K"]
    assert K[0, 0] != K[1, 1]                                                                     # non-square pixels
    Kc = cams["real-centre-outside"]["K"]
    assert Kc[0, 2] < -100 and Kc[1, 2] > 1000                                                    # the principal point well outside every image here
    assert (cams["real-zero-entries-far"]["c2w"][:, :3] == 0).sum() == 4 and (cams["real-generic"]["c2w"][:, :3] == 0).sum() == 0
    assert np.abs(cams["real-zero-entries-far"]["c2w"][:, 3]).min() >= 1e3
    for c in cams.values():                                                                       # rotations: S_j <= |d|, the "< 20 u" of the docstring
        Rm = c["c2w"][:, :3].astype(np.float64)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-6
    sizes = {(H, W) for _, H, W, _ in R.cases()}
    assert {(1, 1), (1, 65), (63, 1), (5, 7), (37, 53), R.LARGE} <= sizes
    syn = {(H % 2, W % 2) for n, H, W, _ in R.cases() if cams[n]["kind"] == "synthetic"}
    assert {(0, 0), (1, 1)} <= syn                                                                # synthetic views with odd and with even H and W
    assert R.LARGE[0] * R.LARGE[1] > R.ONE_PASS and R.LARGE[0] * R.LARGE[1] == 1_056_775
    ids = R.spread_ids(R.LARGE[0] * R.LARGE[1])
    assert (ids < R.ONE_PASS).sum() >= 100 and (ids >= R.ONE_PASS).sum() >= 100


def test_restatement_matches_the_golden_rays():
    """the float32 run of the restatement gives the reference's own rays (tests/golden/raygen_real.npz, captured from the reference) within the bound"""
    from conftest import golden
    g = golden("raygen_real.npz")
    H, W = int(g["H"]), int(g["W"])
    cam = dict(kind="real", K=g["K"].astype(np.float32), c2w=g["c2w"].astype(np.float32)[:3])
    _, d64, _, _, tol = R.restate(cam, H, W, False)
    assert (np.abs(g["rays_d"].astype(np.float64) - d64) <= tol).all()


@pytest.mark.parametrize("case", R.cases(), ids=R.case_id)
def test_rays(back, case):
    R.check_view(back, case)


MUTATION_CASES = {
    "no_half": ("real-generic", 5, 7, True),
    "swap_cx_cy": ("real-generic", 37, 53, False),
    "c2w_transposed": ("real-zero-entries-far", 5, 7, True),
    "normalise_in_ray_diff": ("synthetic-generic", 5, 7, True),
    "fx_in_dydv": ("real-generic", 1, 1, True),
    "pass_two_from_pass_one": ("real-zero-entries-far",) + R.LARGE + (False,),
}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutation_is_caught(mut):
    with pytest.raises(AssertionError):
        R.check_view(R.Numpy32(mut), MUTATION_CASES[mut], log=lambda s: None)
    if mut == "pass_two_from_pass_one":                                                           # ... and only the size past one pass sees it
        R.check_view(R.Numpy32(mut), ("real-zero-entries-far", 37, 53, False), log=lambda s: None)
