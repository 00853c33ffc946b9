"""The voxel radiance cache's index on the CPU: the oracle's VoxelSLF / SLFEmitter in both modes and the restatement of tests/voxel_ref.py against the
literal float32 expression with the cast written out, on the grids and row tables that tests/test_voxel_slf.py runs on the GPU.  This file vouches for the
tables: they hold the planted rows (every grid plane with its float neighbours, the box's ends, zeros, a subnormal, 1e30, the infinities, NaN, and on the
(2, 0, 1) grid the values around 2^31 and 2^63), float64 agrees with the float32 index except within 4 ulp of a plane, and on the uniformly drawn rows
the two disagree on well under the 1 % cap.

Measured on the machine this was written on: share of the 2^15 random rows on which floor in float64 differs from the float32 index: 0 on every grid but
H64[1000.3,1004.7] (0.00055, where the box is 4.4 wide at 1000 and a float spans 1 / 1100 of a cell); planted plane rows that differ: 90, 54, 37 and 687 for
H = 31, 32, 64 and 256.  scatter_add of the restatement, worst |err| / tol: 0.55, 0.56, 0.54 and 0.44 there, 0.000 on the one- and two-cell grids.

Found by these tests and fixed with them: for a coordinate f in [9.2e18, 2^63) the kernel's voxel_coord and the oracle gave cell 0 where the reference's
int64 cast is still valid and clamps to H - 1; both compare against 2^63 now.

The mutations of voxel_ref.MUTATIONS are each refused by check_lookup (test_mutation_is_caught).
"""
import numpy as np
import pytest

import voxel_ref as V

GRID_IDS = [V.grid_id(g) for g in range(len(V.GRIDS))]


@pytest.fixture(params=["libm", "device-arithmetic", "numpy-f32"])
def back(request, oracle_mod):
    if request.param == "numpy-f32":
        return V.Numpy32()
    return V.Oracle(oracle_mod, ("libm", "device-arithmetic").index(request.param))


def test_cast_rule():
    f = np.array([0.0, -0.0, 0.99, -0.99, 1.5, -1.5, 2.0 ** 31, 3e9, 9.21e18, np.nextafter(np.float32(2.0 ** 63), np.float32(0)), 2.0 ** 63, 1e19, -2.0 ** 63, -1e19,
                  np.inf, -np.inf, np.nan, 1e-45], np.float32)
    m = V.INT64_MIN
    want = [0, 0, 0, 0, 1, -1, 2 ** 31, 3_000_000_000, int(np.float32(9.21e18)), 2 ** 63 - 2 ** 39, m, m, m, m, m, m, m, 0]
    assert V.cast_int64(f).tolist() == want
    import torch                                                                                  # ... and it is torch's .long() where torch defines one
    ok = np.isfinite(f) & (np.abs(f) < 2.0 ** 63)
    assert torch.from_numpy(f[ok]).long().tolist() == [w for w, k in zip(want, ok) if k]
    x = np.array([[4.605e18, 0.5, 0.5]], np.float32)                                              # the issue's row: f = 9.21e18 clamps to H - 1 = 1
    assert V.voxel_coords(x, 0.0, 1.0, 2).tolist() == [[1, 1, 1]]
    assert ((torch.from_numpy(x) - 0.0) / (1.0 - 0.0) * 2).long().clamp(0, 1).tolist() == [[1, 1, 1]]


@pytest.mark.parametrize("gi", range(len(V.GRIDS)), ids=GRID_IDS)
def test_tables_hold_the_planted_rows(gi):
    H, lo, hi = V.GRIDS[gi]
    x, rand = V.main_table(gi)
    assert rand.sum() == V.B and len(x) == V.B + 3 * len(V.edge_values(gi))
    edge = np.nonzero(~rand)[0]
    assert edge.min() < len(x) // 50 and edge.max() > len(x) - len(x) // 50                      # the edge rows are at shuffled positions
    for a in range(3):
        col = x[~rand][:, a]
        for p in V.planes(gi):
            assert np.isin(V.near(p, 2), col).all()
        for v in (lo, hi, 1e30, -1e30, np.inf, -np.inf, 2.0 ** -140):
            assert (col == np.float32(v)).any(), v
        assert np.isnan(col).any() and ((col == 0) & np.signbit(col)).any() and ((col == 0) & ~np.signbit(col)).any()
        if gi == V.HUGE_GRID:
            f = col.astype(np.float64) * 2
            for a_, b_ in ((2.0 ** 31 - 256, 2.0 ** 31), (2.0 ** 31, 2.0 ** 31 + 512), (3e9, 3e9 + 1), (9.2e18, 2.0 ** 63), (2.0 ** 63, 2.0 ** 63 + 2.0 ** 39), (2.0 ** 63 + 2.0 ** 39, np.inf)):
                assert ((f >= a_) & (f < b_) & np.isfinite(f)).any(), (a_, b_)
    t = V.grid_tables(gi)
    occ = t["mask"].mean()
    assert (H != 256 or 0.015 < occ < 0.025) and (t["inds"] >= -1).all() and t["inds"].max() == len(t["radiance"]) - 1
    for n in V.LENGTHS:
        xn, rn = V.table(gi, n)
        assert len(xn) == n and (n < 60 or (~rn).sum() >= 30)
    assert V.LENGTHS[-1] == 2_097_152 + 3


@pytest.mark.parametrize("gi", range(len(V.GRIDS)), ids=GRID_IDS)
def test_float64_agrees_away_from_the_planes(gi):
    x, rand = V.main_table(gi)
    share = V.check_float64_agreement(gi, x, rand)
    H, lo, hi = V.GRIDS[gi]
    c32 = V.voxel_coords(x, lo, hi, H)
    with np.errstate(all="ignore"):
        c64 = np.clip(np.floor((x.astype(np.float64) - float(np.float32(lo))) / float(np.float32(hi - lo)) * H), 0, H - 1)
    planted = int(((c32 != c64) & np.isfinite(x) & (np.abs(x) < 1e8))[~rand].any(-1).sum())
    print(f"float64 vs float32 index[{V.grid_id(gi)}]: {share:.5f} of the random rows differ; {planted} planted rows differ")
    if H > 2:
        assert planted > 0                                                                        # the planes are where the two disagree


def test_golden_box_planes_disagree_with_float64():
    """the issue's count: on the 33 planes of the golden box (-0.37, 4.21), H = 32, float32 and float64 disagree on 15"""
    H, lo, hi = V.GRIDS[3]
    p = V.planes(3)
    x = np.stack([p, p, p], -1)
    c64 = np.clip(np.floor((p.astype(np.float64) - lo) / (hi - lo) * H), 0, H - 1)                # the expression in float64 throughout, on the float32 planes
    n = int((V.voxel_coords(x, lo, hi, H)[:, 0] != c64).sum())
    print(f"golden box: float32 and float64 disagree on {n} of its {len(p)} planes")
    assert n == 15


@pytest.mark.parametrize("gi", range(len(V.GRIDS)), ids=GRID_IDS)
def test_lookup(back, gi):
    V.check_lookup(back, gi, V.main_table(gi)[0])


@pytest.mark.parametrize("n", V.LENGTHS)
@pytest.mark.parametrize("gi", [V.HUGE_GRID, 3], ids=[GRID_IDS[V.HUGE_GRID], GRID_IDS[3]])
def test_lookup_lengths(back, gi, n):
    V.check_lookup(back, gi, V.table(gi, n)[0])


@pytest.mark.parametrize("gi", range(len(V.GRIDS)), ids=GRID_IDS)
def test_eval_emitter(back, gi):
    V.check_eval_emitter(back, gi)


@pytest.mark.parametrize("gi", range(len(V.GRIDS)), ids=GRID_IDS)
def test_pooling_of_the_restatement(gi):
    b = V.Numpy32()
    V.check_scatter_add(b, gi)
    V.check_histogram(b, gi)


# ((x - vmin) * H / den is the same float32 number where H is a power of two: the 31-grid is the one that tells it apart, on 45 rows at its planes)
MUTATION_GRIDS = {"h_before_den": 2, "round": 2, "swap_x_z": 5, "threshold_9.2e18": V.HUGE_GRID}


@pytest.mark.parametrize("mut", V.MUTATIONS)
def test_mutation_is_caught(mut):
    gi = MUTATION_GRIDS[mut]
    with pytest.raises(AssertionError):
        V.check_lookup(V.Numpy32(mut), gi, V.main_table(gi)[0], log=lambda s: None)
    if mut != "threshold_9.2e18":
        with pytest.raises(AssertionError):
            V.check_histogram(V.Numpy32(mut), gi, log=lambda s: None)
