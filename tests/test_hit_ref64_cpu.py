"""The closest hit against exact float64 geometry and against its exact symmetries (tests/hit_ref64.py), on the CPU: the oracle's BVH traversal,
the oracle's brute-force loop, and the float32 run of the numpy restatement of DESIGN.md section 2.  tests/test_hit_ref64.py holds the HIP
traversal to the same checks.

Asserted of every backend on every input: soundness of every reported hit (t, uv, min(b), p, the distance of p from the plane, the normal and
its facing, within C units of the exact geometry of the REPORTED triangle), completeness of every ray (no reported t behind a robustly crossed
triangle, no miss where one is robustly crossed), the tie rule (the smallest index of bitwise duplicates), no miss on the closed surfaces, and the
caps on the rows for which a bound says nothing (vacuous hits <= 0.5 %, non-robust rays <= 1 %).  The constants are C = 4 E with E the float32
restatement's own residuals against float64, measured when the tests run (hit_ref64.measured; values in that module's docstring).

The symmetry tests have no tolerance but the 2 u on the normal of an axis permutation or a mirror image: scaling by 2^k reproduces every bit.
Two more tests are exact decisions on exactly representable geometry: an edge function whose float32 products cancel although its exact value is
+-2^-26 takes the exact sign, and axis-parallel rays through the vertices and edge midpoints of a triangle that spans the scene's box hit it.

Mutations of the oracle, each caught by this file (none is committed), with the test that fails:
    uv returned as (W, V) / det; p with b0 and b1 exchanged; sz left out of t; the normal not face-forwarded   test_closest_hit_is_exact, every input
    t >= 0 dropped                                test_closest_hit_is_exact on the soups and, brute force, on the closed mesh
    the tie taken as id > h.id                    test_closest_hit_is_exact[soup-duplicates] (the tie rule)
    the double re-evaluation removed              test_edge_function_zero_takes_the_exact_sign (geometry cannot see it: both answers are within the bounds)
    the BVH pad set to 0                          test_vertices_and_edges_of_the_scene_box_are_hit, BVH only
    an absolute rejection |det| < 1e-12 added     test_scaling_by_a_power_of_two_is_exact
"""
import numpy as np
import pytest

import hit_ref64 as R

BACKENDS = ("bvh", "brute", "numpy-f32")


def run(oracle_mod, back, v, f, o, d):
    if back == "numpy-f32":
        return R.restated_hit(v, f, o, d, R.F32)
    sc = oracle_mod.Scene(v, f)
    p, n, uv, idx, valid = sc.ray_intersect(o, d, brute=back == "brute")
    return dict(idx=idx, valid=valid, t=sc.last_t.copy(), uv=uv, p=p, n=n)


_cache = {}


def result(oracle_mod, back, name):
    if (back, name) not in _cache:
        v, f, o, d, _ = R.scene(name)
        _cache[back, name] = R.restated32(name) if back == "numpy-f32" else run(oracle_mod, back, v, f, o, d)
    return _cache[back, name]


def test_reference_checks_itself():
    """the two float64 formulations agree; the float64 run of the restatement lands on the exact geometry (units of u = 2^-24)"""
    for name in ("closed+1024", "soup-random", "grazing-grid"):
        v, f, o, d, g = R.scene(name)
        o, d = o[:1500], d[:1500]
        t, b, N = R.exact_hits(v, f, o, d, g)
        k = np.random.default_rng(0).integers(0, len(f), len(o))
        t1, b1 = R.exact_one(g, o, d, k)
        un = R.units(g, o, d, k)
        ok = np.isfinite(t1) & (un["t"] <= R.VACUOUS * un["R"])
        ar = np.arange(len(o))
        assert ok.mean() > 0.9
        assert (np.abs(t[ar, k] - t1)[ok] <= 1e-6 * un["t"][ok]).all()
        assert (np.abs(b[:, ar, k] - b1).max(0)[ok] <= 1e-6 * un["b"][ok]).all()
        r64 = R.restated_hit(v, f, o, d, R.F64)
        E64 = R.measure_E(g, o, d, r64)
        assert max(E64.values()) <= 1e-6, E64
        r32 = R.restated_hit(v, f, o, d, R.F32)
        assert (r64["idx"] == r32["idx"]).mean() > 0.99


def test_E_and_constants():
    C, E = R.measured()
    print("E =", {q: round(e, 2) for q, e in E.items()})
    for q in R.QUANT:
        assert 0.1 <= E[q] <= 16 and C[q] == 4 * E[q]                           # above 16 the unit would be wrong for some input


def test_inputs_are_what_they_claim():
    v, f, o, d, g = R.scene("closed")
    assert len(f) == 1280 and len(o) == 20000 and (np.abs(d) == 1).any(1).sum() == 2500
    for off in (64, 1024):
        v2, _, o2, _, _ = R.scene(f"closed+{off}")
        assert np.abs(v2 - off - v).max() <= off * 2.0 ** -24 and (v2 != v + np.float32(0)).any() and o2.dtype == np.float32
    for kind in ("random", "needles", "duplicates", "long"):
        v, f, o, d, g = R.scene(f"soup-{kind}")
        assert len(f) == 1500 and len(o) == 6000 and list(f[0]) == [0, 0, 1]
    g = R.scene("soup-duplicates")[4]
    assert (g.first_dup != np.arange(1500)).sum() == 750 - 1                     # every triangle of the second half but the copy of the degenerate one
    v, f, o, d, g = R.scene("grazing-grid")
    hit = R.restated32("grazing-grid")
    k = hit["idx"][hit["valid"]]
    cos = np.abs((g.N[k] / g.Nlen[k][:, None] * d[hit["valid"]]).sum(-1))
    assert len(f) == 1152 and cos.min() < 5e-3 and np.median(cos) < 0.2


@pytest.mark.parametrize("name", list(R.INPUTS))
@pytest.mark.parametrize("back", BACKENDS)
def test_closest_hit_is_exact(oracle_mod, back, name):
    out = R.check_input(name, result(oracle_mod, back, name))
    print(name, back, out)
    if name not in ("empty", "single", "soup-needles"):
        assert out["n_hit"] >= 1500
    if name == "soup-needles":
        assert out["n_hit"] >= 500


@pytest.mark.parametrize("kz", (0, 1, 2))
@pytest.mark.parametrize("back", BACKENDS)
def test_edge_function_zero_takes_the_exact_sign(oracle_mod, back, kz):
    v, f, o, d, want = R.exact_sign_cases(kz)
    R.check_exact_signs(run(oracle_mod, back, v, f, o, d), want, f"kz = {kz}")


@pytest.mark.parametrize("kz", (0, 1, 2))
@pytest.mark.parametrize("back", BACKENDS)
def test_vertices_and_edges_of_the_scene_box_are_hit(oracle_mod, back, kz):
    v, f, o, d, idx, uv, p = R.boundary_cases(kz)
    R.check_boundary(run(oracle_mod, back, v, f, o, d), idx, uv, p, f"kz = {kz}")


@pytest.mark.parametrize("name", R.SYMMETRY_INPUTS)
@pytest.mark.parametrize("back", BACKENDS)
def test_scaling_by_a_power_of_two_is_exact(oracle_mod, back, name):
    v, f, o, d, _ = R.scene(name)
    res = result(oracle_mod, back, name)
    for k in R.SCALES:
        vk, ok = R.scaled(v, o, k)
        R.assert_scaled(res, run(oracle_mod, back, vk, f, ok, d), k, f"{name} 2^{k}")


@pytest.mark.parametrize("name", R.SYMMETRY_INPUTS)
@pytest.mark.parametrize("back", BACKENDS)
def test_axis_permutation_and_mirror_image(oracle_mod, back, name):
    v, f, o, d, _ = R.scene(name)
    res = result(oracle_mod, back, name)
    rows = R.unique_major_axis(d)
    assert rows.mean() > 0.85
    rp = run(oracle_mod, back, R.permuted(v), f, R.permuted(o), R.permuted(d))
    R.assert_isometry(res, rp, rows, lambda a: a[:, [2, 0, 1]], f"{name} permuted")
    rm = run(oracle_mod, back, R.mirrored(v), f, R.mirrored(o), R.mirrored(d))
    R.assert_isometry(res, rm, np.ones(len(o), bool), R.mirrored, f"{name} mirrored")
