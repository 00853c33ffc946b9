"""The path tracer's MIS stages per path against the float64 reference of tests/pt_stage_ref64.py, on the CPU: the oracle in both of its modes (orc_pt_nee,
orc_pt_brdf_trace with orc_pt_brdf_finish, _apply, orc_pt_accumulate) and the float32 run of the restatement itself, through the check_* functions and on the
tables that tests/test_pt_stage_ref64.py runs the HIP kernels through.  The float32 run and the libm oracle vouch for the tables and measure E; this file
asserts the branch table (at least 8 decided rows on each side of every observable branch, per stage and variant) and the 2 % cap on undecided rows.

Branch table: decided rows (true, false) of the float64 reference, summed over the inputs (box room, open scene, open scene * 2^-7 and * 2^9; the finish
stage also over the synthetic table), as test_branch_table_and_caps prints them:
    emitter-sampling stage, single     emit_pdf < pdf_eps 2868 / 6745   d2 < g_eps 789 / 8401   MIS denominator < mis_eps 1126 / 6887   visibility ray hits 9190 / 423
                                       hit is the sampled triangle 7776 / 1414   another triangle hit is an emitter 594 / 820
    emitter-sampling stage, indirect   emit_pdf < pdf_eps 1257 / 8356   the three hit branches as above (d2 < 1e-12 and the MIS clamp do not exist there)
    finish stage, single               hit 7629 / 6415   hit is an emitter 2310 / 5319   roughness_next > trace_roughness 4839 / 480   cache voxel is empty 993 / 3846
                                       cache sum > 0 1925 / 2914   brdf_pdf > 0 on an emitter 2065 / 245   brdf_pdf.isinf() on an emitter 120 / 2190
    finish stage, indirect             9429 / 6775   2670 / 6759   2901 / 3858   638 / 2263   1023 / 1878   2305 / 365   180 / 2490
Undecided rows: none in the box room, 35 to 39 of 2 900 (1.3 %) in the open scenes, all of them `edge`; none in the finish stage.  The sides that cannot be
reached or cannot differ in an output are listed, with the reason, in pt_stage_ref64's docstring (UNOBSERVABLE).

The restatement is tied to the reference's own Python per path: tools/make_pt_stage_golden.py runs the reference's unmodified path_tracing_single (spp = 1) and
trace_indirect (depth 1 and 2) in float64 on the open scene, the closest hit exact, and records every stage boundary into tests/golden/pt_stage_ref.npz (data
only: 800 + 350 + 350 paths).  The float64 stage formulas of the restatement, fed those records, give every path's L to a relative 1e-12 of the path's terms
(measured: 3.6e-15, 2.2e-15, 9.3e-15) and carry exactly the reference's paths into the second bounce (test_restatement_is_the_references_*).

No finding: the oracle, the float32 restatement, the float64 restatement and the reference's float64 run agree on every decided row.

Mutations of the oracle's arithmetic (orc_pt_nee, orc_pt_brdf_finish: the code both modes share), each tried; five are caught by this file, two cannot be
by any test of the outputs (none is committed):
    the MIS clamp dropped (orc_pt_nee: `den < mis_eps` never applied)                        test_nee[single] on the open scenes: rows outside the envelope
    G selected by "hit" where the reference selects by valid_next (orc_pt_brdf_finish)        test_finish_table / test_brdf_stage: coef2 of emitter hits
    `emit_tri == h.tri` forced true (orc_pt_nee)                                              test_nee: occluded rows and rows that hit E0 in front of E1
    the cache test `> 0` turned into `>= 0`                                                   test_finish_table: valid_next of the zero, empty and (1, -1, 0) voxels
    const2 without w_mis                                                                      NOT caught, and cannot be: const2 != 0 only on a surface hit, where emit_pdf = 0
                                                                                              sets w_mis = 1 (model/emitter.py:207-219 never adds the cache to an emitter's Le)
    g_eps used for pdf_eps (orc_pt_nee)                                                       identical in both variants as the reference has them (1e-6, 1e-6 / 1e-12, 1e-12):
                                                                                              caught only through test_eps_are_separate_arguments, which passes unequal values
    `emit_pdf > 0` turned into `>=`                                                           NOT caught, and cannot be: see UNOBSERVABLE
"""
import numpy as np
import pytest

import pt_stage_ref64 as P


@pytest.fixture(scope="module")
def yard(oracle_mod):
    return P.Yardstick(oracle_mod)


@pytest.fixture(params=["libm", "device-arithmetic", "numpy-f32"])
def back(request, oracle_mod):
    if request.param == "numpy-f32":
        return P.Numpy32()
    return P.Oracle(oracle_mod, ("libm", "device-arithmetic").index(request.param))


def _cap(out, name):
    n_und = sum(out["undecided"].values())
    assert n_und <= P.CAP * out["n"], f"{name}: {n_und} of {out['n']} rows undecided {out['undecided']}"


@pytest.mark.parametrize("variant", list(P.VARIANTS))
@pytest.mark.parametrize("scene", P.SCENES)
def test_nee(back, yard, scene, variant):
    _cap(P.check_nee(back, yard, scene, variant), scene)


@pytest.mark.parametrize("variant", list(P.VARIANTS))
@pytest.mark.parametrize("scene", P.SCENES)
def test_brdf_stage(back, yard, scene, variant):
    _cap(P.check_brdf_stage(back, yard, scene, variant), scene)


@pytest.mark.parametrize("variant,trace_rough,mode", P.FINISH_TABLE_CASES, ids=[f"{v}-{t}-{m}" for v, t, m in P.FINISH_TABLE_CASES])
def test_finish_table(back, yard, variant, trace_rough, mode):
    _cap(P.check_finish_table(back, yard, variant, trace_rough, mode), "table")


@pytest.mark.parametrize("nan_to_zero,drop", P.APPLY_CASES, ids=[f"nan{n}-without-{d}" for n, d in P.APPLY_CASES])
def test_apply(back, nan_to_zero, drop):
    P.check_apply(back, nan_to_zero, drop)


def test_branch_table_and_caps(yard):
    """From the float64 reference alone (the float32 restatement only supplies the sampled directions): every observable branch has at least 8 decided rows on each
    side, per stage and variant, and at most 2 % of any input is undecided."""
    b32 = P.Numpy32()
    for variant in P.VARIANTS:
        nee, fin = {}, {}
        for name in P.SCENES:
            out = P.check_nee(b32, yard, name, variant, log=lambda s: None)
            _cap(out, name)
            P.add_counts(nee, out["branches"])
            out = P.check_brdf_stage(b32, yard, name, variant, log=lambda s: None)
            _cap(out, name)
            P.add_counts(fin, out["branches"])
        for v, tr, mode in P.FINISH_TABLE_CASES:
            if v == variant:
                P.add_counts(fin, P.check_finish_table(b32, yard, v, tr, mode, log=lambda s: None)["branches"])
        print(f"emitter-sampling stage [{variant}]: {nee}")
        print(f"finish stage [{variant}]: {fin}")
        for stage, table in (("nee", nee), ("finish", fin)):
            for br, (a, b) in table.items():
                assert min(a, b) >= P.MIN_SIDE, f"{stage}[{variant}] branch `{br}`: {a} rows true, {b} false"
    print("E (float32 restatement and libm oracle, in envelope units): " + ", ".join(f"{s} {yard.stage_E(s):.3f}" for s in ("nee", "finish")))


def test_inputs_hold_what_they_were_built_for():
    sc = P.scene("open")
    a = sc["em"]["area"]
    assert sc["em"]["K"] >= 4 and a[a > 0].min() <= 1e-10 and a.max() >= 1e7 and len(sc["faces"]) <= 64
    e = sc["em"]["emitter_pdf"] / np.maximum(a, np.float32(1e-12))
    assert (e < 1e-12).any() and (e < 1e-6).sum() >= 2 and (a == 0).any()
    cls = sc["slf"]["cls"]
    assert all((cls == k).sum() >= 64 for k in range(4)) and sc["slf"]["H"] == 8
    assert (sc["slf"]["radiance"] == np.array([1, -1, 0], np.float32)).all(-1).sum() >= 64
    tb = P.finish_table()
    assert len(tb["pdf"]) <= 4096 and np.isnan(tb["pdf"]).any() and np.isinf(tb["pdf"]).any() and (tb["pdf"] == 0).any()
    assert ((tb["pdf"] > 0) & (tb["pdf"] < 2.0 ** -126)).any() and (tb["weight"] == 0).any() and set(tb["tri_class"].tolist()) == set(range(6))
    d2 = ((tb["pos"].astype(np.float64) - tb["pos_next"]) ** 2).sum(-1)
    for k, (lo, hi) in enumerate(((0, 1e-12), (1e-12, 1e-6), (0, 1e-6), (1e-6, 1), (0.5, 2))):
        assert ((d2[tb["d2_class"] == k] > lo) & (d2[tb["d2_class"] == k] < hi)).all(), k


def test_eps_are_separate_arguments(oracle_mod):
    """g_eps and pdf_eps are equal in both of the reference's variants, so a stage that used one for the other would pass every comparison above.  With unequal
    values (g_eps = 1e-6, pdf_eps = 1e-12 and the reverse) the device-arithmetic oracle and the float32 restatement must still agree with float64."""
    yard = P.Yardstick(oracle_mod)
    P.VARIANTS["g6-p12"], P.VARIANTS["g12-p6"] = (np.float32(1e-6), np.float32(1e-12), np.float32(0)), (np.float32(1e-12), np.float32(1e-6), np.float32(0))
    try:
        for v in ("g6-p12", "g12-p6"):
            for b in (P.Oracle(oracle_mod, 1), P.Numpy32()):
                P.check_nee(b, yard, "open", v)
    finally:
        del P.VARIANTS["g6-p12"], P.VARIANTS["g12-p6"]


ACC = [(B, spp) for B in (1, 7, 64) for spp in (1, 3, 5, 64, 70)]


@pytest.mark.parametrize("B,spp", ACC)
def test_accumulate_forward_is_the_documented_sum(oracle_mod, B, spp):
    c = P.accumulate_case(B, spp, 14, 14)
    want = P.Numpy32().accumulate(c)
    got = P.Oracle(oracle_mod, 1).accumulate(c)
    assert (c["path_of"] < 0).any() or B * spp < 8
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("spread", [1, 14])
def test_grad_radiance_against_float64(oracle_mod, spread):
    c = P.accumulate_case(64, 5, 14, spread)
    terms = {k: c[k] for k in ("e0", "path_of", "e1", "coef1", "e2", "coef2", "B", "spp")}
    got = oracle_mod.grad_radiance(terms, c["gL"], 14)
    g64, cnt = P.accumulate_bwd_np(c["gL"], c["e0"], c["path_of"], c["e1"], c["coef1"], c["e2"], c["coef2"], 64, 5, 14)
    g32, _ = P.accumulate_bwd_np(c["gL"], c["e0"], c["path_of"], c["e1"], c["coef1"], c["e2"], c["coef2"], 64, 5, 14, np.float32)
    tol = max(8 * np.abs(g32 - g64).max(), cnt.max() * P.U * np.abs(g64).max())
    assert np.abs(got - g64).max() <= tol
    assert (got[cnt == 0] == 0).all() and (cnt[spread:] == 0).all()


# ------------------------------------------------------------------------------------------------ the restatement against the reference's own Python, per path
class _Golden:
    def __init__(self):
        from conftest import golden
        self.d = golden("pt_stage_ref.npz")

    def rec(self, run, i, kind):
        pre = f"{run}/{i:02d}/{kind}/"
        out = {k[len(pre):]: self.d[k] for k in self.d.files if k.startswith(pre)}
        assert out, pre
        return out


def _bounce64(G, run, i0, x, n, wo, mat, variant, trace_rough):
    """One bounce in float64 from the reference's recorded stage boundaries (records i0 .. i0 + 4: sample_emitter, the visibility hit, sample_brdf, the next hit,
    the material there) -> term1, term2 (radiance included), valid_next, the next hit's record and material"""
    import brdf_ref64 as R
    sc = P.scene("open")
    rad, area = G.d["radiance"].astype(np.float64), sc["em"]["area"].astype(np.float64)
    se, vh, sb, nh, m2 = (G.rec(run, i0 + k, kind) for k, kind in enumerate(("sample_emitter", "hit", "sample_brdf", "hit", "material")))
    np.testing.assert_array_equal(se["position"], x)
    rows = {"rough": mat["roughness"].reshape(-1), "albedo": mat["albedo"], "metal": mat["metallic"].reshape(-1)}
    hit = vh["idx"] >= 0
    k = np.maximum(vh["idx"], 0)
    dl = vh["position"] - x
    coef1 = P.nee_formula(R.cosines(se["wi"], wo, n), 0.0, (dl * dl).sum(-1), np.abs((se["wi"] * vh["normal"]).sum(-1)), hit, ~hit | (se["tri"] == vh["idx"]),
                          se["pdf"].reshape(-1), rows, variant, np.float64)[0]
    e1 = np.where(hit & sc["is_emitter"][k], sc["ord_of"][k], -1)
    term1 = np.where((e1 >= 0)[:, None], coef1 * rad[np.maximum(e1, 0)], 0.0)
    a = {"pos": x, "pos_next": nh["position"], "nrm_next": nh["normal"], "wi": sb["wi"], "tri_next": nh["idx"], "pdf": sb["pdf"].reshape(-1), "weight": sb["weight"]}
    coef2, const2, e2, vn, _, und = P.finish_formula(sc, a, m2["roughness"].reshape(-1), trace_rough, variant[0], np.float64, True, area=area)
    assert not und.any()
    term2 = const2 + np.where((e2 >= 0)[:, None], coef2 * rad[np.maximum(e2, 0)], 0.0)
    return term1, term2, vn, a, m2


def _assert_paths(name, got, want, scale):
    err = np.abs(got - want) / np.maximum(scale.max(-1, keepdims=True), 1e-300)
    print(f"{name}: {len(want)} paths, worst relative deviation {float(err.max()):.3g}, {int((np.abs(want).sum(-1) > 0).sum())} paths carry light")
    assert (err <= 1e-12).all(), f"{name}: paths {np.nonzero((err > 1e-12).any(-1))[0][:8].tolist()}"


def test_restatement_is_the_references_path_tracing_single_per_path():
    """tests/golden/pt_stage_ref.npz (tools/make_pt_stage_golden.py): the reference's unmodified path_tracing_single at spp = 1 in float64 on the open scene, the
    closest hit exact.  Its recorded sampled directions, hits and material rows go through the restatement's float64 stage formulas (constants in double); every
    path's L must agree to a relative 1e-12 of the path's terms: both sides are float64 and only the operation order differs."""
    import brdf_ref64 as R
    G, sc = _Golden(), P.scene("open")
    rad = G.d["radiance"].astype(np.float64)
    h0, mat = G.rec("single", 0, "hit"), G.rec("single", 1, "material")
    k = np.maximum(h0["idx"], 0)
    area0 = (h0["idx"] >= 0) & sc["is_emitter"][k]
    L0 = np.where(area0[:, None], rad[np.maximum(sc["ord_of"][k], 0)], 0.0)
    valid = (h0["idx"] >= 0) & ~area0
    with R.float64_constants():
        t1, t2, vn, _, _ = _bounce64(G, "single", 2, h0["position"][valid], h0["normal"][valid], -G.d["rays_d"][valid], mat, (1e-6, 1e-6, 1e-6), 0.0)
    L, scale = L0.copy(), np.abs(L0)
    L[valid] += t1 + t2
    scale[valid] += np.abs(t1) + np.abs(t2)
    assert valid.sum() >= 300 and area0.sum() >= 8 and (~vn).sum() >= 50 and vn.sum() >= 50
    _assert_paths("path_tracing_single", L, G.d["single/L"], scale)


@pytest.mark.parametrize("depth", [1, 2])
def test_restatement_is_the_references_trace_indirect_per_path(depth):
    """the same for trace_indirect at depth 1 and 2 (1e-12, 1e-12, no MIS clamp; trace_roughness 0.6), and the set of paths that valid_next ends: the positions the
    reference carries into its second bounce are exactly position_next[valid_next] of the restatement"""
    import brdf_ref64 as R
    G, run = _Golden(), f"indirect{depth}"
    x, wo, n = G.d[run + "/position"], G.d[run + "/wo"], G.d[run + "/normal"]
    B = len(x)
    L, scale, rows, thr = np.zeros((B, 3)), np.zeros((B, 3)), np.arange(B), np.ones((B, 3))
    mat, i = G.rec(run, 0, "material"), 1
    with R.float64_constants():
        for d in range(depth):
            t1, t2, vn, a, m2 = _bounce64(G, run, i, x, n, wo, mat, (1e-12, 1e-12, 0.0), 0.6)
            with np.errstate(all="ignore"):
                dL = [np.where(np.isnan(thr * t), 0.0, thr * t) for t in (t1, t2)]
            L[rows] += dL[0] + dL[1]
            scale[rows] += np.abs(dL[0]) + np.abs(dL[1])
            thr = (thr * a["weight"])[vn]
            rows, x, wo, n = rows[vn], a["pos_next"][vn], -a["wi"][vn], a["nrm_next"][vn]
            mat = {k: v[vn] for k, v in m2.items()}
            i += 5
            if d + 1 < depth:
                np.testing.assert_array_equal(G.rec(run, i, "sample_emitter")["position"], x)      # the same paths go on
                assert 20 <= len(x) < B
    _assert_paths(f"trace_indirect depth {depth}", L, G.d[run + "/L"], scale)
