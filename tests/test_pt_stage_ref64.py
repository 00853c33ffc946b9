"""The HIP path-tracing stages per path against the float64 reference of tests/pt_stage_ref64.py, through the library's public entry points: iris_pt_nee,
iris_pt_brdf_trace with iris_pt_brdf_finish, iris_pt_bounce, iris_pt_apply, iris_pt_accumulate_fwd / _bwd and iris_pt_step_accumulate_bwd.  The tables and the
checks are those of tests/test_pt_stage_ref64_cpu.py, which holds the same tables against the oracle in both modes and the float32 run of the restatement:
that file vouches for the inputs, the branch table and the 2 % cap, and measures E (C = 4 E), which is measured again here from the same two CPU backends.

Every stage runs with pt_tile_min = 1 (the tile kernels) and 1 << 40 (one ray per lane), both variants (1e-6, 1e-6, 1e-6 and 1e-12, 1e-12, none), at
1, 63, 64, 65, 257 rows and the full table (at most 2 900 rows, 12 blocks).  Each test prints its worst |err| / tol and the excluded rows by reason.
On an MI355X every stage's worst |err| / (C tol) is the device-arithmetic oracle's (0.23 .. 0.25: C = 4 E, and the row that sets E is computed by the same float32
operations everywhere), on both kernel paths, both variants and through iris_pt_bounce; apply 0.91 of its bound; the backward scatters 0.003 .. 0.07 of theirs.
"""
import numpy as np
import pytest
import torch

import pt_stage_ref64 as P

pytestmark = pytest.mark.gpu
TILE = {"tiles": 1, "lanes": 1 << 40}


class Hip:
    """the library's entry points, numpy in / numpy out"""
    name = "hip"

    def __init__(self, tmp):
        self.dev, self.tmp, self._sc = torch.device("cuda:0"), tmp, {}

    def T(self, a, dtype=None):
        return torch.from_numpy(np.array(a, dtype=dtype)).to(self.dev).contiguous()      # (a copy: the shared tables are read-only)

    def objects(self, sc):
        from iris_amd.model.emitter import SLFEmitterLearn
        from iris_amd.model.slf import VoxelSLF
        from iris_amd.utils.path_tracing import Scene
        key = sc["em"]["key"]
        if key not in self._sc:
            em, s = sc["em"], sc["slf"]
            slf = VoxelSLF(torch.from_numpy(np.array(s["mask"])), s["vmin"], s["vmax"])
            np.testing.assert_array_equal(slf.inds.numpy(), s["inds"])
            slf.radiance[:] = torch.from_numpy(np.array(s["radiance"]))
            ep, sp = str(self.tmp / f"emitter{len(self._sc)}.pth"), str(self.tmp / f"vslf{len(self._sc)}.npz")
            torch.save({"is_emitter": torch.from_numpy(np.array(sc["is_emitter"])), "emitter_vertices": torch.from_numpy(np.array(em["verts"])),
                        "emitter_area": torch.from_numpy(np.array(em["area"])), "emitter_normal": torch.zeros(em["K"], 3), "emitter_radiance": torch.ones(em["K"], 3)}, ep)
            torch.save({"mask": torch.from_numpy(np.array(s["mask"])), "voxel_min": s["vmin"], "voxel_max": s["vmax"], "weight": slf.state_dict()}, sp)
            m = SLFEmitterLearn(ep, sp).to(self.dev)
            np.testing.assert_array_equal(m.emitter_cdf.cpu().numpy(), em["cdf"])               # the table's cdf is the model's
            self._sc[key] = (Scene(np.array(sc["verts"]), np.array(sc["faces"]), device=self.dev), m)
        return self._sc[key]

    def sample_emitter(self, sc, s1, s2, pos):
        return tuple(t.cpu().numpy() for t in self.objects(sc)[1].sample_emitter(self.T(s1), self.T(s2), self.T(pos)))

    def _common(self, rows):
        return [self.T(rows[k]) for k in ("pos", "nrm", "wo", "albedo", "rough", "metal")]

    def nee(self, sc, rows, variant):
        from iris_amd import _lib as L
        scn, em = self.objects(sc)
        n = len(rows["pos"])
        a = self._common(rows) + [self.T(rows["s1"]), self.T(rows["s2"])]
        coef1, e1 = torch.empty(n, 3, device=self.dev), torch.empty(n, device=self.dev, dtype=torch.int32)
        with torch.cuda.device(self.dev):
            L.check(L.lib().iris_pt_nee(scn.handle, em.handle(self.dev), *[L.ptr(t) for t in a], n, L.ptr(coef1), L.ptr(e1), *[float(v) for v in variant], L.stream()))
        return coef1.cpu().numpy(), e1.cpu().numpy()

    def _trace_outputs(self, n):
        d = self.dev
        return [torch.empty(n, 3, device=d), torch.empty(n, device=d), torch.empty(n, 3, device=d), torch.empty(n, 3, device=d), torch.empty(n, 3, device=d),
                torch.empty(n, device=d, dtype=torch.int64), torch.empty(n, device=d, dtype=torch.bool)]

    def brdf_trace(self, sc, rows):
        from iris_amd import _lib as L
        scn, _ = self.objects(sc)
        n = len(rows["pos"])
        a = self._common(rows) + [self.T(rows["s1b"]), self.T(rows["s2b"])]
        out = self._trace_outputs(n)
        with torch.cuda.device(self.dev):
            L.check(L.lib().iris_pt_brdf_trace(scn.handle, *[L.ptr(t) for t in a], n, *[L.ptr(t) for t in out], 0, 0.0, L.stream()))
        return tuple(t.cpu().numpy() for t in out[:6])

    def finish(self, sc, a, rough_next, trace_rough, g_eps, use_slf=True):
        from iris_amd import _lib as L
        _, em = self.objects(sc)
        n = len(a["pdf"])
        t = [self.T(a[k]) for k in ("pos", "pos_next", "nrm_next", "wi")] + [self.T(a["tri_next"], np.int64)]
        rn = None if rough_next is None else self.T(rough_next)
        pw = [self.T(a["pdf"]), self.T(a["weight"])]
        coef2, const2 = torch.empty(n, 3, device=self.dev), torch.empty(n, 3, device=self.dev)
        e2, vn = torch.empty(n, device=self.dev, dtype=torch.int32), torch.empty(n, device=self.dev, dtype=torch.bool)
        with torch.cuda.device(self.dev):
            L.check(L.lib().iris_pt_brdf_finish(em.handle(self.dev), em.slf.handle(self.dev) if use_slf else None, *[L.ptr(x) for x in t], L.ptr(rn) if rn is not None else None,
                                                *[L.ptr(x) for x in pw], n, L.ptr(coef2), L.ptr(const2), L.ptr(e2), L.ptr(vn), float(trace_rough), float(g_eps), L.stream()))
        return coef2.cpu().numpy(), const2.cpu().numpy(), e2.cpu().numpy(), vn.cpu().numpy()

    def apply(self, tb, nan_to_zero, drop):
        from iris_amd import _lib as L
        g = lambda k: None if drop == k else self.T(tb[k])
        Lacc, rows, thr, e, cst, weight = self.T(tb["L"]), g("rows"), g("throughput"), g("e"), g("cst"), g("weight")
        rad, coef = self.T(tb["radiance"]), self.T(tb["coef"])
        p = lambda t: None if t is None else L.ptr(t)
        with torch.cuda.device(self.dev):
            L.check(L.lib().iris_pt_apply(L.ptr(Lacc), p(rows), p(thr), L.ptr(rad), p(e), L.ptr(coef) if e is not None else None, p(cst), p(weight), len(tb["coef"]),
                                          int(nan_to_zero), L.stream()))
        return Lacc.cpu().numpy(), None if thr is None else thr.cpu().numpy()


class HipBounce(Hip):
    """iris_pt_bounce: the emitter-sampling stage and the BRDF-sampling stage of a bounce behind one launch"""
    name = "hip-bounce"

    def _bounce(self, sc, rows, variant):
        from iris_amd import _lib as L
        scn, em = self.objects(sc)
        n = len(rows["pos"])
        a = self._common(rows) + [self.T(rows[k]) for k in ("s1", "s2", "s1b", "s2b")]
        coef1, e1 = torch.empty(n, 3, device=self.dev), torch.empty(n, device=self.dev, dtype=torch.int32)
        out = self._trace_outputs(n)
        with torch.cuda.device(self.dev):
            L.check(L.lib().iris_pt_bounce(scn.handle, em.handle(self.dev), *[L.ptr(t) for t in a], n, L.ptr(coef1), L.ptr(e1), *[float(v) for v in variant],
                                           *[L.ptr(t) for t in out], L.stream()))
        return (coef1.cpu().numpy(), e1.cpu().numpy()), tuple(t.cpu().numpy() for t in out[:6])

    def nee(self, sc, rows, variant):
        return self._bounce(sc, rows, variant)[0]

    def brdf_trace(self, sc, rows):
        return self._bounce(sc, rows, P.VARIANTS["indirect"])[1]


@pytest.fixture(scope="module")
def yard(oracle_mod):
    return P.Yardstick(oracle_mod)


@pytest.fixture(scope="module", params=["stages", "bounce"])
def back(request, tmp_path_factory):
    return (Hip if request.param == "stages" else HipBounce)(tmp_path_factory.mktemp("pt_stage_ref64"))


@pytest.fixture(params=list(TILE))
def tile(request):
    from iris_amd import _lib as L
    L.debug_set("pt_tile_min", TILE[request.param])
    yield request.param
    L.debug_set("pt_tile_min", -1)


@pytest.mark.parametrize("variant", list(P.VARIANTS))
@pytest.mark.parametrize("scene", P.SCENES)
def test_nee(back, yard, tile, scene, variant):
    P.check_nee(back, yard, scene, variant)


@pytest.mark.parametrize("variant", list(P.VARIANTS))
def test_nee_row_counts(back, yard, tile, variant):
    for n in P.ROW_COUNTS[:-1]:
        P.check_nee(back, yard, "open", variant, n)


@pytest.mark.parametrize("variant", list(P.VARIANTS))
@pytest.mark.parametrize("scene", P.SCENES)
def test_brdf_stage(back, yard, tile, scene, variant):
    P.check_brdf_stage(back, yard, scene, variant)


@pytest.mark.parametrize("variant", list(P.VARIANTS))
def test_brdf_stage_row_counts(back, yard, tile, variant):
    for n in P.ROW_COUNTS[:-1]:
        P.check_brdf_stage(back, yard, "open", variant, n)


@pytest.fixture(scope="module")
def hip(tmp_path_factory):
    return Hip(tmp_path_factory.mktemp("pt_stage_ref64_pure"))


@pytest.mark.parametrize("variant,trace_rough,mode", P.FINISH_TABLE_CASES, ids=[f"{v}-{t}-{m}" for v, t, m in P.FINISH_TABLE_CASES])
def test_finish_table(hip, yard, variant, trace_rough, mode):
    for n in P.ROW_COUNTS:
        P.check_finish_table(hip, yard, variant, trace_rough, mode, n)


@pytest.mark.parametrize("nan_to_zero,drop", P.APPLY_CASES, ids=[f"nan{n}-without-{d}" for n, d in P.APPLY_CASES])
def test_apply(hip, nan_to_zero, drop):
    P.check_apply(hip, nan_to_zero, drop)


def _acc_tensors(hip, c, keys):
    return [hip.T(c[k]) for k in keys]


@pytest.mark.parametrize("B", [1, 7, 64])
@pytest.mark.parametrize("spp", [1, 3, 5, 64, 70])
def test_accumulate_forward_is_the_documented_sum(hip, B, spp):
    from iris_amd import _lib as L
    c = P.accumulate_case(B, spp, 14, 14)
    assert (c["e1"] < 0).any() or B * spp < 8
    want = P.Numpy32().accumulate(c)
    t = _acc_tensors(hip, c, ("radiance", "e0", "path_of", "e1", "coef1", "e2", "coef2", "const2"))
    out = torch.empty(B, 3, device=hip.dev)
    with torch.cuda.device(hip.dev):
        L.check(L.lib().iris_pt_accumulate_fwd(*[L.ptr(x) for x in t], B, spp, L.ptr(out), L.stream()))
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("spread", [1, 14])
@pytest.mark.parametrize("n_calls", [0, 1, 3], ids=["accumulate_bwd", "step-1-call", "step-3-calls"])
def test_accumulate_backward_against_float64(hip, n_calls, spread):
    """elementwise against the float64 scatter under max(8 d32, K 2^-24 max|g64|): K the addends of the fullest radiance row, d32 the float32 numpy scatter's own
    deviation; the rows that no path touches stay exactly 0"""
    from iris_amd import _lib as L
    B, spp, n_rad = 64, 5, 14
    pp = spp * max(n_calls, 1)
    c = P.accumulate_case(B, spp, n_rad, spread, seed=n_calls, per_pixel=pp)
    a = (c["gL"], c["e0"], c["path_of"], c["e1"], c["coef1"], c["e2"], c["coef2"], B, spp, n_rad)
    g64, cnt = P.accumulate_bwd_np(*a, per_pixel=pp)
    g32, _ = P.accumulate_bwd_np(*a, T=np.float32, per_pixel=pp)
    tol = max(8 * np.abs(g32 - g64).max(), cnt.max() * P.U * np.abs(g64).max())
    t = _acc_tensors(hip, c, ("gL", "e0", "path_of", "e1", "coef1", "e2", "coef2"))
    out = torch.zeros(n_rad, 3, device=hip.dev)
    with torch.cuda.device(hip.dev):
        if n_calls == 0:
            L.check(L.lib().iris_pt_accumulate_bwd(*[L.ptr(x) for x in t], B, spp, L.ptr(out), L.stream()))
        else:
            L.check(L.lib().iris_pt_step_accumulate_bwd(*[L.ptr(x) for x in t], B, spp, n_calls, L.ptr(out), L.stream()))
    got = out.cpu().numpy()
    err = float(np.abs(got - g64).max())
    print(f"accumulate backward [{n_calls} calls, {spread} rows]: worst |err| / tol {err / tol:.3f}, fullest row {int(cnt.max())} addends")
    assert err <= tol
    assert (got[cnt == 0] == 0).all() and (cnt[spread:] == 0).all() and cnt[:spread].min() > 0
