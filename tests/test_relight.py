"""The relighting stage on the GPU (iris_amd/csrc/iris_relight.h, model/emitter.py AreaEmitter, utils/relight.py): the box room of the golden fixture with
StubMaterial.  Every test runs at <= 65 536 paths."""
import math

import numpy as np
import pytest
import torch

from conftest import golden
from stub_material import StubMaterial
from test_pt_single import _gpu_setup

pytestmark = pytest.mark.gpu
RAY_EPS = 1500.0 * 2.0 ** -24


def _state(g, p):
    return {"is_emitter": torch.from_numpy(g["is_emitter"]), "emitter_vertices": torch.from_numpy(p["emitter_vertices"]),
            "emitter_area": torch.from_numpy(g["emitter_area"]), "emitter_radiance": torch.from_numpy(p["radiance"])}


def _rays(g, H, W, dev):
    """a camera near the floor that looks up: the ceiling lamp fills the middle of the image, ceiling and walls the rest (the fixture's own camera never sees the lamp)"""
    from iris_amd.utils.dataset import real_ldr
    fwd = np.array([0.3, 0.2, 1.0]); fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.array([0.0, 1.0, 0.0])); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c2w = np.stack([right, down, fwd, np.array([1.6, 1.2, 0.4])], 1).astype(np.float32)
    K = np.array([[20.0, 0, W / 2], [0, 20.0, H / 2], [0, 0, 1]], np.float32)
    return real_ldr.to_world(real_ldr.get_direction(K, (H, W)), c2w, True, K, device=dev)


# ------------------------------------------------------------------------------------------------------------------ 1
def test_area_emitter_against_the_reference_lines():
    """eval_emitter / sample_emitter against a float64 restatement of model/emitter.py:69-131; bounds: test_pt_single.check_units' for SLFEmitter."""
    from iris_amd.model.emitter import AreaEmitter
    from iris_amd.utils import lights as LT
    dev = torch.device("cuda:0")
    g, p = golden("bake_box.npz"), golden("pt_single.npz")
    panel = LT.parse_light_config({"panel": {"type": "rectangle", "to_world": [{"type": "translate", "value": [1.0, 2.0, 1.0]}, {"type": "scale", "value": [0.2, 0.3, 1.0]}],
                                             "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [3.0, 2.0, 1.0]}}}})
    c = LT.compose(g["verts"], g["faces"], _state(g, p), panel, keep_lights=1.0)
    em = AreaEmitter(c["emitter"]).to(dev)
    F, K, B = c["faces"].shape[0], 4, 4096
    assert em.n_emitters == K
    gen = torch.Generator().manual_seed(11)
    tri = torch.randint(-1, F, (B,), generator=gen)
    tri[:64] = -1; tri[64:128] = 12; tri[128:192] = 15; tri[192:256] = 3
    pos = torch.rand(B, 3, generator=gen) * 3
    s1, s2 = torch.rand(B, generator=gen), torch.rand(B, 2, generator=gen)
    s1[:4] = torch.tensor([0.0, 0.25, 0.5, 0.999999])
    Le, pdf, vn = em.eval_emitter(pos.to(dev), None, tri.to(dev))
    wi, spdf, stri = em.sample_emitter(s1.to(dev), s2.to(dev), pos.to(dev))
    # float64 restatement
    is_em, area, rad, ev = c["emitter"]["is_emitter"], c["emitter"]["emitter_area"].double(), c["emitter"]["emitter_radiance"], c["emitter"]["emitter_vertices"].double()
    eidx = torch.full((F,), -1, dtype=torch.long); eidx[is_em] = torch.arange(K)
    epdf = torch.full((K,), 1.0 / K, dtype=torch.float64)
    vis = tri != -1
    is_area = is_em[tri.clamp_min(0)] & vis
    rLe = torch.zeros(B, 3); rpdf = torch.zeros(B, dtype=torch.float64)
    e = eidx[tri[is_area]]
    rLe[is_area] = rad[e]; rpdf[is_area] = epdf[e] / area[e].clamp_min(1e-12)
    assert torch.equal(Le.cpu(), rLe) and torch.equal(vn.cpu(), (~is_area) & vis)
    np.testing.assert_allclose(pdf.cpu().numpy()[:, 0], rpdf.numpy(), rtol=1e-6)
    assert is_area.sum() > 200 and (~vis).sum() > 60 and ((~is_area) & vis).sum() > 1000
    np.testing.assert_array_equal(em(tri.to(dev)).cpu().numpy(), rLe.numpy())                   # forward: on triangle_idx alone
    ei = torch.searchsorted(em.emitter_cdf.cpu(), s1.clamp_min(1e-12)).clamp_max(K - 1)
    xi1 = s2[:, 0].double().sqrt()
    u, v = (1 - xi1)[:, None], (xi1 * s2[:, 1].double())[:, None]
    p1 = ev[ei][:, 0] * u + ev[ei][:, 1] * v + ev[ei][:, 2] * (1 - u - v)
    rwi = torch.nn.functional.normalize(p1 - pos.double(), dim=-1)
    assert torch.equal(stri.cpu(), torch.arange(F)[is_em][ei])
    np.testing.assert_allclose(wi.cpu().numpy(), rwi.numpy(), atol=2e-6, rtol=0)
    np.testing.assert_allclose(spdf.cpu().numpy()[:, 0], (epdf[ei] / area[ei].clamp_min(1e-12)).numpy(), rtol=1e-6)
    # a table without any area light is legal; nothing is sampled from it
    from iris_amd import _lib as L
    dark = AreaEmitter(LT.compose(g["verts"], g["faces"], _state(g, p), None)["emitter"]).to(dev)
    Le0, pdf0, vn0 = dark.eval_emitter(pos.to(dev), None, tri.clamp_max(13).to(dev))
    assert dark.n_emitters == 0 and not Le0.any() and not pdf0.any() and torch.equal(vn0.cpu(), tri != -1)
    with pytest.raises(L.IrisError):
        dark.sample_emitter(s1.to(dev), s2.to(dev), pos.to(dev))


# ------------------------------------------------------------------------------------------------------------------ 2
def test_relit_loop_is_the_pinned_one(tmp_path, monkeypatch):
    """keep_lights = 1 and no inserted lights: path_tracing_relit(max_depth 6) on recorded draws == jitter / ray_intersect / primary emitter row + trace_indirect
    (indir_depth 5) on an SLFEmitter whose cache is all zero (zero rows never end a path and add +0), bit for bit."""
    from iris_amd import _lib as L
    from iris_amd.utils import lights as LT
    from iris_amd.utils import path_tracing as PT
    from iris_amd.utils.relight import RelitScene, path_tracing_relit
    dev = torch.device("cuda:0")
    g, p, sc, em = _gpu_setup(tmp_path, dev)
    em.slf.radiance.zero_()
    H, W, spp = 16, 24, 5
    rays_o, rays_d, dxdu, dydv = _rays(g, H, W, dev)
    B, N0 = H * W, H * W * spp
    mat = StubMaterial()
    # the composition of existing public calls, its draws recorded
    torch.manual_seed(5)
    recorded = [torch.rand(2, B, spp, device=dev)]
    real_draws = PT._bounce_draws

    def recording(nxt, own, N, dev_):
        out = tuple(t.clone() for t in real_draws(nxt, own, N, dev_))
        recorded.extend(out)
        return out
    monkeypatch.setattr(PT, "_bounce_draws", recording)
    with torch.no_grad():
        wi0 = torch.empty(N0, 3, device=dev)
        L.check(L.lib().iris_pt_jitter(L.ptr(rays_d), L.ptr(dxdu), L.ptr(dydv), L.ptr(recorded[0]), B, spp, L.ptr(wi0), L.stream()))
        pos, nrm, _, tri, _ = PT.ray_intersect(sc, rays_o.repeat_interleave(spp, 0), wi0)
        e0 = torch.empty(N0, device=dev, dtype=torch.int32); vn = torch.empty(N0, device=dev, dtype=torch.bool)
        L.check(L.lib().iris_pt_primary_emit(em.handle(dev), L.ptr(tri), N0, L.ptr(e0), L.ptr(vn), L.stream()))
        rad = em.radiance_on(dev)
        ref = torch.zeros(N0, 3, device=dev)
        ref[e0 >= 0] = rad[e0[e0 >= 0].long()]
        ref[vn] = ref[vn] + PT.trace_indirect(sc, em, mat, pos[vn].contiguous(), (-wi0[vn]).contiguous(), nrm[vn].contiguous(), 5)
    monkeypatch.setattr(PT, "_bounce_draws", real_draws)
    assert len(recorded) == 1 + 4 * 5 and 0 < int(vn.sum()) < N0 and int((e0 >= 0).sum()) > 0
    relit = RelitScene(LT.compose(g["verts"], g["faces"], _state(g, p), None, keep_lights=1.0), dev)
    assert relit.n_emitters == 2 and relit.n_spots == 0 and not relit.has_classes
    # the BRDF weights of every bounce, as the integrator's _Pool hands them out: the float (N,3) pieces of a bounce are coef1, wi, weight, ... in that order
    from iris_amd.utils import relight as RL
    pools = []

    class RecordingPool(PT._Pool):
        def __init__(self, *a):
            super().__init__(*a)
            self.n3 = []
            pools.append(self)

        def f(self, *shape):
            t = super().f(*shape)
            if len(shape) == 2 and shape[1] == 3:
                self.n3.append(t)
            return t
    monkeypatch.setattr(RL, "_Pool", RecordingPool)
    got = path_tracing_relit(relit, mat, rays_o, rays_d, dxdu, dydv, spp, 6, uniforms=recorded, return_paths=True)
    monkeypatch.setattr(RL, "_Pool", PT._Pool)
    weights = [pl.n3[2] for pl in pools]
    assert len(weights) == 5 and all(bool(torch.isfinite(w).all()) and float(w.max()) > 0 for w in weights)  # (an infinite weight times the zero cache row is NaN in the old sequence)
    assert got.shape == (N0, 3) and float(got.max()) > 0
    assert torch.equal(got, ref)
    # the mean: sequential in s, times 1.0f / spp
    Lm = path_tracing_relit(relit, mat, rays_o, rays_d, dxdu, dydv, spp, 6, uniforms=recorded)
    acc = torch.zeros(B, 3, device=dev)
    for s in range(spp):
        acc = acc + got.reshape(B, spp, 3)[:, s]
    assert torch.equal(Lm, acc * torch.tensor(1.0, device=dev).div(spp))
    # max_depth 1: emitters only
    L1 = path_tracing_relit(relit, mat, rays_o, rays_d, dxdu, dydv, spp, 1, uniforms=recorded[:1], return_paths=True)
    only = torch.zeros(N0, 3, device=dev); only[e0 >= 0] = rad[e0[e0 >= 0].long()]
    assert torch.equal(L1, only)


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.fixture(scope="module")
def bounce_scene():
    from iris_amd.utils import lights as LT
    from iris_amd.utils.relight import RelitScene
    g, p = golden("bake_box.npz"), golden("pt_single.npz")
    return g, RelitScene(LT.compose(g["verts"], g["faces"], _state(g, p), None, keep_lights=1.0), torch.device("cuda:0"))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4099])
def test_fused_shade_is_the_three_launch_sequence(bounce_scene, N):
    """iris_relight_shade == iris_pt_apply(e1) -> iris_pt_brdf_finish(trace_roughness = +inf, no cache) -> iris_pt_apply(e2, const2, weight) on one bounce's
    arrays: L, throughput and valid_next bit for bit."""
    from iris_amd import _lib as L
    from iris_amd.utils import path_tracing as PT
    dev = torch.device("cuda:0")
    g, relit = bounce_scene
    lib, eh = L.lib(), relit.emitter.handle(dev)
    gen = torch.Generator().manual_seed(100 + N)
    R = lambda *s: torch.rand(*s, generator=gen).to(dev)          # noqa: E731
    d = torch.nn.functional.normalize(R(N, 3) * 2 - 1, dim=-1)
    o = torch.tensor([2.0, 1.5, 1.2], device=dev).expand(N, 3).contiguous()
    pos, nrm, _, tri, ok = PT.ray_intersect(relit.scene, o, d)
    assert bool(ok.all())
    wo = (-d).contiguous()
    a, r, m = PT._mat_tensors(StubMaterial()(pos))
    s1, s2, s1b, s2b = R(N), R(N, 2), R(N), R(N, 2)
    f3 = lambda: torch.empty(N, 3, device=dev)                    # noqa: E731
    coef1, wi, w, pos_n, nrm_n = f3(), f3(), f3(), f3(), f3()
    e1 = torch.empty(N, device=dev, dtype=torch.int32); pdf = torch.empty(N, device=dev)
    tri_n = torch.empty(N, device=dev, dtype=torch.int64); hit = torch.empty(N, device=dev, dtype=torch.bool)
    L.check(lib.iris_pt_bounce(relit.scene.handle, eh, L.ptr(pos), L.ptr(nrm), L.ptr(wo), L.ptr(a), L.ptr(r), L.ptr(m), L.ptr(s1), L.ptr(s2), L.ptr(s1b), L.ptr(s2b), N,
                               L.ptr(coef1), L.ptr(e1), 1e-12, 1e-12, 0.0, L.ptr(wi), L.ptr(pdf), L.ptr(w), L.ptr(pos_n), L.ptr(nrm_n), L.ptr(tri_n), L.ptr(hit), L.stream()))
    e1[::7] = -1                                                   # a few paths whose emitter sample is lost
    assert bool(torch.isfinite(w).all())
    an, rn, mn = (t.clone() for t in PT._mat_tensors(StubMaterial()(pos_n)))
    rows = torch.randperm(N + 3, generator=gen)[:N].to(device=dev, dtype=torch.int32)           # shuffled, unique
    L0, t0 = R(N + 3, 3), R(N, 3) * 1.3 + 0.2
    rad = relit.emitter.radiance_on(dev)
    # the sequence
    Ls, ts = L0.clone(), t0.clone()
    coef2, const2 = f3(), f3()
    e2 = torch.empty(N, device=dev, dtype=torch.int32); vs = torch.empty(N, device=dev, dtype=torch.bool)
    L.check(lib.iris_pt_apply(L.ptr(Ls), L.ptr(rows), L.ptr(ts), L.ptr(rad), L.ptr(e1), L.ptr(coef1), None, None, N, 1, L.stream()))
    L.check(lib.iris_pt_brdf_finish(eh, None, L.ptr(pos), L.ptr(pos_n), L.ptr(nrm_n), L.ptr(wi), L.ptr(tri_n), L.ptr(rn), L.ptr(pdf), L.ptr(w), N,
                                    L.ptr(coef2), L.ptr(const2), L.ptr(e2), L.ptr(vs), math.inf, 1e-12, L.stream()))
    L.check(lib.iris_pt_apply(L.ptr(Ls), L.ptr(rows), L.ptr(ts), L.ptr(rad), L.ptr(e2), L.ptr(coef2), L.ptr(const2), L.ptr(w), N, 1, L.stream()))
    # the fused stage
    Lf, tf = L0.clone(), t0.clone()
    vf = torch.empty(N, device=dev, dtype=torch.bool)
    L.check(lib.iris_relight_shade(eh, None, 0, None, 0, L.ptr(pos), L.ptr(pos_n), L.ptr(nrm_n), L.ptr(wi), L.ptr(tri_n), L.ptr(pdf), L.ptr(w), L.ptr(an), L.ptr(rn), L.ptr(mn),
                                   L.ptr(rad), L.ptr(e1), L.ptr(coef1), None, None, None, L.ptr(Lf), L.ptr(rows), L.ptr(tf), L.ptr(vf), N, 1e-12, L.stream()))
    assert torch.equal(Lf, Ls) and torch.equal(tf, ts) and torch.equal(vf, vs)
    if N == 4099:                                                  # (the case that is sure to hold every kind of path)
        assert not torch.equal(Ls, L0) and int((e2 >= 0).sum()) > 0 and 0 < int(vs.sum()) < N and int(((e1 >= 0) & (coef1.sum(-1) > 0)).sum()) > 0
    # without a roughness bound the finish stage still insists on its cache
    with pytest.raises(L.IrisError):
        L.check(lib.iris_pt_brdf_finish(eh, None, L.ptr(pos), L.ptr(pos_n), L.ptr(nrm_n), L.ptr(wi), L.ptr(tri_n), L.ptr(rn), L.ptr(pdf), L.ptr(w), N,
                                        L.ptr(coef2), L.ptr(const2), L.ptr(e2), L.ptr(vs), 0.6, 1e-12, L.stream()))


# ------------------------------------------------------------------------------------------------------------------ 4
def _spot_room(keep_lights=0.0):
    from iris_amd.utils import lights as LT
    g, p = golden("bake_box.npz"), golden("pt_single.npz")
    o2, far = np.array([0.5, 0.5, 1.3]), np.array([4.0, 2.5, 1.3])
    cfg = {"down": {"type": "spot", "origin": [2.0, 1.5, 2.0], "target": [2.0, 1.5, 0.0], "cutoff_angle": 30.0, "intensity": {"type": "rgb", "value": [4.0, 3.0, 2.0]}},
           "across": {"type": "spot", "origin": o2.tolist(), "target": far.tolist(), "cutoff_angle": 25.0, "intensity": {"type": "rgb", "value": [1.0, 5.0, 9.0]}},
           "ball": {"type": "sphere", "to_world": [{"type": "translate", "value": (0.5 * (o2 + far)).tolist()}, {"type": "scale", "value": [0.3, 0.3, 0.3]}],
                    "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.5, 0.5]}}}}
    return g, p, LT.compose(g["verts"], g["faces"], _state(g, p), LT.parse_light_config(cfg), keep_lights=keep_lights)


def _brdf64(wi, wo, n, albedo, rough, metal):
    """model/brdf.py:138-175 eval_brdf (iris_pt.h eval_brdf1) in float64; returns brdf * NoL (N,3)"""
    dot = lambda a, b: (a * b).sum(-1)                            # noqa: E731
    h = torch.nn.functional.normalize(wi + wo, dim=-1)
    NoL, NoV, VoH, NoH = dot(wi, n).clamp_min(0), dot(wo, n).clamp_min(0), dot(wo, h).clamp_min(0), dot(n, h).clamp_min(0)
    a2 = rough ** 4
    D = a2 / (math.pi * (NoH * NoH * (a2 - 1) + 1) ** 2)
    k = (rough + 1) ** 2 / 8
    G = 1 / (NoL * (1 - k) + k) / (NoV * (1 - k) + k)
    kd = albedo * (1 - metal)[:, None]
    ks = 0.04 * (1 - metal)[:, None] + albedo * metal[:, None]
    F = ks + (1 - ks) * ((1 - VoH) ** 5)[:, None]
    return kd / math.pi * NoL[:, None] + (D * G)[:, None] * F / 4.0 * NoL[:, None]


def test_spot_stage_against_float64():
    """iris_pt_nee_spot's (coef, e) against a float64 restatement of its documented formula on the same float32 inputs, occlusion from ray_intersect.
    Tolerance, from the number formats: eval_brdf in float32 is held to rtol 2e-4, atol 1e-5 (test_pt_single.check_units); the falloff's numerator
    cutoff - acos(c) carries the absolute error of acos(c) near 25 - 30 degrees, <= 2.5 ulp(1) / sin(19 degrees) ~ 5e-7, over cutoff - beam >= 0.109 rad: 5e-6
    absolute; d^2 and the products add a few ulp (covered by the rtol).  So |coef - ref| <= 2e-4 |ref| + S / d^2 (1e-5 + 5e-6 brdf).
    Left out: points within 1e-4 rad of a cone boundary or with an occluder within 1e-4 of the light's distance d; at most 1 % of the points."""
    from iris_amd import _lib as L
    from iris_amd.utils import path_tracing as PT
    from iris_amd.utils.relight import RelitScene
    dev = torch.device("cuda:0")
    g, p, c = _spot_room()
    relit = RelitScene(c, dev)
    S, N = relit.n_spots, 8192
    assert S == 2 and relit.n_emitters == 0 and relit.has_classes
    gen = torch.Generator().manual_seed(4)
    R = lambda *s: torch.rand(*s, generator=gen)                  # noqa: E731
    face = torch.randint(0, 5, (N,), generator=gen)
    uv = R(N, 2)
    pos, nrm = torch.zeros(N, 3), torch.zeros(N, 3)
    for k, (origin, eu, ev, nn) in enumerate((((0, 0, 0), (4, 0, 0), (0, 3, 0), (0, 0, 1)), ((0, 0, 0), (4, 0, 0), (0, 0, 2.6), (0, 1, 0)), ((0, 3, 0), (4, 0, 0), (0, 0, 2.6), (0, -1, 0)),
                                              ((0, 0, 0), (0, 3, 0), (0, 0, 2.6), (1, 0, 0)), ((4, 0, 0), (0, 3, 0), (0, 0, 2.6), (-1, 0, 0)))):
        sel = face == k
        pos[sel] = torch.tensor(origin, dtype=torch.float32) + uv[sel, :1] * torch.tensor(eu, dtype=torch.float32) + uv[sel, 1:] * torch.tensor(ev, dtype=torch.float32)
        nrm[sel] = torch.tensor(nn, dtype=torch.float32)
    wo = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    wo = torch.where(((wo * nrm).sum(-1) < 0)[:, None], wo - 2 * (wo * nrm).sum(-1, keepdim=True) * nrm, wo)
    wo = torch.nn.functional.normalize(wo + 0.05 * nrm, dim=-1)                                   # above the surface
    pick = R(N)
    a, r, m = PT._mat_tensors(StubMaterial()(pos))
    pos_d, nrm_d, wo_d, pick_d = pos.to(dev), nrm.to(dev), wo.to(dev).contiguous(), pick.to(dev)
    a_d, r_d, m_d = a.to(dev), r.to(dev), m.to(dev)
    coef = torch.empty(N, 3, device=dev); e = torch.empty(N, device=dev, dtype=torch.int32)
    L.check(L.lib().iris_pt_nee_spot(relit.scene.handle, L.ptr(pos_d), L.ptr(nrm_d), L.ptr(wo_d), L.ptr(a_d), L.ptr(r_d), L.ptr(m_d), L.ptr(pick_d), L.ptr(relit.spots), S, N,
                                     L.ptr(coef), L.ptr(e), L.stream()))
    # float64 restatement
    sp = relit.spots.cpu().double()
    j = (pick * np.float32(S)).to(torch.int64).clamp(0, S - 1)
    x = pos.double()
    dlt = sp[j, 0:3] - x
    d = dlt.norm(dim=-1)
    wi = dlt / d[:, None]
    cosang = (-wi * sp[j, 3:6]).sum(-1)
    ang = torch.acos(cosang.clamp(-1, 1))
    cutoff, beam = sp[j, 6], sp[j, 7]
    fall = torch.where(cosang >= sp[j, 9], torch.ones_like(ang), torch.where(cosang > sp[j, 8], (cutoff - ang) / (cutoff - beam), torch.zeros_like(ang)))
    wi32 = wi.float().to(dev)
    o32 = (pos_d + np.float32(RAY_EPS) * wi32).contiguous()
    hp, _, _, _, hv = PT.ray_intersect(relit.scene, o32, wi32.contiguous())
    dist = (hp.cpu().double() - o32.cpu().double()).norm(dim=-1)
    limit = (d - RAY_EPS) * (1 - 1e-4)
    occluded = hv.cpu() & (dist < limit)
    lit = (~occluded) & (fall > 0)
    brdf = _brdf64(wi, wo.double(), nrm.double(), a.double(), r.double(), m.double())
    ref = torch.where(lit[:, None], (S * fall / d.pow(2).clamp_min(1e-12))[:, None] * brdf, torch.zeros_like(brdf))
    # left out: the cone boundaries and occluders at the light's own distance
    out = ((ang - cutoff).abs() < 1e-4) | ((ang - beam).abs() < 1e-4) | (hv.cpu() & ((dist - d).abs() < 1e-4))
    assert float(out.float().mean()) <= 0.01
    keep = ~out
    e_ref = torch.where(lit, j, torch.full_like(j, -1))
    print("spot stage: left out", int(out.sum()), "lit", int(lit.sum()), "occluded in cone", int((occluded & (fall > 0)).sum()),
          "max abs err", float((coef.cpu().double() - ref)[keep].abs().max()))
    assert torch.equal(e.cpu().long()[keep], e_ref[keep])
    tol = 2e-4 * ref.abs() + (S / d.pow(2))[:, None] * (1e-5 + 5e-6 * brdf)
    assert bool(((coef.cpu().double() - ref).abs() <= tol)[keep].all())
    # both spots light something, both fall-off zones and the occluder are exercised
    assert all(int((lit & (j == k)).sum()) > 50 for k in range(S))
    assert int((lit & (fall < 1)).sum()) > 50 and int((occluded & (fall > 0)).sum()) > 20


# ------------------------------------------------------------------------------------------------------------------ 5
def test_relit_room_end_to_end():
    """absorbers, a constant material, spots and an inserted area light through path_tracing_relit and relight_view"""
    from iris_amd.render_relight import relight_view
    from iris_amd.utils import lights as LT
    from iris_amd.utils.relight import RelitScene, path_tracing_relit
    dev = torch.device("cuda:0")
    g, p, c = _spot_room()
    H, W, spp = 16, 24, 4
    rays = _rays(g, H, W, dev)
    mat = StubMaterial()
    # the room with its lamp switched off and nothing put in: black
    dark = RelitScene(LT.compose(g["verts"], g["faces"], _state(g, p), None), dev)
    assert dark.n_emitters == 0 and dark.has_classes
    assert not path_tracing_relit(dark, mat, *rays, spp, 4).any()
    # spots alone (K = 0): light arrives, finite and non-negative; at max_depth 1 nothing does (a spot is not visible)
    spots = RelitScene(c, dev)
    torch.manual_seed(3)
    Ls = path_tracing_relit(spots, mat, *rays, spp, 3)
    assert Ls.shape == (H * W, 3) and bool(torch.isfinite(Ls).all()) and float(Ls.min()) >= 0 and float(Ls.max()) > 0
    assert not path_tracing_relit(spots, mat, *rays, spp, 1).any()
    # an emissive panel on top: the view stage (denoiser, response model, box average at anti_aliasing 2)
    cfg = {"panel": {"type": "rectangle", "to_world": [{"type": "translate", "value": [2.0, 1.5, 2.4]}, {"type": "scale", "value": [0.5, 0.5, 0.5]}, {"type": "rotate", "axis": [1, 0, 0], "angle": 180}],
                     "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [20, 20, 20]}}}}
    panel = RelitScene(LT.compose(g["verts"], g["faces"], _state(g, p), LT.parse_light_config(cfg)), dev)
    assert panel.n_emitters == 2
    from iris_amd.model.crf import EmorCRF
    k = torch.linspace(0, 1, 1024)
    crf = EmorCRF.from_arrays(k ** 0.45, torch.stack([torch.sin(3.14159 * k * (i + 1)) * 0.05 for i in range(3)]))
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
    crf = crf.to(dev)
    h, w = H // 2, W // 2
    out = relight_view(panel, mat, crf, rays, (h, w), 8, 4, indir_depth=1, anti_aliasing=2)
    assert out["rgb_full"].shape == (H, W, 3) and out["rounds"] == 2
    assert bool(torch.isfinite(out["rgb_full"]).all()) and float(out["rgb_full"].mean()) > 0
    # the LDR image: the response of the denoised image at the anti-aliased size, then the mean of every 2 x 2 block (four numbers in [0,1]: a few ulp of 1)
    with torch.no_grad():
        full = crf(out["rgb_full"].reshape(-1, 3).contiguous(), 1.0).reshape(h, 2, w, 2, 3)
    blocks = (full[:, 0, :, 0] + full[:, 0, :, 1] + full[:, 1, :, 0] + full[:, 1, :, 1]) / 4
    assert out["rgb_ldr"].shape == (h, w, 3) and float(blocks.max() - blocks.min()) > 0.01
    np.testing.assert_allclose(out["rgb_ldr"].cpu().numpy(), blocks.cpu().numpy(), rtol=0, atol=1e-6)
    # without a response model there is no LDR image, and without the denoiser the HDR image is the plain mean of the rounds
    raw = relight_view(panel, mat, None, rays, (h, w), 4, 4, indir_depth=1, anti_aliasing=2, denoise=False)
    assert raw["rgb_ldr"] is None and raw["rounds"] == 1 and raw["rgb_full"].shape == (H, W, 3)


# ------------------------------------------------------------------------------------------------------------------ 6
def _class_room(keep_lights=0.0):
    """the box room with every surface class: its lamp (switched off: absorbers), a diffuse ball (constant material 1), a conductor plate (constant material 2), an emissive
    panel (class 0, in the emitter table) and two spots"""
    from iris_amd.utils import lights as LT
    g, p = golden("bake_box.npz"), golden("pt_single.npz")
    cfg = {"down": {"type": "spot", "origin": [2.0, 1.5, 2.0], "target": [2.0, 1.5, 0.0], "cutoff_angle": 30.0, "intensity": {"type": "rgb", "value": [4.0, 3.0, 2.0]}},
           "across": {"type": "spot", "origin": [0.5, 0.5, 1.3], "target": [4.0, 2.5, 1.3], "cutoff_angle": 25.0, "intensity": {"type": "rgb", "value": [1.0, 5.0, 9.0]}},
           "ball": {"type": "sphere", "to_world": [{"type": "translate", "value": [3.0, 2.0, 1.0]}, {"type": "scale", "value": [0.5, 0.5, 0.5]}],
                    "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.5, 0.3]}}},
           "plate": {"type": "rectangle", "to_world": [{"type": "translate", "value": [1.0, 2.2, 1.2]}, {"type": "rotate", "axis": [1, 0, 0], "angle": 90}, {"type": "scale", "value": [0.6, 0.6, 0.6]}],
                     "bsdf": {"type": "twosided", "bsdf": {"type": "conductor", "material": "none"}}},
           "panel": {"type": "rectangle", "to_world": [{"type": "translate", "value": [2.0, 0.8, 0.3]}, {"type": "scale", "value": [0.5, 0.5, 0.5]}],
                     "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [20, 15, 10]}}}}
    return g, p, LT.compose(g["verts"], g["faces"], _state(g, p), LT.parse_light_config(cfg), keep_lights=keep_lights)


def test_surface_classes_against_indexing():
    """iris_relight_surface on misses, out-of-range indices, network, absorber and constant-material hits against torch indexing: the overridden rows hold cmat's
    (albedo, roughness, metallic), every other row is untouched, valid &= surf >= 0."""
    from iris_amd import _lib as L
    dev = torch.device("cuda:0")
    _, _, c = _class_room()
    surf = torch.as_tensor(c["surf"], dtype=torch.int32)
    cmat = torch.as_tensor(c["cmat"], dtype=torch.float32).reshape(-1, 5)
    F, N = surf.shape[0], 4099
    assert cmat.shape[0] == 2 and not torch.equal(cmat[0], cmat[1]) and int((surf == -1).sum()) == 2 and int((surf == 1).sum()) == 320 and int((surf == 2).sum()) == 2
    gen = torch.Generator().manual_seed(21)
    tri = torch.randint(-1, F, (N,), generator=gen)
    lamp, plate = torch.nonzero(surf == -1)[:, 0], torch.nonzero(surf == 2)[:, 0]
    tri[:40] = -1; tri[40:80] = lamp[0]; tri[80:120] = lamp[1]; tri[120:160] = plate[0]; tri[160:200] = plate[1]; tri[200:300] = torch.randint(0, 12, (100,), generator=gen)
    tri[300:310] = F; tri[310:320] = F + 1000; tri[320:330] = -7                                  # outside the table: left alone, like a miss
    tri = tri[torch.randperm(N, generator=gen)]
    a0, r0, m0 = torch.rand(N, 3, generator=gen), torch.rand(N, generator=gen), torch.rand(N, generator=gen)
    v0 = torch.rand(N, generator=gen) < 0.8
    inside = (tri >= 0) & (tri < F)
    cls = torch.zeros(N, dtype=torch.long); cls[inside] = surf[tri[inside]].long()
    sel = cls > 0
    ea, er, em_ = a0.clone(), r0.clone(), m0.clone()
    ea[sel] = cmat[cls[sel] - 1, :3]; er[sel] = cmat[cls[sel] - 1, 3]; em_[sel] = cmat[cls[sel] - 1, 4]
    ev = v0 & (cls >= 0)
    assert int(sel.sum()) > 300 and int((cls == 2).sum()) >= 80 and int((cls < 0).sum()) >= 80 and int((v0 & (cls < 0)).sum()) > 0 and int((~inside).sum()) >= 70
    surf_d, cmat_d, tri_d = surf.to(dev), cmat.to(dev).contiguous(), tri.to(dev)
    a, r, m, v = a0.to(dev), r0.to(dev), m0.to(dev), v0.to(dev)
    lib = L.lib()
    L.check(lib.iris_relight_surface(L.ptr(surf_d), F, L.ptr(cmat_d), 2, L.ptr(tri_d), N, L.ptr(a), L.ptr(r), L.ptr(m), L.ptr(v), L.stream()))
    assert torch.equal(a.cpu(), ea) and torch.equal(r.cpu(), er) and torch.equal(m.cpu(), em_) and torch.equal(v.cpu(), ev)
    # the two forms the integrator uses: the class alone (primary hits), the rows alone (the first material evaluation)
    v = v0.to(dev)
    L.check(lib.iris_relight_surface(L.ptr(surf_d), F, L.ptr(cmat_d), 2, L.ptr(tri_d), N, None, None, None, L.ptr(v), L.stream()))
    assert torch.equal(v.cpu(), ev)
    a, r, m = a0.to(dev), r0.to(dev), m0.to(dev)
    L.check(lib.iris_relight_surface(L.ptr(surf_d), F, L.ptr(cmat_d), 2, L.ptr(tri_d), N, L.ptr(a), L.ptr(r), L.ptr(m), None, L.stream()))
    assert torch.equal(a.cpu(), ea) and torch.equal(r.cpu(), er) and torch.equal(m.cpu(), em_)
    # no class table: nothing happens
    a, v = a0.to(dev), v0.to(dev)
    L.check(lib.iris_relight_surface(None, 0, None, 0, L.ptr(tri_d), N, L.ptr(a), L.ptr(r), L.ptr(m), L.ptr(v), L.stream()))
    assert torch.equal(a.cpu(), a0) and torch.equal(v.cpu(), v0)


# ------------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("N", [65, 4099])
def test_fused_shade_with_classes_and_spots(N):
    """iris_relight_shade with surface classes, constant materials and the spot pair against the launches it stands for: iris_pt_apply(e1) -> iris_pt_apply with the
    spot table (the spot term is one more term of the same accumulation) -> iris_pt_brdf_finish(+inf) -> iris_pt_apply(e2, weight), the class mask and the material
    override applied by torch indexing.  L, throughput, valid_next and the material rows bit for bit."""
    from iris_amd import _lib as L
    from iris_amd.utils import path_tracing as PT
    from iris_amd.utils.relight import RelitScene
    dev = torch.device("cuda:0")
    _, _, c = _class_room()
    relit = RelitScene(c, dev)
    assert relit.n_emitters == 2 and relit.n_spots == 2 and relit.has_classes
    lib, eh, S = L.lib(), relit.emitter.handle(dev), relit.n_spots
    surf, n_surf, cmat, n_cmat = relit.surf_args()
    gen = torch.Generator().manual_seed(200 + N)
    R = lambda *s: torch.rand(*s, generator=gen).to(dev)          # noqa: E731
    d = torch.nn.functional.normalize(R(N, 3) * 2 - 1, dim=-1)
    o = torch.tensor([2.0, 1.5, 1.6], device=dev).expand(N, 3).contiguous()
    pos, nrm, _, tri, ok = PT.ray_intersect(relit.scene, o, d)
    assert bool(ok.all())
    wo = (-d).contiguous()
    a, r, m = PT._mat_tensors(StubMaterial()(pos))
    s1, s2, s1b, s2b, pick = R(N), R(N, 2), R(N), R(N, 2), R(N)
    f3 = lambda: torch.empty(N, 3, device=dev)                    # noqa: E731
    i32 = lambda: torch.empty(N, device=dev, dtype=torch.int32)   # noqa: E731
    coef1, wi, w, pos_n, nrm_n, coef_s = f3(), f3(), f3(), f3(), f3(), f3()
    e1, e_s, pdf = i32(), i32(), torch.empty(N, device=dev)
    tri_n = torch.empty(N, device=dev, dtype=torch.int64); hit = torch.empty(N, device=dev, dtype=torch.bool)
    L.check(lib.iris_pt_bounce(relit.scene.handle, eh, L.ptr(pos), L.ptr(nrm), L.ptr(wo), L.ptr(a), L.ptr(r), L.ptr(m), L.ptr(s1), L.ptr(s2), L.ptr(s1b), L.ptr(s2b), N,
                               L.ptr(coef1), L.ptr(e1), 1e-12, 1e-12, 0.0, L.ptr(wi), L.ptr(pdf), L.ptr(w), L.ptr(pos_n), L.ptr(nrm_n), L.ptr(tri_n), L.ptr(hit), L.stream()))
    L.check(lib.iris_pt_nee_spot(relit.scene.handle, L.ptr(pos), L.ptr(nrm), L.ptr(wo), L.ptr(a), L.ptr(r), L.ptr(m), L.ptr(pick), L.ptr(relit.spots), S, N,
                                 L.ptr(coef_s), L.ptr(e_s), L.stream()))
    assert bool(torch.isfinite(w).all())
    an0, rn0, mn0 = (t.clone() for t in PT._mat_tensors(StubMaterial()(pos_n)))
    rows = torch.randperm(N + 3, generator=gen)[:N].to(device=dev, dtype=torch.int32)
    L0, t0 = R(N + 3, 3), R(N, 3) * 1.3 + 0.2
    rad, inten = relit.emitter.radiance_on(dev), relit.spot_intensity
    # the launches the stage stands for
    Ls, ts = L0.clone(), t0.clone()
    coef2, const2, e2 = f3(), f3(), i32()
    vs = torch.empty(N, device=dev, dtype=torch.bool)
    L.check(lib.iris_pt_apply(L.ptr(Ls), L.ptr(rows), L.ptr(ts), L.ptr(rad), L.ptr(e1), L.ptr(coef1), None, None, N, 1, L.stream()))
    no_spot = Ls.clone()
    L.check(lib.iris_pt_apply(L.ptr(Ls), L.ptr(rows), L.ptr(ts), L.ptr(inten), L.ptr(e_s), L.ptr(coef_s), None, None, N, 1, L.stream()))
    L.check(lib.iris_pt_brdf_finish(eh, None, L.ptr(pos), L.ptr(pos_n), L.ptr(nrm_n), L.ptr(wi), L.ptr(tri_n), L.ptr(rn0), L.ptr(pdf), L.ptr(w), N,
                                    L.ptr(coef2), L.ptr(const2), L.ptr(e2), L.ptr(vs), math.inf, 1e-12, L.stream()))
    L.check(lib.iris_pt_apply(L.ptr(Ls), L.ptr(rows), L.ptr(ts), L.ptr(rad), L.ptr(e2), L.ptr(coef2), L.ptr(const2), L.ptr(w), N, 1, L.stream()))
    cls = torch.zeros(N, device=dev, dtype=torch.long)
    hitn = tri_n >= 0
    cls[hitn] = relit.surf[tri_n[hitn]].long()
    sel = cls > 0
    ea, er, em_ = an0.clone(), rn0.clone(), mn0.clone()
    ea[sel] = relit.cmat[cls[sel] - 1, :3]; er[sel] = relit.cmat[cls[sel] - 1, 3]; em_[sel] = relit.cmat[cls[sel] - 1, 4]
    ev = vs & (cls >= 0)
    # the fused stage
    Lf, tf = L0.clone(), t0.clone()
    an, rn, mn = an0.clone(), rn0.clone(), mn0.clone()
    vf = torch.empty(N, device=dev, dtype=torch.bool)
    L.check(lib.iris_relight_shade(eh, surf, n_surf, cmat, n_cmat, L.ptr(pos), L.ptr(pos_n), L.ptr(nrm_n), L.ptr(wi), L.ptr(tri_n), L.ptr(pdf), L.ptr(w), L.ptr(an), L.ptr(rn), L.ptr(mn),
                                   L.ptr(rad), L.ptr(e1), L.ptr(coef1), L.ptr(inten), L.ptr(e_s), L.ptr(coef_s), L.ptr(Lf), L.ptr(rows), L.ptr(tf), L.ptr(vf), N, 1e-12, L.stream()))
    assert torch.equal(Lf, Ls) and torch.equal(tf, ts) and torch.equal(vf, ev)
    assert torch.equal(an, ea) and torch.equal(rn, er) and torch.equal(mn, em_)
    if N == 4099:                                                  # every kind of path is there, and each term moves L
        lit_s = (e_s >= 0) & (coef_s.sum(-1) > 0)
        assert all(int((lit_s & (e_s == k)).sum()) > 10 for k in range(S)) and not torch.equal(no_spot, L0) and int((e2 >= 0).sum()) > 0
        spot_moves = (Ls[rows.long()] != no_spot[rows.long()]).any(-1)
        assert int((spot_moves & lit_s).sum()) > 10
        assert int((vs & (cls < 0)).sum()) > 10 and int((cls == 1).sum()) > 10 and int((cls == 2).sum()) > 10 and 0 < int(ev.sum()) < int(vs.sum())


# ------------------------------------------------------------------------------------------------------------------ 8
def test_switched_off_lamp_ends_paths(monkeypatch):
    """A lamp switched off (absorber class, not in the emitter table) is a lamp whose radiance is zero: with spots as the only light, the room composed with
    keep_lights = 0 (K = 0: iris_pt_brdf_trace, the class decides) and the room composed with keep_lights = 1 and the lamp's radiance rows set to zero (K = 2:
    iris_pt_bounce, the emitter table decides; a zero row adds +0) end the same paths, draw the same numbers from the same seed and leave the same bits.
    If absorbers were ignored, the paths that reach the lamp would go on and gather light: shown with the class table cleared by hand."""
    from iris_amd.utils import relight as RL
    from iris_amd.utils.relight import RelitScene, path_tracing_relit
    dev = torch.device("cuda:0")
    g, p, c_off = _spot_room()
    H, W, spp, depth = 16, 24, 4, 4
    rays = _rays(g, H, W, dev)
    mat = StubMaterial()
    c_zero = dict(_spot_room(keep_lights=1.0)[2])
    c_zero["emitter"] = dict(c_zero["emitter"]); c_zero["emitter"]["emitter_radiance"] = torch.zeros_like(c_zero["emitter"]["emitter_radiance"])
    c_ign = dict(c_off); c_ign["surf"] = np.where(np.asarray(c_off["surf"]) < 0, 0, np.asarray(c_off["surf"])).astype(np.int32)
    counts = []
    real = RL._bounce_draws

    def counting(nxt, own, N, dev_):
        counts[-1].append(N)
        return real(nxt, own, N, dev_)
    monkeypatch.setattr(RL, "_bounce_draws", counting)
    imgs = []
    for comp in (c_off, c_zero, c_ign):
        relit = RelitScene(comp, dev)
        counts.append([])
        torch.manual_seed(17)
        imgs.append(path_tracing_relit(relit, mat, *rays, spp, depth, return_paths=True))
    off, zero, ign = imgs
    N0 = H * W * spp
    assert RelitScene(c_off, dev).n_emitters == 0 and RelitScene(c_zero, dev).n_emitters == 2 and int((np.asarray(c_zero["surf"]) < 0).sum()) == 0
    # the lamp is seen directly (those paths end at once) and is reached again at every bounce
    assert len(counts[0]) == depth - 1 and counts[0][0] < N0 and all(counts[0][k + 1] < counts[0][k] for k in range(depth - 2))
    assert counts[1] == counts[0] and torch.equal(off, zero) and float(off.max()) > 0
    # with the classes ignored nothing ends a path in this closed room, and the image changes
    assert counts[2][0] == N0 and counts[2][-1] > counts[0][-1] and not torch.equal(ign, off)
    # a path that starts on the lamp is black; with the classes ignored those same paths are lit
    first = (off == 0).all(-1)
    assert int(first.sum()) >= N0 - counts[0][0] and int((ign[first] > 0).any(-1).sum()) > 0


# ------------------------------------------------------------------------------------------------------------------ 9
def test_cli_main_writes_the_views(tmp_path):
    """python -m iris_amd.render_relight end to end on the box room: mesh, emitter file, checkpoint (response model), light file with a disco ball (recomposed per
    view), --cameras, --material; the EXR of a view holds what relight_view returns under the CLI's seed."""
    import json
    from iris_amd import render_relight as RR
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils.cameras import view_rays
    from iris_amd.utils import lights as LT
    from iris_amd.utils.exr import read_exr
    from iris_amd.utils.relight import RelitScene
    dev = torch.device("cuda:0")
    g, p = golden("bake_box.npz"), golden("pt_single.npz")
    h, w, a = 8, 12, 2
    data, bake, ckpt_dir, outp = tmp_path / "data", tmp_path / "bake", tmp_path / "ckpt" / "exp", tmp_path / "out"
    for d in (data, bake, ckpt_dir):
        d.mkdir(parents=True)
    with open(data / "scene.obj", "w") as fh:
        fh.writelines("v {:.9g} {:.9g} {:.9g}\n".format(*v) for v in g["verts"].tolist())
        fh.writelines("f {} {} {}\n".format(*(i + 1 for i in t)) for t in g["faces"].tolist())
    torch.save(_state(g, p), bake / "emitter.pth")
    torch.save({"voxel_min": float(g["voxel_min"]), "voxel_max": float(g["voxel_max"])}, bake / "vslf.npz")
    k = torch.linspace(0, 1, 1024)
    crf = EmorCRF.from_arrays(k ** 0.45, torch.stack([torch.sin(3.14159 * k * (i + 1)) * 0.05 for i in range(3)]))
    torch.save({"state_dict": {"model_crf." + n: v for n, v in crf.state_dict().items()}}, ckpt_dir / "last.ckpt")
    cfg = {"type": "scene", "panel": {"type": "rectangle", "to_world": [{"type": "translate", "value": [2.0, 1.5, 0.2]}, {"type": "scale", "value": [0.5, 0.5, 0.5]}],
                                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [6, 6, 6]}}},
           "disco_ball": {"position": [1.0, 1.0, 1.5], "radius": 0.2, "light_intensity": 5, "light_num": 3, "spot_intensity": 10, "T": 4}}
    with open(data / "relight.json", "w") as fh:
        json.dump(cfg, fh)
    fwd = np.array([0.3, 0.2, 1.0]); fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.array([0.0, 1.0, 0.0])); right /= np.linalg.norm(right)
    c2w = np.stack([right, np.cross(fwd, right), fwd, np.array([1.6, 1.2, 0.4])], 1).astype(np.float32)
    K = np.array([[10.0, 0, w / 2], [0, 10.0, h / 2], [0, 0, 1]], np.float32)
    with open(data / "cameras.json", "w") as fh:
        json.dump({"img_hw": [h, w], "views": [{"K": K.tolist(), "c2w": c2w.tolist()}] * 2}, fh)
    RR.main(["--experiment_name", "exp", "--checkpoint_path", str(tmp_path / "ckpt"), "--ckpt", "last.ckpt", "--dataset", "generic", str(data), "--cameras", str(data / "cameras.json"),
             "--emitter_path", str(bake), "--light_cfg", str(data / "relight.json"), "--output_path", str(outp), "--SPP", "4", "--spp", "2", "--indir_depth", "1",
             "--anti_aliasing", str(a), "--material", "stub_material:material", "--seed", "3", "--sphere_subdiv", "0"])
    exr = [read_exr(str(outp / f"{i:05d}_rgb.exr")) for i in range(2)]
    assert all(e.shape == (h * a, w * a, 3) and np.isfinite(e).all() and e.max() > 0 for e in exr)
    assert not np.array_equal(exr[0], exr[1])                    # (the same camera twice: the disco ball has turned, and the seed is the view's)
    try:
        from PIL import Image
        png = np.asarray(Image.open(outp / "00001_rgb.png"))
        assert png.shape == (h, w, 3) and png.dtype == np.uint8 and png.max() > 0
    except ImportError:
        assert not (outp / "00001_rgb.png").exists()
    # view 1 again through relight_view: the disco ball at time step 1, the CLI's seed, the camera at the anti-aliased size
    lights = LT.load_light_config(str(data / "relight.json"))
    relit = RelitScene(LT.compose(g["verts"], g["faces"], _state(g, p), lights.at(1), 0.0, 0), dev)
    assert relit.n_spots == 3 and relit.n_emitters == 2 + 3 * 20
    rays = view_rays(RR.scaled_view({"kind": "real", "K": K, "c2w": c2w}, a), (h * a, w * a), dev, ray_diff=True)
    torch.manual_seed(3 * 1000003 + 1); torch.cuda.manual_seed(3 * 1000003 + 1)
    out = RR.relight_view(relit, StubMaterial(), crf.to(dev), rays, (h, w), 4, 2, 1, anti_aliasing=a)
    np.testing.assert_array_equal(exr[1], out["rgb_full"].cpu().numpy())
    assert out["rgb_ldr"].shape == (h, w, 3)
