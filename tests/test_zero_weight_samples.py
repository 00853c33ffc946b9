"""Zero-weight specular samples (iris_bake.h, dead_samples_skippable): the production bake kernels do not trace a specular sample whose
two GGX weights are both +0 -- it adds Le * 0 to both sums.  The instrumented (`stats`) instantiations and the launches that return per-sample
triangle ids keep tracing every sample, so they are an independent path to compare with: production maps must equal instrumented maps and
the device-arithmetic oracle (which traces everything) bit for bit.

The weights come from the oracle's own Python surface (oracle.sample_specular returns g0 and g1; oracle.philox_u2 the kernels' uniforms), not from a
numpy restatement of the formulas."""
import numpy as np
import pytest
import torch

from test_hip_parity import dev, room_setup, T, N  # noqa: F401  (fixtures)

gpu = pytest.mark.gpu

ROUGH = [None, 0.412, 0.608, 0.804, 1.0]       # the diffuse lobe + the four roughness levels with a measurable dead share
STREAM = {None: 0, 0.412: 3, 0.608: 4, 0.804: 5, 1.0: 6}


def _grazing(nrm, cos=0.05):
    """Unit directions with n . wo = cos: mostly tangent, a little along the normal."""
    n = nrm.astype(np.float64)
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    t = np.cross(n, a); t /= np.linalg.norm(t, axis=1, keepdims=True)
    return (cos * n + np.sqrt(1.0 - cos * cos) * t).astype(np.float32)


def _inputs(s, P):
    """P primary hits of the room; every second pixel looks along the surface (n . wo ~ 0.05)."""
    pos, nrm, wo = s["pos"][:P].copy(), s["nrm"][:P].copy(), s["wo"][:P].copy()
    wo[1::2] = _grazing(nrm[1::2])
    return pos, nrm, wo


def _launch(bs, s, pos, nrm, wo, rough, spp, seed, **kw):
    if rough is None:
        r = bs.bake_diffuse(s["sc"], s["em"], pos, nrm, spp, seed=seed, stream_id=0, **kw)
        return (r,) if isinstance(r, torch.Tensor) else r
    return bs.bake_specular(s["sc"], s["em"], pos, nrm, wo, rough, spp, seed=seed, stream_id=STREAM[rough], **kw)


@gpu
@pytest.mark.parametrize("spp", [16, 128, 40])
@pytest.mark.parametrize("variant", ["tile_sorted", "pixel_per_wave"])
def test_production_equals_instrumented(dev, room_setup, variant, spp):
    from iris_amd import _lib as L
    from iris_amd import bake_shading as bs
    s = room_setup
    v = {"tile_sorted": L.BAKE_TILE_SORTED, "pixel_per_wave": L.BAKE_PIXEL_PER_WAVE}[variant]
    P = min(len(s["pos"]), 3001)
    pos, nrm, wo = (T(x, dev) for x in _inputs(s, P))
    for rough in ROUGH:
        st = torch.zeros(20, device=dev, dtype=torch.int64)
        inst = _launch(bs, s, pos, nrm, wo, rough, spp, 3, stats=st, variant=v)
        prod = _launch(bs, s, pos, nrm, wo, rough, spp, 3, variant=v)
        assert int(st[0]) == P * spp, "the instrumented launch traces every sample"
        for x, y in zip(prod, inst):
            assert torch.isfinite(y).all()
            assert torch.equal(x, y), (variant, spp, rough)


@gpu
@pytest.mark.parametrize("spp", [16, 128, 40])
def test_view_kernel_equals_instrumented_per_lobe_launches(dev, room_setup, spp):
    from iris_amd import _lib as L
    from iris_amd import bake_shading as bs
    s = room_setup
    P = min(len(s["pos"]), 3001)
    pos, nrm, wo = (T(x, dev) for x in _inputs(s, P))
    res = bs.bake_lobes(s["sc"], s["em"], pos, nrm, wo, ROUGH, [spp] * len(ROUGH), seed=3, stream_ids=[STREAM[r] for r in ROUGH])
    for k, rough in enumerate(ROUGH):
        st = torch.zeros(20, device=dev, dtype=torch.int64)
        inst = _launch(bs, s, pos, nrm, wo, rough, spp, 3, stats=st, variant=L.BAKE_TILE_SORTED)
        got = (res[k],) if rough is None else res[k]
        for x, y in zip(got, inst):
            assert torch.equal(x, y), (spp, rough)


@gpu
def test_all_dead_tiles(dev, oracle_mod, room_setup):
    """Normals flipped (n . wo < -0.3) at roughness 0.02: the half vector stays within a fraction of a degree of n, so wi . n ~ wo . n < 0 for every
    sample, every weight is +0 and no tile has a live ray.  The launches must return, with maps that are exactly zero and equal the oracle's."""
    from iris_amd import _lib as L
    from iris_amd import bake_shading as bs
    s = room_setup
    front = (s["nrm"] * s["wo"]).sum(1) > 0.3
    pos, nrm, wo = s["pos"][front][:1500], -s["nrm"][front][:1500], s["wo"][front][:1500]
    P, spp = len(pos), 64
    assert P >= 500
    with oracle_mod.device_arithmetic():
        o0, o1 = oracle_mod.bake(s["osc"], s["oem"], pos, nrm, spp, wo=wo, roughness=np.float32(0.02), seed=13, stream=1)
    tp, tn, tw = T(pos, dev), T(nrm, dev), T(wo, dev)
    outs = [bs.bake_specular(s["sc"], s["em"], tp, tn, tw, 0.02, spp, seed=13, stream_id=1, variant=v)
            for v in (L.BAKE_AUTO, L.BAKE_TILE_SORTED, L.BAKE_PIXEL_PER_WAVE)]
    outs.append(bs.bake_lobes(s["sc"], s["em"], tp, tn, tw, [0.02], [spp], seed=13, stream_ids=[1])[0])
    torch.cuda.synchronize()
    for a, b in outs:
        a, b = N(a), N(b)
        assert not a.any() and not b.any()
        assert not np.signbit(a).any() and not np.signbit(b).any()
        np.testing.assert_array_equal(a, o0)
        np.testing.assert_array_equal(b, o1)


@gpu
def test_per_sample_triangle_ids_still_trace(dev, oracle_mod, room_setup):
    """With per-sample triangle ids requested nothing is skipped: the ids of the zero-weight samples equal the oracle's, hit or miss."""
    from iris_amd import _lib as L
    from iris_amd import bake_shading as bs
    s = room_setup
    P, spp, rough, seed, stream = 1000, 40, 1.0, 17, 6
    pos, nrm, wo = _inputs(s, P)
    with oracle_mod.device_arithmetic():
        o0, o1, otri = oracle_mod.bake(s["osc"], s["oem"], pos, nrm, spp, wo=wo, roughness=np.float32(rough), seed=seed, stream=stream, want_tri=True)
        u2 = oracle_mod.philox_u2(seed, 0, stream, P * spp)
        _, _, g0, g1 = oracle_mod.sample_specular(u2, np.repeat(wo, spp, 0), np.repeat(nrm, spp, 0), rough)
    dead = (g0.reshape(-1) == 0) & (g1.reshape(-1) == 0)
    assert 0.3 < dead.mean() < 0.7
    for v in (L.BAKE_AUTO, L.BAKE_PIXEL_PER_WAVE):
        a, b, tri = bs.bake_specular(s["sc"], s["em"], T(pos, dev), T(nrm, dev), T(wo, dev), rough, spp, seed=seed, stream_id=stream, want_tri=True, variant=v)
        np.testing.assert_array_equal(N(tri)[dead], otri[dead])
        np.testing.assert_array_equal(N(tri), otri)
        np.testing.assert_array_equal(N(a), o0)
        np.testing.assert_array_equal(N(b), o1)
    # ... and the skipping launch gives the same maps
    a, b = bs.bake_specular(s["sc"], s["em"], T(pos, dev), T(nrm, dev), T(wo, dev), rough, spp, seed=seed, stream_id=stream)
    np.testing.assert_array_equal(N(a), o0)
    np.testing.assert_array_equal(N(b), o1)


def test_weights_are_both_zero_or_both_positive(oracle_mod, capsys):
    """What the predicate rests on, taken from the oracle's specular sampler in device-arithmetic mode (oracle.sample_specular exposes g0 and g1)
    on primary hits of the synthetic room, at every roughness level and for the camera's own wo as well as grazing ones: the two weights of a
    sample are finite and either both bit-equal to +0.0 or both positive.  Prints the dead share per level."""
    from tools import synth
    r = synth.room(0, 20_000)
    osc = oracle_mod.Scene(r["vertices"], r["faces"])
    K, c2w = synth.camera(64, 64, 2)
    o, d = oracle_mod.raygen_real(K, c2w, 64, 64)
    _, n, _, _, valid = osc.ray_intersect(o, d)
    nrm, wo = n[valid], -d[valid]
    assert len(nrm) >= 2000
    spp = 64
    shares = {}
    for k, rough in enumerate(np.linspace(0.02, 1.0, 6).astype(np.float32)):
        for name, w in (("camera", wo), ("grazing", _grazing(nrm))):
            with oracle_mod.device_arithmetic():
                u2 = oracle_mod.philox_u2(5, 0, 1 + k, len(nrm) * spp)
                _, _, g0, g1 = oracle_mod.sample_specular(u2, np.repeat(w, spp, 0), np.repeat(nrm, spp, 0), rough)
            g0, g1 = g0.reshape(-1), g1.reshape(-1)
            assert np.isfinite(g0).all() and np.isfinite(g1).all()
            z0, z1 = g0.view(np.uint32) == 0, g1.view(np.uint32) == 0          # bit-equal to +0.0
            shares[(round(float(rough), 3), name)] = float((z0 & z1).mean())
            assert ((z0 & z1) | ((g0 > 0) & (g1 > 0))).all(), (rough, name, int((z0 != z1).sum()), int((g0 < 0).sum()), int((g1 < 0).sum()))
    with capsys.disabled():
        print("\ndead share (g0 == g1 == +0) per roughness level:", shares)
    assert shares[(1.0, "camera")] > 0.3 and shares[(0.02, "camera")] < 0.01
