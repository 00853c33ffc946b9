"""8(f)-3: packed shading cache + the BRDF trainer's shading combine (utils/dataset/scannetpp/dataset.py:359-377,409-414;
train_brdf_crf.py:195-203).  GPU tests call the HIP kernels through the C ABI and compare with the golden vectors captured from the
reference (tests/golden/shade_cached.npz) and bit for bit with the oracle.

Below them, the combine and its three gradients per element against the float64 closed form of tests/shade_ref64.py, through ShadingCache.shade and
autograd: R in {1, 2, 5, 6, 8}; roughness at every level knot, at its float neighbours and outside [0.02, 1] (brdf_ref64.lerp_case); metallic and albedo
with exact 0 and 1; a 4099-row cache indexed by a permutation, with repeats and not at all; batches of 1, 63, 65 and 2^15.  The bounds are the rounding
counts of shade_ref64's docstring, which tests/test_shading_cache_cpu.py validates on the oracle and on the float32 restatement.  g_roughness is exactly 0
wherever floor and ceil of the level coincide.

Worst |err| / tol on an MI355X over all R and batches: L 0.41, g_albedo 0.60, g_metallic 0.40, g_roughness 0.38 (the oracle's figures: the kernels' bits)."""
import os

import numpy as np
import pytest

import shade_ref64 as SR
from conftest import golden, rel_l2

R = 6


def _maps(g):
    return g["map_0"], [g[f"map_{1 + j}"] for j in range(R)], [g[f"map_{1 + R + j}"] for j in range(R)]


@pytest.mark.gpu
def test_pack_and_slice_match_reference():
    import torch
    from iris_amd.utils.shading_cache import ShadingCache
    g = golden("shade_cached.npz")
    d, s0, s1 = _maps(g)
    dev = torch.device("cuda:0")
    cache = ShadingCache(len(d), R, dev)
    assert cache.row_floats == 40
    cache.put_view(0, torch.from_numpy(d).to(dev), [torch.from_numpy(m).to(dev) for m in s0], [torch.from_numpy(m).to(dev) for m in s1])
    idx = torch.from_numpy(g["idx"]).to(dev)
    di, sp0, sp1 = cache.gather(idx)
    np.testing.assert_array_equal(di.cpu().numpy(), g["diffuse"])
    np.testing.assert_array_equal(sp0.cpu().numpy(), g["specular0"])
    np.testing.assert_array_equal(sp1.cpu().numpy(), g["specular1"])
    full = torch.cat([t.reshape(len(d), -1) for t in cache.gather(None)], 1)
    np.testing.assert_array_equal(full.cpu().numpy(), g["all_cache"])
    rows = cache.rows.cpu().numpy()
    np.testing.assert_array_equal(rows[:, 3], 0)                       # pad lane
    np.testing.assert_array_equal(rows[:, 4 + 6 * 2:4 + 6 * 2 + 3], s0[2])   # level-interleaved: level 2 spec0, then spec1
    np.testing.assert_array_equal(rows[:, 4 + 6 * 2 + 3:4 + 6 * 3], s1[2])


@pytest.mark.gpu
def test_shade_cached_forward_backward(oracle_mod):
    import torch
    from iris_amd.utils.shading_cache import ShadingCache
    g = golden("shade_cached.npz")
    d, s0, s1 = _maps(g)
    dev = torch.device("cuda:0")
    cache = ShadingCache(len(d), R, dev)
    cache.put_view(0, torch.from_numpy(d).to(dev), [torch.from_numpy(m).to(dev) for m in s0], [torch.from_numpy(m).to(dev) for m in s1])
    idx = torch.from_numpy(g["idx"]).to(dev)
    albedo = torch.from_numpy(g["albedo"]).to(dev).requires_grad_(True)
    metallic = torch.from_numpy(g["metallic"]).to(dev).requires_grad_(True)
    rough = torch.from_numpy(g["roughness"]).to(dev).requires_grad_(True)
    Lc = cache.shade(idx, albedo, metallic, rough)
    np.testing.assert_array_equal(Lc.detach().cpu().numpy(), g["L"])            # forward: bit-exact with the reference's torch ops
    ga, gm, gr = torch.autograd.grad(Lc, [albedo, metallic, rough], torch.from_numpy(g["gL"]).to(dev))
    assert gm.shape == metallic.shape and gr.shape == rough.shape
    # reference autograd (its own summation order): north_star tolerance 1e-4 rel-L2, observed ~1e-7
    for mine, ref in ((ga, g["g_albedo"]), (gm, g["g_metallic"]), (gr, g["g_roughness"])):
        assert rel_l2(mine.cpu().numpy(), ref) < 1e-6
    # oracle (same summation order): bit-exact
    _, oa, om, og = oracle_mod.shade_cached(g["all_cache"], g["idx"], g["albedo"], g["metallic"], g["roughness"], g["gL"])
    np.testing.assert_array_equal(ga.cpu().numpy(), oa)
    np.testing.assert_array_equal(gm.cpu().numpy(), om)
    np.testing.assert_array_equal(gr.cpu().numpy(), og)
    # only the requested gradients are produced
    Lc2 = cache.shade(idx, albedo.detach(), metallic.detach(), rough)
    (gr2,) = torch.autograd.grad(Lc2, [rough], torch.from_numpy(g["gL"]).to(dev))
    np.testing.assert_array_equal(gr2.cpu().numpy(), og)


@pytest.mark.gpu
def test_shade_cached_large_random_vs_oracle(oracle_mod):
    """2 M rows, random permutation batch, odd level count (padded rows), empty batch."""
    import torch
    from iris_amd.utils.shading_cache import ShadingCache
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    for Rl, n, B in ((6, 200_000, 65_536), (5, 10_000, 4096), (1, 1000, 1000)):
        maps = [rng.random((n, 3), dtype=np.float32) * 3 for _ in range(1 + 2 * Rl)]
        cache = ShadingCache(n, Rl, dev)
        assert cache.row_floats % 4 == 0
        cache.put_view(0, torch.from_numpy(maps[0]).to(dev), [torch.from_numpy(m).to(dev) for m in maps[1:1 + Rl]],
                       [torch.from_numpy(m).to(dev) for m in maps[1 + Rl:]])
        rows_ref = oracle_mod.cache_pack(maps[0], maps[1:1 + Rl], maps[1 + Rl:])
        idx = rng.permutation(n)[:B].astype(np.int64)
        albedo = rng.random((B, 3), dtype=np.float32); metallic = rng.random((B, 1), dtype=np.float32)
        rough = (rng.random((B, 1), dtype=np.float32) * 0.98 + 0.02).astype(np.float32) if Rl > 1 else np.full((B, 1), 0.02, np.float32)
        gL = rng.standard_normal((B, 3)).astype(np.float32)
        a = torch.from_numpy(albedo).to(dev).requires_grad_(True); m = torch.from_numpy(metallic).to(dev).requires_grad_(True)
        r = torch.from_numpy(rough).to(dev).requires_grad_(True)
        Lc = cache.shade(torch.from_numpy(idx).to(dev), a, m, r)
        ga, gm, gr = torch.autograd.grad(Lc, [a, m, r], torch.from_numpy(gL).to(dev))
        oL, oa, om, og = oracle_mod.shade_cached(rows_ref, idx, albedo, metallic, rough, gL)
        np.testing.assert_array_equal(Lc.detach().cpu().numpy(), oL)
        np.testing.assert_array_equal(ga.cpu().numpy(), oa)
        np.testing.assert_array_equal(gm.cpu().numpy(), om)
        np.testing.assert_array_equal(gr.cpu().numpy(), og)
    e = cache.shade(torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, 3, device=dev), torch.empty(0, 1, device=dev),
                    torch.empty(0, 1, device=dev))
    assert e.shape == (0, 3)


@pytest.mark.gpu
def test_cache_from_bake_and_exr_round_trip(tmp_path):
    """bake_view -> table (no files) equals bake_view -> EXR files -> table."""
    import torch
    from iris_amd import bake_shading as bs
    from iris_amd.utils import exr
    from iris_amd.utils.dataset import real_ldr
    from iris_amd.utils.shading_cache import ShadingCache
    from tools import synth
    from test_sharding_gpu import _setup
    dev = torch.device("cuda:0")
    os.makedirs(tmp_path / "em", exist_ok=True)
    g, scene, emitter = _setup(dev, str(tmp_path / "em"))
    H, W = 24, 32
    views = []
    for v in range(2):
        K, _ = synth.camera(H, W, v)
        xs, ds = real_ldr.to_world(real_ldr.get_direction(K, (H, W)), g["c2w"], False, device=dev)
        views.append(bs.bake_view(scene, emitter, xs, ds, 16, [8] * 6, seed=v, image_width=W))
    c1 = ShadingCache.from_bake(views)
    for i, v in enumerate(views):
        os.makedirs(tmp_path / "diffuse", exist_ok=True); os.makedirs(tmp_path / "specular", exist_ok=True)
        exr.write_exr(str(tmp_path / "diffuse" / ("%03d.exr" % i)), v["diffuse"].reshape(H, W, 3).cpu().numpy())
        for j in range(6):
            exr.write_exr(str(tmp_path / "specular" / ("%03d_0_%d.exr" % (i, j))), v["specular0"][j].reshape(H, W, 3).cpu().numpy())
            exr.write_exr(str(tmp_path / "specular" / ("%03d_1_%d.exr" % (i, j))), v["specular1"][j].reshape(H, W, 3).cpu().numpy())
    c2 = ShadingCache.from_exr_dir(str(tmp_path), 2, 6, dev)
    assert torch.equal(c1.rows, c2.rows)
    assert float(c1.rows.abs().sum()) > 0


class HipShade:
    """ShadingCache.shade and torch.autograd.grad, numpy in / numpy out"""
    name = "hip"

    def cache(self, R):
        import torch
        from iris_amd.utils.shading_cache import ShadingCache
        dev = torch.device("cuda:0")
        T = lambda a: torch.from_numpy(np.array(a)).to(dev)
        d, s0, s1 = SR.cache_maps(R)
        cache = ShadingCache(SR.N_ROWS, R, dev)
        cache.rows.fill_(float("nan"))                                  # (put_view writes every lane, the padding included)
        cache.put_view(0, T(d), [T(m) for m in s0], [T(m) for m in s1])
        return cache, T

    def shade(self, c):
        import torch
        cache, T = self.cache(c["R"])
        a, m, r = (T(c[k]).requires_grad_(True) for k in ("albedo", "metallic", "rough"))
        L = cache.shade(None if c["idx"] is None else T(c["idx"]), a, m, r)
        ga, gm, gr = torch.autograd.grad(L, [a, m, r], T(c["gL"]))
        assert gm.shape == m.shape and gr.shape == r.shape
        return L.detach().cpu().numpy(), ga.cpu().numpy(), gm.reshape(-1).cpu().numpy(), gr.reshape(-1).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", SR.BATCHES, ids=SR.batch_id)
@pytest.mark.parametrize("levels", SR.LEVELS)
def test_shade_against_float64(levels, batch):
    SR.check_shade(HipShade(), levels, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("levels", SR.LEVELS)
def test_gather_returns_the_packed_maps(levels):
    """gather: the maps bit for bit for every R, through a permutation, an index with repeats and no index; the rows' padding lanes are zero"""
    cache, T = HipShade().cache(levels)
    d, s0, s1 = SR.cache_maps(levels)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)
    for B, mode in SR.BATCHES:
        idx = SR.case(levels, B, mode)["idx"]
        rows = np.arange(SR.N_ROWS) if idx is None else idx
        di, sp0, sp1 = (t.cpu().numpy() for t in cache.gather(None if idx is None else T(idx)))
        assert di.shape == (len(rows), 3) and sp0.shape == (len(rows), levels, 3) and sp1.shape == (len(rows), levels, 3)
        assert np.array_equal(bits(di), bits(d[rows]))
        assert np.array_equal(bits(sp0), bits(np.stack(s0, 1)[rows])) and np.array_equal(bits(sp1), bits(np.stack(s1, 1)[rows]))
    raw = cache.rows.cpu().numpy()
    assert raw.shape[1] % 4 == 0 and raw.shape[1] >= 4 + 6 * levels
    assert (bits(raw[:, 3]) == 0).all() and (bits(raw[:, 4 + 6 * levels:]) == 0).all()
