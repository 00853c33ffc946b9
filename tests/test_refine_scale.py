"""refine_shading's integrators (trace_indirect, path_tracing_det_diff / _spec, utils/path_tracing.py:409-502 / :50-212) and path_tracing (:214-318) against the
device-arithmetic oracle at the scene and batch sizes refine actually runs, bit for bit.

Which kernels a bounce of trace_indirect runs is decided by its path count N (iris_pt_bounce, iris_amd/csrc/iris_hip.hip): below `merged_min` the two
stages are launched one after the other with one ray per lane; from there the merged pt_bounce_kernel traces both rays of a path in one launch; from
`full_min` on the two stages run as tiled launches of full 4096-ray tiles.  The cases below cover the three regimes with real BVHs and real survivor
patterns (compaction every bounce), and assert from the oracle's `stats` that the regime they claim was the one that ran.

The draws come from oracle.DrawSource: the oracle asks for each draw when the survivor count of the bounce is known and records it; the record is handed
to the GPU integrator unchanged.  The material is the CPU StubMaterial (or its edge-value variant) on both sides, so both see identical rows."""
import argparse
import os
import threading

import numpy as np
import pytest
import torch

from stub_material import EdgeStubMaterial, StubMaterial, edge_material_np, stub_material_np

WAVES = 6          # IRIS_PT_WAVES (iris_amd/csrc/iris_pt.h): resident workgroups per CU of the tile kernels
U = 2.0 ** -24     # unit roundoff of float32


def regime_bounds():
    """(merged_min, full_min) of iris_pt_bounce for this device (pt_tiling in iris_hip.hip): merged when pt_tiling(2 N) holds, i.e. 2 N >= 512 * blocks;
    full tiles when the stage tile (N / (2 blocks) rounded up to 256) reaches 4096, i.e. N / (2 blocks) >= 3841."""
    blocks = torch.cuda.get_device_properties(0).multi_processor_count * WAVES
    return 256 * blocks, 3841 * 2 * blocks


def regime(n):
    merged_min, full_min = regime_bounds()
    return "two-stage" if n < merged_min else ("merged" if n < full_min else "full-tiles")


# ------------------------------------------------------------------------------------------------------------------ CPU: the draw source
def test_draw_source_equals_recorded_list(oracle_mod):
    """On the box: the oracle fed by a DrawSource equals the oracle fed that source's record, for trace_indirect and both path_tracing_det lobes; the
    record has the survivor count of every depth; planted edge values are present."""
    from test_pt_single import _box
    from conftest import golden
    r = golden("refine.npz")
    _, _, sc, em = _box(oracle_mod)
    v = r["valid"]
    for edge in (0.0, 0.05):
        src, st = oracle_mod.DrawSource(3, edge_frac=edge), {}
        a = oracle_mod.trace_indirect(sc, em, stub_material_np, r["position"][v], -r["rays_d"][v], r["normal"][v], 3, src, stats=st)
        b = oracle_mod.trace_indirect(sc, em, stub_material_np, r["position"][v], -r["rays_d"][v], r["normal"][v], 3, src.recorded)
        np.testing.assert_array_equal(a, b)
        assert st["N"][0] == int(v.sum()) and st["N"][1:] == st["continue"][:-1] and len(src.recorded) == 4 * len(st["N"])
        assert [u.shape[0] for u in src.recorded] == [n for n in st["N"] for _ in range(4)]
        if edge:
            for u in src.recorded:
                assert (u == 0.0).any() and (u == np.float32(1 - 2 ** -24)).any() and u.max() < 1.0
        for rough in (None, np.float32(0.412)):
            src = oracle_mod.DrawSource(4, edge_frac=edge)
            args = (sc, em, stub_material_np, r["position"], r["rays_d"], r["normal"], r["triangle_idx"], 4, 3)
            a, ta, wa = oracle_mod.path_tracing_det(*args, src, roughness=rough, return_total=True)
            b = oracle_mod.path_tracing_det(*args, src.recorded, roughness=rough)
            for x, y in zip((a,) if rough is None else a, (b,) if rough is None else b):
                np.testing.assert_array_equal(x, y)
            assert ta.shape == wa.shape == (int((r["triangle_idx"] != -1).sum()), 4, 3)
            m = ta.mean(1, dtype=np.float64).astype(np.float32) if rough is None else (wa[..., :1] * ta).mean(1, dtype=np.float64).astype(np.float32)
            np.testing.assert_array_equal(m, (a if rough is None else a[0])[r["triangle_idx"] != -1])


# ------------------------------------------------------------------------------------------------------------------ GPU fixtures
def _world(oracle_mod, tmp, dev, verts, faces, is_em, slf=None, emi=None, scene=None):
    """GPU scene + SLFEmitterLearn (with emitter_vertices: NEE samples) and the oracle twin, whose SLFEmitter gets the module's own emitter_cdf"""
    from tools import synth
    from iris_amd.model.emitter import SLFEmitterLearn
    from iris_amd.model.slf import VoxelSLF
    from iris_amd.utils.path_tracing import Scene
    s = slf if slf is not None else synth.slf_for(verts, faces, 256)
    e = emi if emi is not None else synth.emitters_for(verts, faces, is_em)
    vs = VoxelSLF(torch.from_numpy(s["mask"]), s["voxel_min"], s["voxel_max"])
    vs.radiance[:] = torch.from_numpy(s["radiance"])
    ep, sp = os.path.join(tmp, "emitter.pth"), os.path.join(tmp, "vslf.npz")
    torch.save({"is_emitter": torch.from_numpy(e["is_emitter"]), "emitter_vertices": torch.from_numpy(e["emitter_vertices"]),
                "emitter_area": torch.from_numpy(e["emitter_area"]), "emitter_normal": torch.zeros(len(e["emitter_area"]), 3),
                "emitter_radiance": torch.from_numpy(e["emitter_radiance"])}, ep)
    torch.save({"mask": torch.from_numpy(s["mask"]), "voxel_min": s["voxel_min"], "voxel_max": s["voxel_max"], "weight": vs.state_dict()}, sp)
    em = SLFEmitterLearn(ep, sp)
    sc = scene if scene is not None else Scene(verts, faces, device=dev)
    osc = oracle_mod.Scene(verts, faces)
    oslf = oracle_mod.VoxelSLF(s["inds"], s["radiance"], s["voxel_min"], s["voxel_max"])
    oem = oracle_mod.SLFEmitter(e["is_emitter"], e["emitter_radiance"], e["emitter_area"], oslf, e["emitter_vertices"], em.emitter_cdf.numpy())
    return {"sc": sc, "em": em, "osc": osc, "oem": oem, "verts": verts}


def _primary(oracle_mod, w, H, W, view):
    """primary hits of a synth camera through the oracle: positions, ray directions (wis), normals, triangle ids (-1 = miss), as numpy"""
    from tools import synth
    K, c2w = synth.camera(H, W, view)
    o, d = oracle_mod.raygen_real(K, c2w, H, W)
    p, n, _, idx, _ = w["osc"].ray_intersect(o, d)
    return p, d, n, idx


@pytest.fixture(scope="module")
def dev():
    from iris_amd import _lib as L
    L.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bench_world(dev, oracle_mod, tmp_path_factory):
    """bench.py's own workload (room seed 1, 1.0 M triangles, H = 256 SLF), built by bench.build_workload"""
    import bench
    ns = argparse.Namespace(scene_seed=1, tris=1_000_000, slf_res=256, layout=0, long_walls=False)
    room, slf, emi, scene, _ = bench.build_workload(ns, dev)
    return _world(oracle_mod, str(tmp_path_factory.mktemp("bench")), dev, room["vertices"], room["faces"], room["is_emitter"], slf, emi, scene)


@pytest.fixture(scope="module")
def room0():
    from tools import synth
    return synth.room(0, 200_000)


@pytest.fixture(scope="module")
def open_world(dev, oracle_mod, room0, tmp_path_factory):
    """the 0.2 M-triangle room without its non-emitting ceiling triangles and without the x = X wall: primary, BRDF and NEE rays escape"""
    from tools import synth
    v, f, ie = room0["vertices"], room0["faces"], room0["is_emitter"]
    tri = v[f].astype(np.float64)
    cen = tri.mean(1)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]); n /= np.linalg.norm(n, axis=1, keepdims=True)
    X, _, Z = synth.ROOM
    drop = ((np.abs(n[:, 2]) > 0.9) & (cen[:, 2] > Z - 0.05) & ~ie) | ((np.abs(n[:, 0]) > 0.9) & (cen[:, 0] > X - 0.05))
    assert 0 < drop.sum() < len(f) // 4
    return _world(oracle_mod, str(tmp_path_factory.mktemp("open")), dev, v, np.ascontiguousarray(f[~drop]), np.ascontiguousarray(ie[~drop]))


@pytest.fixture(scope="module")
def closed_world(dev, oracle_mod, room0, tmp_path_factory):
    return _world(oracle_mod, str(tmp_path_factory.mktemp("closed")), dev, room0["vertices"], room0["faces"], room0["is_emitter"])


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _N(t):
    return t.detach().cpu().numpy()


def _dispatch(mode):
    from iris_amd import _lib as L
    L.debug_set("pt_tile_min", {"default": -1, "tiles": 1, "no-tiles": 1 << 40}[mode])


def _gpu_det(w, dev, mat, prim, spp, depth, rough, rec):
    """(public map(s), per-path totals (P, spp, 3), lobe weights (P, spp, 3)) of the GPU integrator on recorded draws"""
    from iris_amd.utils.path_tracing import _det_common, path_tracing_det_diff, path_tracing_det_spec
    p, d, n, idx = (_T(a, dev) for a in prim)
    u = [_T(x, dev) for x in rec]
    if rough is None:
        out = (_N(path_tracing_det_diff(w["sc"], w["em"], mat, p, d, n, None, idx, spp, depth, uniforms=u)),)
    else:
        out = tuple(_N(t) for t in path_tracing_det_spec(w["sc"], w["em"], mat, float(rough), p, d, n, None, idx, spp, depth, uniforms=u))
    _, wt, total = _det_common(w["sc"], w["em"], mat, p, d, n, idx, spp, depth, 1 if rough is None else 2, 0.0 if rough is None else float(rough), u)
    return out, _N(total), _N(wt).reshape(total.shape)


def _assert_det(oracle_mod, got, gtot, gw, oout, otot, ow, idx, rough):
    """totals and lobe weights bit for bit; the maps at rounding level.
    The GPU map is torch's f32 mean over spp of f32 terms x_k (the totals, or weight * total for the specular lobes: the same f32 products on both sides,
    since the totals are equal); the oracle's is the f64 mean rounded once to f32.  Any order of an f32 sum of n terms is within (n - 1) u sum|x_k| of the
    exact sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4), the division by n adds at most u |mean| and the oracle's rounding u |mean|:
    |GPU - oracle| <= (spp + 1) u mean|x_k| per pixel and channel (7.7e-6 relative to mean|x| at spp 128).  A changed sample changes the totals, which are
    compared exactly; this bound only pins the reduction."""
    np.testing.assert_array_equal(gtot, otot)
    np.testing.assert_array_equal(gw, ow)
    sel = idx != -1
    spp = otot.shape[1]
    for k, (g, o) in enumerate(zip(got, (oout,) if rough is None else oout)):
        x = otot.astype(np.float64) if rough is None else (ow[..., k:k + 1] * otot).astype(np.float64)
        bound = (spp + 1) * U * np.abs(x).mean(1)
        assert np.all(np.abs(g[sel].astype(np.float64) - o[sel]) <= bound), k
        assert not g[~sel].any() and not o[~sel].any()


# ------------------------------------------------------------------------------------------------------------------ A + B: the bench scene
@pytest.fixture(scope="module")
def case_a_indirect(bench_world, oracle_mod):
    """trace_indirect on refine's reference batch (10 240 primary hits x spp 128 = 1.31 M paths, depth 5): inputs, record, oracle result, stats"""
    p, d, n, idx = _primary(oracle_mod, bench_world, 80, 128, 5)
    assert (idx >= 0).all()
    rep = lambda a: np.ascontiguousarray(np.repeat(a, 128, 0))          # noqa: E731
    pos, wo, nrm = rep(p), rep(-d), rep(n)
    src, st = oracle_mod.DrawSource(101), {}
    with oracle_mod.device_arithmetic():
        L = oracle_mod.trace_indirect(bench_world["osc"], bench_world["oem"], stub_material_np, pos, wo, nrm, 5, src, stats=st)
    print("case A trace_indirect stats", st)
    return {"pos": pos, "wo": wo, "nrm": nrm, "rec": src.recorded, "L": L, "stats": st}


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_a_reference_batch_merged_kernel(dev, oracle_mod, bench_world, case_a_indirect):
    """A: the reference batch through path_tracing_det_diff (per-path totals bit for bit, the map at rounding level) and trace_indirect called directly,
    with every depth in the merged regime; path_tracing_det_spec at roughness 0.02 and 1.0 on 20 480 pixels x spp 64."""
    from iris_amd.utils.path_tracing import trace_indirect
    w = bench_world
    prim = _primary(oracle_mod, w, 80, 128, 5)
    assert (prim[3] >= 0).all() and prim[3].shape[0] == 10240
    src, st = oracle_mod.DrawSource(102), {}
    with oracle_mod.device_arithmetic():
        o, ot, ow = oracle_mod.path_tracing_det(w["osc"], w["oem"], stub_material_np, *prim, 128, 5, src, stats=st, return_total=True)
    print("case A det_diff stats", st)
    assert all(regime(x) == "merged" for x in st["N"]), st["N"]
    got, gt, gw = _gpu_det(w, dev, StubMaterial(), prim, 128, 5, None, src.recorded)
    _assert_det(oracle_mod, got, gt, gw, o, ot, ow, prim[3], None)

    c = case_a_indirect
    assert all(regime(x) == "merged" for x in c["stats"]["N"]), c["stats"]["N"]
    Li = trace_indirect(w["sc"], w["em"], StubMaterial(), _T(c["pos"], dev), _T(c["wo"], dev), _T(c["nrm"], dev), 5, uniforms=[_T(u, dev) for u in c["rec"]])
    np.testing.assert_array_equal(_N(Li), c["L"])

    prim2 = _primary(oracle_mod, w, 128, 160, 21)
    assert (prim2[3] >= 0).all()
    for rough in (np.float32(0.02), np.float32(1.0)):
        src, st = oracle_mod.DrawSource(103), {}
        with oracle_mod.device_arithmetic():
            o, ot, ow = oracle_mod.path_tracing_det(w["osc"], w["oem"], stub_material_np, *prim2, 64, 5, src, roughness=rough, stats=st, return_total=True)
        print(f"case A det_spec r={rough} stats", st)
        assert regime(st["N"][0]) == "merged", st["N"]
        got, gt, gw = _gpu_det(w, dev, StubMaterial(), prim2, 64, 5, rough, src.recorded)
        _assert_det(oracle_mod, got, gt, gw, o, ot, ow, prim2[3], rough)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_b_default_batch_full_tiles(dev, bench_world, case_a_indirect):
    """B: refine's default batch (21 M paths).  Paths are independent and compaction keeps their order, so 16 copies of A's batch have, at every depth,
    16 copies of A's survivors: A's recorded draws tiled 16 times are this batch's draws, and every copy must equal A's oracle result."""
    from iris_amd.utils.path_tracing import trace_indirect
    c, R = case_a_indirect, 16
    N0 = c["pos"].shape[0]
    ns = [R * x for x in c["stats"]["N"]]
    print("case B per-depth N", ns)
    assert all(regime(x) == "full-tiles" for x in ns), ns
    tile = lambda a: torch.from_numpy(a).to(dev).repeat(R, *([1] * (a.ndim - 1)))          # noqa: E731
    u = [tile(x) for x in c["rec"]]
    Li = trace_indirect(bench_world["sc"], bench_world["em"], StubMaterial(), tile(c["pos"]), tile(c["wo"]), tile(c["nrm"]), 5, uniforms=u)
    del u
    Li = _N(Li).reshape(R, N0, 3)
    for k in range(R):
        np.testing.assert_array_equal(Li[k], c["L"], err_msg=f"copy {k}")


# ------------------------------------------------------------------------------------------------------------------ C: the open scene
@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_c_open_scene_regime_crossing(dev, oracle_mod, open_world):
    """C: some primary rays miss (sel is not every row), BRDF and NEE rays escape, and the survivor count of one call falls from the merged regime into the
    two-stage one; a second small batch at depth 12 ends with no survivors.  Every case equals the oracle under the default dispatch, with the tile path
    forced and with it disabled."""
    from iris_amd.utils.path_tracing import trace_indirect
    w = open_world
    prim = _primary(oracle_mod, w, 64, 96, 0)
    assert 0 < (prim[3] == -1).sum() < 0.5 * prim[3].size             # primary misses
    spp = 160
    src, st = oracle_mod.DrawSource(201), {}
    with oracle_mod.device_arithmetic():
        o, ot, ow = oracle_mod.path_tracing_det(w["osc"], w["oem"], stub_material_np, *prim, spp, 5, src, stats=st, return_total=True)
    print("case C det_diff stats", st)
    assert 0.02 < st["brdf_miss"][0] / st["N"][0] < 0.9
    assert regime(st["N"][0]) == "merged" and regime(st["N"][-1]) == "two-stage", st["N"]
    # the small batch: points just outside the open wall, facing out -- every BRDF ray escapes, depth 1 has no paths (trace_indirect's N == 0 break)
    rng = np.random.default_rng(7)
    from tools import synth
    X, Y, Z = synth.ROOM
    sp = np.stack([np.full(48, X + 0.3), rng.uniform(0.3, Y - 0.3, 48), rng.uniform(0.3, Z - 0.3, 48)], 1).astype(np.float32)
    sn = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (48, 1))
    swo = rng.normal(size=(48, 3)).astype(np.float32); swo[:, 0] = np.abs(swo[:, 0]) + 0.2
    swo = (swo / np.linalg.norm(swo, axis=1, keepdims=True)).astype(np.float32)
    src2, st2 = oracle_mod.DrawSource(202), {}
    with oracle_mod.device_arithmetic():
        oL2 = oracle_mod.trace_indirect(w["osc"], w["oem"], stub_material_np, sp, swo, sn, 12, src2, stats=st2)
    print("case C depth-12 batch stats", st2)
    assert len(st2["N"]) < 12 and st2["continue"][-1] == 0
    try:
        for mode in ("default", "tiles", "no-tiles"):
            _dispatch(mode)
            got, gt, gw = _gpu_det(w, dev, StubMaterial(), prim, spp, 5, None, src.recorded)
            _assert_det(oracle_mod, got, gt, gw, o, ot, ow, prim[3], None)
            L2 = trace_indirect(w["sc"], w["em"], StubMaterial(), _T(sp, dev), _T(swo, dev), _T(sn, dev), 12, uniforms=[_T(x, dev) for x in src2.recorded])
            np.testing.assert_array_equal(_N(L2), oL2, err_msg=mode)
    finally:
        _dispatch("default")


# ------------------------------------------------------------------------------------------------------------------ D: edges
@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_d_edges_at_dispatch_boundaries(dev, oracle_mod, bench_world):
    """D: draws with 0.0 and 1 - 2**-24 planted, a material with roughness exactly 0.02 / 1.0 / float32(0.6) and its neighbours and metallic 0 / 1, at
    batch sizes on both sides of every dispatch boundary (computed from the device's CU count), through trace_indirect (depth 2) and, at the stage-tiling
    boundary, path_tracing_det_diff (its first lobe is one stage launch)."""
    from iris_amd.utils.path_tracing import trace_indirect
    w = bench_world
    merged_min, _ = regime_bounds()
    p, d, n, idx = _primary(oracle_mod, w, 64, 64, 13)
    assert (idx >= 0).all()
    mat = EdgeStubMaterial()
    seen = set()
    for k, N in enumerate((1, 255, 257, 4097, merged_min - 1, merged_min, 2 * merged_min - 1, 2 * merged_min)):
        rows = np.arange(N) % p.shape[0]
        pos, wo, nrm = (np.ascontiguousarray(a[rows]) for a in (p, -d, n))
        src, st = oracle_mod.DrawSource(300 + k, edge_frac=0.02), {}
        with oracle_mod.device_arithmetic():
            oL = oracle_mod.trace_indirect(w["osc"], w["oem"], edge_material_np, pos, wo, nrm, 2, src, stats=st)
        seen.add(regime(N))
        L = trace_indirect(w["sc"], w["em"], mat, _T(pos, dev), _T(wo, dev), _T(nrm, dev), 2, uniforms=[_T(x, dev) for x in src.recorded])
        np.testing.assert_array_equal(_N(L), oL, err_msg=str(N))
    assert seen == {"two-stage", "merged"}
    r = edge_material_np(p)["roughness"].reshape(-1)
    assert all((r == x).any() for x in EdgeStubMaterial.ROUGH)
    for N in (2 * merged_min - 1, 2 * merged_min):                      # the stage kernels tile from 2 * merged_min rays on
        rows = np.arange(N) % p.shape[0]
        prim = tuple(np.ascontiguousarray(a[rows]) for a in (p, d, n, idx))
        src, st = oracle_mod.DrawSource(400 + N % 7, edge_frac=0.02), {}
        with oracle_mod.device_arithmetic():
            o, ot, ow = oracle_mod.path_tracing_det(w["osc"], w["oem"], edge_material_np, *prim, 1, 2, src, stats=st, return_total=True)
        got, gt, gw = _gpu_det(w, dev, mat, prim, 1, 2, None, src.recorded)
        _assert_det(oracle_mod, got, gt, gw, o, ot, ow, prim[3], None)


# ------------------------------------------------------------------------------------------------------------------ E: path_tracing
@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_e_path_tracing_full(dev, oracle_mod, closed_world):
    """E: render.py's integrator on the closed 0.2 M-triangle room, 8 192 camera rays x spp 8, indir_depth 3: L bit for bit"""
    from iris_amd.utils.path_tracing import path_tracing
    from tools import synth
    w = closed_world
    K, c2w = synth.camera(64, 128, 3)
    rays = oracle_mod.raygen_real(K, c2w, 64, 128, ray_diff=True)
    src, st = oracle_mod.DrawSource(501), {}
    with oracle_mod.device_arithmetic():
        oL, _ = oracle_mod.path_tracing(w["osc"], w["oem"], stub_material_np, *rays, 8, 3, src)
    L = path_tracing(w["sc"], w["em"], StubMaterial(), *(_T(a, dev) for a in rays), 8, 3, uniforms=[_T(x, dev) for x in src.recorded])
    assert len(src.recorded) == 5 + 4 * 3
    np.testing.assert_array_equal(_N(L), oL)


# ------------------------------------------------------------------------------------------------------------------ threads
@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_concurrent_trace_indirect_on_two_streams(dev, oracle_mod, bench_world, case_a_indirect):
    """Two host threads, each on its own stream, run trace_indirect on two different recorded batches at the same time: the survivor count each bounce
    reads back must be its own (path_tracing._Counts), so each result equals its serial result bit for bit."""
    from iris_amd.utils.path_tracing import trace_indirect
    w, c = bench_world, case_a_indirect
    p, d, n, idx = _primary(oracle_mod, w, 64, 100, 17)
    rows = np.arange(420_000) % p.shape[0]
    pos2, wo2, nrm2 = (np.ascontiguousarray(a[rows]) for a in (p, -d, n))
    src2 = oracle_mod.DrawSource(601)
    with oracle_mod.device_arithmetic():
        oracle_mod.trace_indirect(w["osc"], w["oem"], stub_material_np, pos2, wo2, nrm2, 4, src2)
    jobs = [((c["pos"], c["wo"], c["nrm"]), 5, c["rec"]), ((pos2, wo2, nrm2), 4, src2.recorded)]
    jobs = [(tuple(_T(a, dev) for a in x), depth, [_T(u, dev) for u in rec]) for x, depth, rec in jobs]
    serial = [_N(trace_indirect(w["sc"], w["em"], StubMaterial(), *x, depth, uniforms=rec)) for x, depth, rec in jobs]
    np.testing.assert_array_equal(serial[0], c["L"])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in jobs]
    for rep in range(3):
        out, err = [None, None], []

        def run(k):
            try:
                with torch.cuda.device(dev), torch.cuda.stream(streams[k]):
                    x, depth, rec = jobs[k]
                    L = trace_indirect(w["sc"], w["em"], StubMaterial(), *x, depth, uniforms=rec)
                    streams[k].synchronize()
                    out[k] = _N(L)
            except Exception as e:          # (reported below: an exception in a thread would be lost)
                err.append(repr(e))
        ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not err, (rep, err)
        for k in range(2):
            np.testing.assert_array_equal(out[k], serial[k], err_msg=f"repetition {rep}, batch {k}")
