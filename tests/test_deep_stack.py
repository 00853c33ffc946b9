"""Every traversal driver of iris_trace.h on rays whose stack outgrows its LDS part: the domino scenes of tests/deep_scenes.py (tall one-sided trees out of a few
dozen triangles) through ray_intersect in its three instantiations, the bake kernels (24-entry pixel-per-wave, 12-entry tiles with the workspace slab), the
path-tracing stages (24-entry plain, 10-entry tiles with a private spill), the pooling and label kernels, and the capacity of 96 entries from both sides.
Every comparison is bit for bit: against the oracle's brute force, against the device-arithmetic oracle, or between two kernels that must agree.  How deep each
ray's stack gets is taken from tools/stack_replay (tests/test_deep_stack_cpu.py asserts, without a GPU, that these scenes and rays are what they claim to be)."""
import numpy as np
import pytest
import torch

import deep_scenes as ds
from test_hip_parity import _emitter_files

pytestmark = pytest.mark.gpu

N_RAYS = 16384
COUNTS = (1, 63, 64, 65, 257, 16384)
BUILDS = [(4, -1), (1, -1), (4, 0), (1, 0)]           # (bvh_max_leaf, bvh_presplit_x10: -1 = the default, 8.0)
RAY_EPS = np.float32(1500.0 * 2.0 ** -24)


def N(t):
    return t.detach().cpu().numpy()


def same(a, b):
    """torch.equal on the bits (a NaN equals itself)"""
    if a.is_floating_point():
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def T(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a)).to(dev)                 # (a copy: the shared references are read-only)
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return ds.build_replay(tmp_path_factory.mktemp("stack_replay"))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("replays")


_REF = {}


def brute(oracle_mod, name):
    """(rays, kind, the oracle's brute-force hits) of a scene's 16 384 rays: computed once, left unchanged"""
    if name not in _REF:
        v, f = ds.scene(name)
        o, d, kind = ds.rays(name, N_RAYS)
        ref = oracle_mod.Scene(v, f).ray_intersect(o, d, brute=True)
        for a in (o, d, kind) + tuple(ref):
            a.setflags(write=False)
        _REF[name] = (o, d, kind, ref)
    return _REF[name]


def build_scene(name, dev, layout=None, leaf=4, presplit_x10=-1):
    from iris_amd import _lib as L
    from iris_amd.utils.path_tracing import Scene
    v, f = ds.scene(name)
    L.debug_set("bvh_max_leaf", leaf); L.debug_set("bvh_presplit_x10", presplit_x10)
    try:
        return Scene(v, f, device=dev, layout=L.BVH_DEFAULT if layout is None else layout)
    finally:
        L.debug_set("bvh_max_leaf", -1); L.debug_set("bvh_presplit_x10", -1)


class plain_kernels:
    """inside: the phase-scheduled instantiation of the one-ray-per-lane kernels (no latency mode)"""

    def __enter__(self):
        from iris_amd import _lib as L
        L.debug_set("joint_max_rays", 0)

    def __exit__(self, *a):
        from iris_amd import _lib as L
        L.debug_set("joint_max_rays", -1)


# ------------------------------------------------------------------------------------------------ closest hit
@pytest.mark.parametrize("leaf,presplit_x10", BUILDS)
@pytest.mark.parametrize("name", ds.TRACED)
def test_closest_hit_equals_brute_force(dev, oracle_mod, exe, work, name, leaf, presplit_x10):
    """ray_intersect through <Q8, joint>, <Q8> and <F32> (trace_q8_joint / trace_bvh4: 24 entries in LDS, the rest in the private spill array), deep and shallow rays
    in alternating lanes and in whole waves, 1 ... 16 384 rays: index, barycentrics, position and normal of the oracle's brute force.  "accepted" is the deepest
    tree iris_scene_create takes: its deep rays hold 85 (87 at one triangle per leaf) of the 96 entries."""
    from iris_amd import _lib as L
    from iris_amd.utils.path_tracing import ray_intersect
    o, d, kind, (rp, rn, ruv, ridx, rvalid) = brute(oracle_mod, name)
    v, f = ds.scene(name)
    host = ds.replay(exe, work, v, f, o[:64], d[:64], leaf, 8.0 if presplit_x10 < 0 else presplit_x10 / 10)
    assert 3 * host["depth"] + 4 <= ds.stack_sizes()["capacity"]               # nothing here may trace a tree deeper than the stacks
    to, td = T(o, dev), T(d, dev)
    orders = {"mixed": ds.mixed_order(kind), "blocked": ds.blocked_order(kind)}
    for layout in (L.BVH4_Q8, L.BVH4_F32):
        sc = build_scene(name, dev, layout, leaf, presplit_x10)
        info = sc.info()
        assert info["depth"] == host["depth"] and info["n_leaf_records"] == host["n_leaf_records"], (info, host["depth"])
        for mode in (("joint", "plain") if layout == L.BVH4_Q8 else ("f32",)):
            for oname, perm in orders.items():
                for n in COUNTS:
                    sub = perm[:n]
                    ts = torch.from_numpy(sub).to(dev)
                    if mode == "plain":
                        with plain_kernels():
                            p, nr, uv, idx, valid = ray_intersect(sc, to[ts].contiguous(), td[ts].contiguous())
                    else:
                        p, nr, uv, idx, valid = ray_intersect(sc, to[ts].contiguous(), td[ts].contiguous())
                    tag = (name, mode, oname, n)
                    np.testing.assert_array_equal(N(idx), ridx[sub], err_msg=str(tag))
                    np.testing.assert_array_equal(N(valid), rvalid[sub], err_msg=str(tag))
                    np.testing.assert_array_equal(N(uv), ruv[sub], err_msg=str(tag))
                    np.testing.assert_array_equal(N(p), rp[sub], err_msg=str(tag))
                    np.testing.assert_array_equal(N(nr), rn[sub], err_msg=str(tag))
    assert 0.3 < rvalid.mean() < 0.8


@pytest.mark.parametrize("layout", ["q8", "f32"])
def test_a_tree_deeper_than_the_stacks_is_refused(dev, exe, work, layout):
    """3 * depth + 4 > 96: iris_scene_create refuses, for both layouts and every leaf size; no kernel ever sees this tree.  Neither the cone whose box areas overflow."""
    from iris_amd import _lib as L
    lay = L.BVH4_Q8 if layout == "q8" else L.BVH4_F32
    v, f = ds.scene("refused")
    o, d, _ = ds.rays("refused", 8)
    for leaf, ps in BUILDS:
        host = ds.replay(exe, work, v, f, o, d, leaf, 8.0 if ps < 0 else ps / 10)
        assert 3 * host["depth"] + 4 > ds.stack_sizes()["capacity"]
        with pytest.raises(L.IrisError, match="too deep"):
            build_scene("refused", dev, lay, leaf, ps)
    with pytest.raises(L.IrisError, match="not finite"):
        build_scene("overflow", dev, lay)


# ------------------------------------------------------------------------------------------------ bake kernels
SLF_RANGE = (-1.0e9, 3.0e10)      # the voxel grid spans the whole cone (coordinates up to 1.5^59 = 2.4e10)


@pytest.fixture(scope="module")
def cone(dev, oracle_mod, exe, work, tmp_path_factory):
    """the 60-triangle cone with an emitter table (every fourth domino emits) and a small VoxelSLF, on the device and in the oracle; shading points near the apex
    looking down the cone (deep rays) alternate with points beyond the far end looking back (shallow rays), so every tile and every wave holds both"""
    from tools import synth
    from iris_amd.model.emitter import SLFEmitter, SLFEmitterLearn
    v, f = ds.scene("cone60")
    is_em = np.arange(len(f)) % 4 == 1
    e = synth.emitters_for(v, f, is_em)
    ev = e["emitter_vertices"].astype(np.float64)           # (the areas in double: the far dominoes' cross products overflow float32, their areas do not)
    e["emitter_area"] = (np.linalg.norm(np.cross(ev[:, 1] - ev[:, 0], ev[:, 2] - ev[:, 0]), axis=-1) / 2.0).astype(np.float32)
    assert np.isfinite(e["emitter_area"]).all()
    s = synth.slf_for(v, f, 8, *SLF_RANGE)
    tmp = tmp_path_factory.mktemp("cone")
    ep, sp = _emitter_files(tmp, e["is_emitter"], e["emitter_area"], e["emitter_radiance"], s["mask"], s["inds"], s["radiance"], s["voxel_min"], s["voxel_max"])
    em = SLFEmitter(ep, sp)
    d2 = tmp / "learn"; d2.mkdir()
    ep2, sp2 = str(d2 / "emitter.pth"), str(d2 / "vslf.npz")
    st = torch.load(ep); st["emitter_vertices"] = torch.from_numpy(e["emitter_vertices"]); torch.save(st, ep2)
    torch.save(torch.load(sp), sp2)
    eml = SLFEmitterLearn(ep2, sp2).to(dev)
    osc = oracle_mod.Scene(v, f)
    oslf = oracle_mod.VoxelSLF(s["inds"], s["radiance"], s["voxel_min"], s["voxel_max"])
    oem = oracle_mod.SLFEmitter(e["is_emitter"], e["emitter_radiance"], e["emitter_area"], oslf)
    sc = build_scene("cone60", dev)
    host = ds.replay(exe, work, v, f, np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))
    assert sc.info()["depth"] == host["depth"]
    return {"v": v, "f": f, "sc": sc, "em": em, "eml": eml, "osc": osc, "oem": oem, "depth": host["depth"]}


def shading_points(P, seed=0):
    """(pos, nrm, wo) float32: even rows near the apex, normals inside the cone; odd rows beyond the far end, facing back"""
    rng = np.random.default_rng(seed)
    x_hi = 1.5 ** 59
    ab, ab2 = rng.uniform(0.2, 0.6, (P, 2)), rng.uniform(0.15, 0.45, (P, 2))
    far = np.arange(P) % 2 == 1
    line = np.concatenate([np.ones((P, 1)), ab], 1)
    pos = np.where(far[:, None], 1.5 * x_hi, 0.5) * line
    nrm = np.concatenate([np.ones((P, 1)), ab2], 1)
    nrm = np.where(far[:, None], -1.0, 1.0) * nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    wo = nrm + 0.2 * rng.normal(size=(P, 3))
    wo = wo / np.linalg.norm(wo, axis=1, keepdims=True)
    return pos.astype(np.float32), nrm.astype(np.float32), wo.astype(np.float32)


def test_the_overflow_slab_holds_the_deepest_stack(cone):
    """iris_bake_workspace_bytes: [256 B][blocks x tile rays x 16 (32) B][blocks x (capacity - LDS part) x 256 entries]; Stack<12, GLOBAL_OVF> writes entry sp at
    (sp - 12) * 256 + lane of its workgroup's part.  Read before the first tile launch: the deepest stack this scene can make (3 per level) is inside."""
    from iris_amd import _lib as L
    s = ds.stack_sizes()
    lib = L.lib()
    tile_rays = int(lib.iris_bake_tile_max_spp())
    b0, b1 = int(lib.iris_bake_workspace_bytes(128, 16, 0)), int(lib.iris_bake_workspace_bytes(128, 16, 1))
    blocks, rem = divmod(b1 - b0, tile_rays * 16)
    assert rem == 0 and blocks > 0
    slab, rem = divmod(b0 - 256 - blocks * tile_rays * 16, blocks * 256 * 4)
    assert rem == 0 and slab == s["capacity"] - s["bake_tile"]
    assert 3 * cone["depth"] - s["bake_tile"] <= slab


@pytest.mark.parametrize("spp", [16, 20, 64])
def test_bake_kernels_on_the_cone(dev, oracle_mod, cone, spp):
    """bake_diffuse and bake_specular, pixel-per-wave (trace_bvh4, 24 + private spill) and tile-sorted (trace_stream, 12 + the workspace slab): every bit of the
    device-arithmetic oracle, hit triangles included."""
    from iris_amd import _lib as L
    from iris_amd import bake_shading as bs
    P = 128
    pos, nrm, wo = shading_points(P)
    pix = np.arange(P, dtype=np.int32) * 5 + 2
    with oracle_mod.device_arithmetic():
        want = {None: oracle_mod.bake(cone["osc"], cone["oem"], pos, nrm, spp, seed=3, stream=0, pix_id=pix, want_tri=True)}
        for k, r in ((1, 0.02), (4, 0.608), (6, 1.0)):
            want[r] = oracle_mod.bake(cone["osc"], cone["oem"], pos, nrm, spp, wo=wo, roughness=np.float32(r), seed=3, stream=k, pix_id=pix, want_tri=True)
    otri = want[None][-1].reshape(P, spp)
    assert (otri[0::2] == 0).mean() > 0.1 and (otri[0::2] < 0).mean() > 0.1 and (otri[1::2] >= 0).mean() > 0.1        # near points: hits of the first domino and escapes
    for variant in (L.BAKE_PIXEL_PER_WAVE, L.BAKE_TILE_SORTED):
        got = bs.bake_diffuse(cone["sc"], cone["em"], T(pos, dev), T(nrm, dev), spp, seed=3, stream_id=0, pix_id=T(pix, dev), want_tri=True, variant=variant)
        for a, b in zip(got, want[None]):
            np.testing.assert_array_equal(N(a), b, err_msg=str(("diffuse", variant)))
        plain = bs.bake_diffuse(cone["sc"], cone["em"], T(pos, dev), T(nrm, dev), spp, seed=3, stream_id=0, pix_id=T(pix, dev), variant=variant)
        np.testing.assert_array_equal(N(plain), want[None][0])                       # (without the triangle output: the production instantiation)
        for k, r in ((1, 0.02), (4, 0.608), (6, 1.0)):
            got = bs.bake_specular(cone["sc"], cone["em"], T(pos, dev), T(nrm, dev), T(wo, dev), r, spp, seed=3, stream_id=k, pix_id=T(pix, dev), want_tri=True,
                                   variant=variant)
            for a, b in zip(got, want[r]):
                np.testing.assert_array_equal(N(a), b, err_msg=str((r, variant)))
            got = bs.bake_specular(cone["sc"], cone["em"], T(pos, dev), T(nrm, dev), T(wo, dev), r, spp, seed=3, stream_id=k, pix_id=T(pix, dev), variant=variant)
            for a, b in zip(got, want[r][:2]):
                np.testing.assert_array_equal(N(a), b, err_msg=str((r, variant, "skipping zero-weight samples")))


def test_bake_view_on_the_cone(dev, oracle_mod, cone):
    """bake_view_kernel (all lobes of a view behind one tile launch) from a camera at the apex looking down the cone: primary hits on the first domino and misses,
    the maps of the device-arithmetic oracle on the hits."""
    from iris_amd import bake_shading as bs
    H, W = 24, 32
    a, b = np.meshgrid(np.linspace(0.05, 0.95, W), np.linspace(0.05, 0.95, H))
    d = np.stack([np.ones(H * W), a.ravel(), b.ravel()], 1)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = np.tile(np.array([[0.5, 0.25, 0.25]], np.float32), (H * W, 1))
    out = bs.bake_view(cone["sc"], cone["em"], T(o, dev), T(d, dev), 16, [16] * 6, seed=2, image_width=W)
    op, on, _, oidx, ovalid = cone["osc"].ray_intersect(o, d)
    assert 50 < ovalid.sum() < H * W - 50 and out["n_valid"] == int(ovalid.sum())
    pos, nrm, wo = op[ovalid], on[ovalid], -d[ovalid]
    pix = np.nonzero(ovalid)[0].astype(np.int32)
    vt = torch.from_numpy(ovalid).to(dev)
    with oracle_mod.device_arithmetic():
        (oLd,) = oracle_mod.bake(cone["osc"], cone["oem"], pos, nrm, 16, seed=2, stream=0, pix_id=pix)
        np.testing.assert_array_equal(N(out["diffuse"][vt]), oLd)
        for k, r in enumerate(np.linspace(0.02, 1.0, 6).astype(np.float32)):
            o0, o1 = oracle_mod.bake(cone["osc"], cone["oem"], pos, nrm, 16, wo=wo, roughness=np.float32(torch.linspace(0.02, 1.0, 6)[k]), seed=2, stream=k + 1, pix_id=pix)
            np.testing.assert_array_equal(N(out["specular0"][k][vt]), o0, err_msg=str(k))
            np.testing.assert_array_equal(N(out["specular1"][k][vt]), o1, err_msg=str(k))


@pytest.mark.parametrize("spp", [16, 20, 64])
def test_stack_depth_counters_on_the_cone(dev, oracle_mod, exe, work, cone, spp):
    """The instrumented kernels on rays the host replay knows: sp_gt16 is at least the number of rays the replay sees above 16 entries (not merely >= 0), the per-ray
    counters agree between the two variants, and the instrumented build returns the production bits."""
    from iris_amd import _lib as L
    from iris_amd import bake_shading as bs
    from test_stats import NAMES, PER_RAY, _check
    P = 128
    pos, nrm, wo = shading_points(P, seed=1)
    u2 = np.random.default_rng(spp).random((P * spp, 2)).astype(np.float32)
    rep = lambda a: np.repeat(a, spp, 0)
    with oracle_mod.device_arithmetic():
        wi_d = oracle_mod.sample_diffuse(u2, rep(nrm))[0]
        wi_s = oracle_mod.sample_specular(u2, rep(wo), rep(nrm), 0.608)[0]
    for lobe, rough, wi in ((0, None, wi_d), (4, 0.608, wi_s)):
        o = rep(pos) + RAY_EPS * wi                                                # float32: position + RayEpsilon * wi as the kernel forms it
        host = ds.replay(exe, work, cone["v"], cone["f"], o, wi)
        above = {t: int((host["max_q8"] > t).sum()) for t in (8, 12, 16)}
        print(f"spp {spp} lobe {lobe}: replay sees {above} of {P * spp} rays above 8 / 12 / 16 entries, deepest {int(host['max_q8'].max())}")
        assert above[16] > P * spp // 16 and host["max_q8"].max() > ds.stack_sizes()["plain"]
        got = {}
        for variant in (L.BAKE_TILE_SORTED, L.BAKE_PIXEL_PER_WAVE):
            st = torch.zeros(20, device=dev, dtype=torch.int64)
            if rough is None:
                a = (bs.bake_diffuse(cone["sc"], cone["em"], T(pos, dev), T(nrm, dev), spp, u2=T(u2, dev), stats=st, variant=variant),)
                b = (bs.bake_diffuse(cone["sc"], cone["em"], T(pos, dev), T(nrm, dev), spp, u2=T(u2, dev), variant=variant),)
            else:
                a = bs.bake_specular(cone["sc"], cone["em"], T(pos, dev), T(nrm, dev), T(wo, dev), rough, spp, u2=T(u2, dev), stats=st, variant=variant)
                b = bs.bake_specular(cone["sc"], cone["em"], T(pos, dev), T(nrm, dev), T(wo, dev), rough, spp, u2=T(u2, dev), variant=variant)
            for x, y in zip(a, b):
                assert torch.equal(x, y)
            got[variant] = _check(N(st), P * spp)
            print(f"   variant {variant}: sp_gt8 {got[variant]['sp_gt8']} sp_gt12 {got[variant]['sp_gt12']} sp_gt16 {got[variant]['sp_gt16']}")
            assert got[variant]["sp_gt16"] >= above[16]
        for k in PER_RAY:
            assert got[L.BAKE_TILE_SORTED][k] == got[L.BAKE_PIXEL_PER_WAVE][k], (lobe, k, got)
        assert len(NAMES) == 20


# ------------------------------------------------------------------------------------------------ path-tracing stages
def stage_points(n, dev, seed):
    pos, nrm, wo = shading_points(n, seed)
    return T(pos, dev), T(nrm, dev), T(wo, dev)


@pytest.mark.parametrize("n", [255, 4096, 16384])
def test_pt_stages_tiled_equal_plain_on_the_cone(dev, cone, n):
    """pt_tiled_kernel (trace_stream, 10 entries in LDS + private spill) against the one-ray-per-lane kernels (24 + spill; latency mode and phase mode), every output
    of the three lobes and of the emitter-sampling stage bit for bit; and the next-hit triangles are ray_intersect's along the same rays."""
    from iris_amd import _lib as L
    from iris_amd.utils.path_tracing import ray_intersect
    from test_pt_tiled import _stage_outputs
    pts = stage_points(n, dev, seed=n)
    try:
        L.debug_set("pt_tile_min", 1 << 40)
        joint = _stage_outputs(cone["sc"], cone["eml"], dev, n, seed=n, points=pts)
        with plain_kernels():
            plain = _stage_outputs(cone["sc"], cone["eml"], dev, n, seed=n, points=pts)
        L.debug_set("pt_tile_min", 1)
        tiled = _stage_outputs(cone["sc"], cone["eml"], dev, n, seed=n, points=pts)
    finally:
        L.debug_set("pt_tile_min", -1)
    assert len(joint) == len(plain) == len(tiled) == 20
    for k, (a, b, c) in enumerate(zip(joint, plain, tiled)):
        assert same(a, b), ("joint against plain", k)
        assert same(a, c), ("plain against tiled", k)
    for lobe in range(3):
        wi, tri = joint[6 * lobe], joint[6 * lobe + 5]
        o = pts[0] + float(RAY_EPS) * wi
        idx = ray_intersect(cone["sc"], o.contiguous(), wi.contiguous())[3]
        assert torch.equal(tri, idx), lobe
        t = N(tri)
        assert (t[0::2] == 0).mean() > 0.05 and (t[0::2] < 0).mean() > 0.05        # from the apex: the first domino, or past every hypotenuse
    assert int((joint[19] >= 0).sum()) > 0                                         # visible emitters


@pytest.mark.parametrize("n", [255, 4096, 16384])
def test_pt_bounce_equals_its_two_stages_on_the_cone(dev, cone, n):
    """iris_pt_bounce (2 n rays sorted and traced together: pt_bounce_kernel, 10 + spill, or its small-call fall-back) against iris_pt_nee + iris_pt_brdf_trace"""
    from iris_amd import _lib as L
    pos, nrm, wo = stage_points(n, dev, seed=n + 1)
    g = torch.Generator(device="cpu").manual_seed(n)
    R = lambda *s: torch.rand(*s, generator=g).to(dev)
    albedo, rough, metal = R(n, 3).contiguous(), (R(n) * 0.9 + 0.05).contiguous(), R(n).contiguous()
    s1, s2, s1b, s2b = R(n), R(n, 2), R(n), R(n, 2)
    sc, em = cone["sc"], cone["eml"]

    def outs():
        return ([torch.empty(n, 3, device=dev), torch.empty(n, device=dev, dtype=torch.int32)],
                [torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev),
                 torch.empty(n, device=dev, dtype=torch.int64), torch.empty(n, device=dev, dtype=torch.bool)])
    lib = L.lib()
    first = None
    for tile_min in (1 << 40, 1):
        L.debug_set("pt_tile_min", tile_min)
        try:
            a1, b1 = outs()
            with torch.cuda.device(dev):
                L.check(lib.iris_pt_nee(sc.handle, em.handle(dev), L.ptr(pos), L.ptr(nrm), L.ptr(wo), L.ptr(albedo), L.ptr(rough), L.ptr(metal), L.ptr(s1), L.ptr(s2), n,
                                        L.ptr(a1[0]), L.ptr(a1[1]), 1e-12, 1e-12, 0.0, L.stream()))
                L.check(lib.iris_pt_brdf_trace(sc.handle, L.ptr(pos), L.ptr(nrm), L.ptr(wo), L.ptr(albedo), L.ptr(rough), L.ptr(metal), L.ptr(s1b), L.ptr(s2b), n,
                                               *[L.ptr(t) for t in b1], 0, 0.0, L.stream()))
                a2, b2 = outs()
                L.check(lib.iris_pt_bounce(sc.handle, em.handle(dev), L.ptr(pos), L.ptr(nrm), L.ptr(wo), L.ptr(albedo), L.ptr(rough), L.ptr(metal), L.ptr(s1), L.ptr(s2), L.ptr(s1b),
                                           L.ptr(s2b), n, L.ptr(a2[0]), L.ptr(a2[1]), 1e-12, 1e-12, 0.0, *[L.ptr(t) for t in b2], L.stream()))
            for k, (x, y) in enumerate(zip(a1 + b1, a2 + b2)):
                assert same(x, y), (tile_min, k)
            if first is None:
                first = a1 + b1
            for k, (x, y) in enumerate(zip(first, a1 + b1)):
                assert same(x, y), ("plain against tiled stages", k)
        finally:
            L.debug_set("pt_tile_min", -1)
    assert int((b1[5] >= 0).sum()) > 0 and int((b1[5] < 0).sum()) > 0


def test_pt_primary_from_the_apex(dev, cone):
    """iris_pt_primary (jitter + closest hit in one launch) from a camera at the apex looking down the cone, against ray_intersect along the directions it returns"""
    from iris_amd.utils.path_tracing import jittered_primary_hit, ray_intersect
    H, W, spp = 24, 32, 4
    a, b = np.meshgrid(np.linspace(0.05, 0.95, W), np.linspace(0.05, 0.95, H))
    d = np.stack([np.ones(H * W), a.ravel(), b.ravel()], 1).astype(np.float32)
    o = np.tile(np.array([[0.5, 0.25, 0.25]], np.float32), (H * W, 1))
    dx = np.tile(np.array([[0.0, 0.9 / W, 0.0]], np.float32), (H * W, 1)); dy = np.tile(np.array([[0.0, 0.0, 0.9 / H]], np.float32), (H * W, 1))
    dudv = torch.rand(2, H * W, spp, generator=torch.Generator().manual_seed(1)).to(dev)
    for plain in (False, True):
        if plain:
            with plain_kernels():
                out = jittered_primary_hit(cone["sc"], cone["eml"], T(o, dev), T(d, dev), T(dx, dev), T(dy, dev), dudv)
        else:
            out = jittered_primary_hit(cone["sc"], cone["eml"], T(o, dev), T(d, dev), T(dx, dev), T(dy, dev), dudv)
        p, nr, _, idx, valid = ray_intersect(cone["sc"], T(o, dev).repeat_interleave(spp, 0).contiguous(), out["wi"].contiguous())
        assert same(out["position"], p) and same(out["normal"], nr)
        assert 0.2 < float(valid.float().mean()) < 0.8


# ------------------------------------------------------------------------------------------------ the other kernels that own a stack
@pytest.mark.parametrize("name", ["flat60", "cone60"])
def test_pool_and_label_kernels_on_deep_rays(dev, oracle_mod, name):
    """pool_view_kernel and the two label kernels over explicit rays of a deep scene, latency mode and phase mode: the comparisons of test_prebake_fused.py and
    test_segmentation.py (a host restatement over ray_intersect's hits), and those hits are the oracle's brute force."""
    import segmentation_ref as ref
    from iris_amd.utils.segmentation import label_view, vote_view
    from test_prebake_fused import Host, Sinks, hits_of
    o, d, kind, (_, _, _, ridx, rvalid) = brute(oracle_mod, name)
    n = 1961                                                   # a multiple of neither 64 nor the block size
    sub = ds.mixed_order(kind)[:n]
    rays = torch.cat([T(o[sub], dev), T(d[sub], dev)], -1).contiguous()
    sc = build_scene(name, dev)
    F = sc.n_triangles
    pos, idx, valid = hits_of(sc, rays)
    np.testing.assert_array_equal(idx, ridx[sub]); np.testing.assert_array_equal(valid, rvalid[sub])
    assert 0.3 < valid.mean() < 0.8
    radiance = (np.random.default_rng(2).random((n, 3)) * 3.0).astype(np.float32)
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, 7, n).astype(np.float32)).to(dev)
    table = 301 + np.arange(F)
    want_hist = np.zeros((F, 7), np.int64)
    ref.vote(idx, valid, N(labels), F, 7, want_hist)
    rays12 = torch.cat([rays, torch.full((n, 6), 7.0, device=dev)], -1)

    def run():
        Host(n_tri=F).pool(pos, idx, valid, radiance).check(Sinks(n_tri=F).pool(sc, rays=rays, image=T(radiance, dev)).numpy())
        hist = torch.zeros(F, 7, dtype=torch.int32, device=dev)
        assert vote_view(sc, hist, labels, rays=rays12) is None
        assert np.array_equal(N(hist).astype(np.int64), want_hist)
        got = label_view(sc, torch.from_numpy(table.astype(np.int32)).to(dev), miss=-1, dtype=torch.float32, rays=rays12)
        assert np.array_equal(N(got).astype(np.int64), ref.label_view(idx, valid, table, -1))
    run()
    with plain_kernels():
        run()


def test_spot_stage_on_the_cone(dev, cone):
    """iris_pt_nee_spot (pt_nee_spot_kernel: trace_bvh4, 24 + spill) with a spot at the apex and one beyond the far end, shading points all along the cone: the shadow
    rays towards the far spot run the deep traversal, those towards the apex the shallow one, in the same wave.  The lit / occluded decision against a composition
    of ray_intersect along the same rays, as tests/test_relight.py test_spot_stage_against_float64 makes it, and latency mode against phase mode bit for bit.
    Left out of the composition: points within 1e-4 rad of the cone's boundary, and points whose occluder lies within 1e-5 d of the kernel's limit (1 - 1e-4) d --
    the scene spans ten decades, so the margin is relative; the distance from the float32 hit position carries a relative error near 1e-6."""
    from iris_amd import _lib as L
    from iris_amd.utils.path_tracing import ray_intersect
    n, S = 4097, 2
    rng = np.random.default_rng(9)
    x_hi = 1.5 ** 59
    ax = np.array([1.0, 0.4, 0.4]) / np.linalg.norm([1.0, 0.4, 0.4])
    cut, beam = np.deg2rad(60.0), np.deg2rad(40.0)
    ax2 = np.array([1.0, 0.6, 0.6]) / np.linalg.norm([1.0, 0.6, 0.6])          # (the far spot sits outside the hypotenuses: points with a + b > 1 see it)
    spots = np.array([[0.25, 0.1, 0.1, *ax, cut, beam, np.cos(cut), np.cos(beam)],
                      [1.5 * x_hi, 0.9 * x_hi, 0.9 * x_hi, *(-ax2), cut, beam, np.cos(cut), np.cos(beam)]], np.float32)
    s = np.exp(rng.uniform(np.log(2.0), np.log(x_hi), n))
    pos = (s[:, None] * np.concatenate([np.ones((n, 1)), rng.uniform(0.1, 0.9, (n, 2))], 1)).astype(np.float32)
    nrm = rng.normal(size=(n, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    wo = rng.normal(size=(n, 3)); wo = (wo / np.linalg.norm(wo, axis=1, keepdims=True)).astype(np.float32)
    alb, rough, metal = rng.random((n, 3)).astype(np.float32), (rng.random(n) * 0.9 + 0.05).astype(np.float32), rng.random(n).astype(np.float32)
    pick = rng.random(n).astype(np.float32)
    args = [T(a, dev) for a in (pos, nrm, wo, alb, rough, metal, pick, spots)]

    def run():
        coef = torch.empty(n, 3, device=dev); e = torch.empty(n, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            L.check(L.lib().iris_pt_nee_spot(cone["sc"].handle, *[L.ptr(t) for t in args], S, n, L.ptr(coef), L.ptr(e), L.stream()))
        return coef, e
    coef, e = run()
    with plain_kernels():
        coef_p, e_p = run()
    assert same(coef, coef_p) and torch.equal(e, e_p)
    # the composition
    j = np.clip((pick * np.float32(S)).astype(np.int64), 0, S - 1)
    dlt = spots[j, :3].astype(np.float64) - pos
    d = np.linalg.norm(dlt, axis=1)
    wi = dlt / d[:, None]
    ang = np.arccos(np.clip((-wi * spots[j, 3:6]).sum(1), -1, 1))
    wi32 = T(wi.astype(np.float32), dev)
    o32 = (args[0] + float(RAY_EPS) * wi32).contiguous()
    hp, _, _, _, hv = ray_intersect(cone["sc"], o32, wi32.contiguous())
    dist = np.linalg.norm(N(hp).astype(np.float64) - N(o32), axis=1)
    hv = N(hv)
    limit = (d - RAY_EPS) * (1 - 1e-4)                        # the kernel's rule: an occluder nearer than the light by more than 1e-4 of its distance
    occluded = hv & (dist < limit)
    lit = ~occluded & (ang < cut)
    out = (np.abs(ang - cut) < 1e-4) | (hv & (np.abs(dist - limit) < 1e-5 * d))
    assert out.mean() <= 0.01
    np.testing.assert_array_equal(N(e)[~out], np.where(lit, j, -1)[~out])
    for k in range(S):                                                             # either spot lights some points and is hidden from others
        assert (lit & (j == k)).sum() > 50 and (occluded & (ang < cut) & (j == k)).sum() > 50, k
