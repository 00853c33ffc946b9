"""The trainers' pixel batches on the GPU: iris_pixel_batch (iris_amd/csrc/iris_batch.h) and PixelSet (iris_amd/utils/dataset/pixel_set.py).

Every comparison is torch.equal: the kernel computes the rays with the whole-view kernel's own per-pixel function, decodes 8-bit levels as
np.float32(u / 255.0) and copies everything else; PixelSet adds indexing only.  Three views of 5 x 7 pixels with distinct cameras, as real (K) and
as synthetic (focal) views.  No test here hands the device an id outside [0, 105): tests/test_raygen_ref64.py does (zero rows, segment -1), and asks
the kernel for rows of a view larger than one pass of the whole-view kernel."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as NF

pytestmark = pytest.mark.gpu

H, W, V = 5, 7, 3
HW, N = H * W, H * W * V
ONE_PASS = 4096 * 256          # iris_pixel_batch's launch1d: at most 4096 blocks of 256 threads, then the grid-stride loop
OUTPUTS = ("rays", "rgbs", "int_albedo", "segmentation", "exposure", "positions")


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    f = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(np.asarray(up, np.float64), f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    return np.concatenate([np.stack([r, u, f], 1), np.asarray(eye, np.float64).reshape(3, 1)], 1).astype(np.float32)


def cameras(synthetic):
    """inside the open box of `box_scene`: view 0 looks out of the missing +z face (its outer columns still see the walls), 1 and 2 at walls"""
    poses = [look_at((0.1, -0.05, 0.0), (0.2, 0.1, 1.0)), look_at((-0.3, 0.2, 0.1), (0.4, -0.1, -1.0)), look_at((0.2, 0.1, -0.4), (1.0, 0.3, 0.5))]
    if synthetic:
        return [dict(kind="synthetic", focal=f, c2w=p) for f, p in zip((2.5, 3.25, 4.0), poses)]
    Ks = [np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32) for fx, fy, cx, cy in ((2.5, 2.75, 3.4, 2.6), (3.0, 3.5, 3.5, 2.5), (4.0, 3.75, 3.7, 2.2))]
    return [dict(kind="real", K=K, c2w=p) for K, p in zip(Ks, poses)]


def whole_views(cams, synthetic, ray_diff, dev="cuda"):
    """(N,12) = the concatenated iris_raygen_real / iris_raygen_synthetic outputs of all views (zeros for the differentials without ray_diff)"""
    from iris_amd.utils.dataset import real_ldr, synthetic_ldr
    rows = []
    for cam in cams:
        if synthetic:
            out = synthetic_ldr.get_rays(synthetic_ldr.get_ray_directions(H, W, cam["focal"]), cam["c2w"], focal=cam["focal"] if ray_diff else None, device=dev)
        else:
            out = real_ldr.to_world(real_ldr.get_direction(cam["K"], (H, W)), cam["c2w"], ray_diff, device=dev)
        out = list(out) + [torch.zeros(HW, 3, device=dev)] * (4 - len(out))
        rows.append(torch.cat(out, 1))
    return torch.cat(rows)


def stores(seed=0):
    """host stores of the N pixels: an 8-bit image with all 256 levels, 8-bit albedo, float images, segment ids, per-view exposure, positions"""
    g = np.random.default_rng(seed)
    rgb = g.permutation(np.arange(3 * N) % 256).astype(np.uint8).reshape(N, 3)
    assert len(np.unique(rgb)) == 256
    return dict(rgb=rgb, int_albedo=g.integers(0, 256, (N, 3)).astype(np.uint8), rgb_f=g.normal(size=(N, 3)).astype(np.float32),
                albedo_f=g.random((N, 3)).astype(np.float32), segmentation=g.integers(-5, 2 ** 31 - 1, N).astype(np.int32),
                exposure=(0.5 + g.random(V)).astype(np.float32), positions=g.normal(size=(N, 3)).astype(np.float32))


def pixel_batch(ids, cams, synthetic, ray_diff, st=None, rgb="rgb", albedo="int_albedo", want=OUTPUTS):
    """iris_pixel_batch called directly -> {name: tensor} of the outputs in `want`"""
    from iris_amd import _lib as L
    from iris_amd.utils.dataset.pixel_set import camera_table
    dev = ids.device
    table = torch.from_numpy(camera_table(cams, synthetic)).to(dev)
    d = {k: torch.from_numpy(v).to(dev) for k, v in (st or {}).items()}
    B = ids.shape[0]
    shapes = dict(rays=((B, 12), torch.float32), rgbs=((B, 3), torch.float32), int_albedo=((B, 3), torch.float32), segmentation=((B,), torch.int64),
                  exposure=((B, 1), torch.float32), positions=((B, 3), torch.float32))
    out = {k: torch.full(shapes[k][0], -7, device=dev, dtype=shapes[k][1]) for k in want}
    p = lambda k: L.ptr(out[k]) if k in out else None
    s = lambda k: L.ptr(d[k]) if k in d else None
    L.check(L.lib().iris_pixel_batch(L.ptr(ids) if B else None, B, L.ptr(table), V, H, W, int(ray_diff), int(synthetic), s(rgb), int(rgb == "rgb"), s(albedo),
                                     int(albedo == "int_albedo"), s("segmentation"), s("positions"), s("exposure"), p("rays"), p("rgbs"), p("int_albedo"),
                                     p("segmentation"), p("exposure"), p("positions"), L.stream()))
    return out


def shuffled_ids(seed, extra=20):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randperm(N, generator=g), torch.randint(0, N, (extra,), generator=g)]).cuda()


# ---- the kernel
@pytest.mark.parametrize("ray_diff", [1, 0])
@pytest.mark.parametrize("synthetic", [False, True])
def test_rays_are_the_whole_view_rays(synthetic, ray_diff):
    cams = cameras(synthetic)
    ref = whole_views(cams, synthetic, ray_diff)
    assert ref.shape == (N, 12) and bool(torch.isfinite(ref).all())
    assert len({tuple(r) for r in ref[:, :3].cpu().tolist()}) == V, "three distinct cameras"
    g = torch.Generator().manual_seed(5)
    for ids in (shuffled_ids(1), torch.tensor([N - 1]).cuda(), torch.tensor([0]).cuda(), torch.randint(0, N, (ONE_PASS + 5,), generator=g).cuda()):
        rays = pixel_batch(ids, cams, synthetic, ray_diff, want=("rays",))["rays"]
        assert torch.equal(rays, ref[ids]), ids.shape
    if not ray_diff:
        assert float(ref[:, 6:].abs().max()) == 0.0 and float((ref[:, 3:6].norm(dim=1) - 1).abs().max()) < 1e-6
    empty = pixel_batch(torch.zeros(0, dtype=torch.int64, device="cuda"), cams, synthetic, ray_diff, want=("rays",))["rays"]
    assert empty.shape == (0, 12)
    torch.cuda.synchronize()


@pytest.mark.parametrize("synthetic", [False, True])
def test_stores(synthetic):
    cams, st, ids = cameras(synthetic), stores(), shuffled_ids(2)
    i = ids.cpu()
    out = pixel_batch(ids, cams, synthetic, 1, st)
    assert torch.equal(out["rgbs"].cpu(), torch.from_numpy((st["rgb"] / 255).astype(np.float32))[i])
    assert torch.equal(out["int_albedo"].cpu(), torch.from_numpy((st["int_albedo"] / 255.0).astype(np.float32))[i])
    assert out["segmentation"].dtype == torch.int64 and torch.equal(out["segmentation"].cpu(), torch.from_numpy(st["segmentation"]).long()[i])
    assert out["exposure"].shape == (ids.shape[0], 1) and torch.equal(out["exposure"].cpu(), torch.from_numpy(st["exposure"])[i // HW].reshape(-1, 1))
    assert torch.equal(out["positions"].cpu(), torch.from_numpy(st["positions"])[i])
    assert torch.equal(out["rays"], whole_views(cams, synthetic, 1)[ids])
    # float32 stores pass through bit for bit
    f = pixel_batch(ids, cams, synthetic, 1, st, rgb="rgb_f", albedo="albedo_f", want=("rgbs", "int_albedo"))
    assert torch.equal(f["rgbs"].cpu().view(torch.int32), torch.from_numpy(st["rgb_f"])[i].view(torch.int32))
    assert torch.equal(f["int_albedo"].cpu().view(torch.int32), torch.from_numpy(st["albedo_f"])[i].view(torch.int32))
    # every combination of outputs: what is asked for is what the full call gives
    for k in range(len(OUTPUTS) + 1):
        for want in itertools.combinations(OUTPUTS, k):
            part = pixel_batch(ids, cams, synthetic, 1, st, want=want)
            assert set(part) == set(want) and all(torch.equal(part[n], out[n]) for n in want), want


def test_output_without_its_store_is_an_error():
    from iris_amd import _lib as L
    with pytest.raises(L.IrisError):
        pixel_batch(shuffled_ids(3), cameras(False), False, 1, st=None, want=("rays", "rgbs"))


# ---- PixelSet
def box_scene(dev="cuda"):
    """the cube [-1, 1]^3 without its +z face: rays through the opening miss"""
    from iris_amd.utils.path_tracing import Scene
    v = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float32)
    quads = [(0, 1, 3, 2), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]          # -z, -y, +y, -x, +x
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return Scene(v, f, device=dev)


def make_set(synthetic, batch_size, st, **kw):
    from iris_amd.utils.dataset import PixelSet
    per_view = [st["rgb"][v * HW:(v + 1) * HW].reshape(H, W, 3) for v in range(V)]                    # one array per view / one tensor for all: both forms
    return PixelSet(cameras(synthetic), (H, W), per_view, segmentation=torch.from_numpy(st["segmentation"]).cuda(), int_albedo=st["int_albedo"],
                    exposure=st["exposure"], synthetic=synthetic, batch_size=batch_size, device="cuda", **kw)


@pytest.mark.parametrize("synthetic", [False, True])
def test_valid_list(synthetic):
    from iris_amd.utils.path_tracing import ray_intersect
    st, scene = stores(), box_scene()
    ps = make_set(synthetic, 16, st)
    assert ps.rgb.dtype == torch.uint8 and ps.int_albedo.dtype == torch.uint8 and ps.segmentation.dtype == torch.int32
    assert len(ps) == -(-N // 16) and sorted(torch.cat([ps[i]["idx"] for i in range(len(ps))]).tolist()) == list(range(N))
    ref = whole_views(cameras(synthetic), synthetic, 1)
    want = torch.cat([ray_intersect(scene, ref[v * HW:(v + 1) * HW, :3].contiguous(), NF.normalize(ref[v * HW:(v + 1) * HW, 3:6], dim=-1))[4].nonzero().reshape(-1) + v * HW
                      for v in range(V)])
    n = ps.restrict_to_hits(scene, store_positions=True)
    print(f"synthetic {synthetic}: {n} of {N} pixels hit the open box")
    assert 0 < n < N and n == want.shape[0] and torch.equal(ps.kept, want)
    assert len(ps) == -(-n // 16)
    gen = torch.Generator(device="cuda").manual_seed(11)
    ps.resample(gen)
    batches = [ps[i] for i in range(len(ps))]
    assert [b["idx"].shape[0] for b in batches] == [16] * (n // 16) + ([n % 16] if n % 16 else [])
    assert torch.equal(torch.cat([b["idx"] for b in batches]).sort().values, want), "each kept id once per epoch"
    first = batches[0]["idx"].clone()
    ps.resample(gen)
    assert not torch.equal(ps[0]["idx"], first)
    for b in batches:
        assert set(b) == {"rays", "rgbs", "segmentation", "int_albedo", "exposure", "idx", "positions"}
        assert torch.equal(b["rays"], ref[b["idx"]])
        pos, _, _, _, valid = ray_intersect(scene, b["rays"][:, :3].contiguous(), NF.normalize(b["rays"][:, 3:6], dim=-1))
        assert bool(valid.all()) and torch.equal(b["positions"], pos)
        i = b["idx"].cpu()
        assert torch.equal(b["rgbs"].cpu(), torch.from_numpy((st["rgb"] / 255).astype(np.float32))[i])
        assert torch.equal(b["exposure"].cpu(), torch.from_numpy(st["exposure"])[i // HW].reshape(-1, 1))
    with pytest.raises(IndexError):
        ps[len(ps)]
    with pytest.raises(ValueError):
        ps.set_order(torch.tensor([0, N]))                 # refused on the host: nothing is launched


def test_materialised_cache_and_set_order():
    from iris_amd.utils.shading_cache import ShadingCache
    st = stores()
    ps = make_set(False, 50, st, materialise_cache=True)
    cache = ShadingCache(N)
    cache.rows.copy_(torch.rand(cache.rows.shape, generator=torch.Generator().manual_seed(4)))
    ps.attach_cache(cache)
    ids = shuffled_ids(6)
    ps.set_order(ids.cpu().numpy())
    assert len(ps) == 3
    got = [ps[i] for i in range(3)]
    assert torch.equal(torch.cat([b["idx"] for b in got]), ids) and got[2]["idx"].shape[0] == ids.shape[0] - 100
    for b in got:
        for name, want in zip(("diffuse", "specular0", "specular1"), cache.gather(b["idx"])):
            assert torch.equal(b[name], want)
        assert "positions" not in b
    with pytest.raises(ValueError):
        ps.attach_cache(ShadingCache(N - 1))


def step_loss(batch, cache, crf):
    from iris_amd.utils.losses import brdf_crf_loss
    from stub_material import StubMaterial
    m = StubMaterial()(batch["positions"])
    leaf = torch.cat([m["albedo"], m["roughness"], m["metallic"]], 1).requires_grad_(True)
    out = brdf_crf_loss(dict(albedo=leaf[:, :3], roughness=leaf[:, 3:4], metallic=leaf[:, 4:5]), cache=cache, idx=batch["idx"], crf=crf,
                        exposure=batch["exposure"], rgbs_gt=batch["rgbs"], segmentation=batch["segmentation"], positions=batch["positions"],
                        albedo_prior=batch["int_albedo"], has_part=1, la=0.01, seed=3)
    crf.weight.grad = None
    out["loss"].backward()
    return out["loss"].detach(), leaf.grad, crf.weight.grad.clone()


def test_step():
    """one brdf_crf_loss forward and backward on a PixelSet batch = the same step on a batch indexed out of float tables with plain torch"""
    from iris_amd.model.crf import EmorCRF
    from iris_amd.utils.path_tracing import ray_intersect
    from iris_amd.utils.shading_cache import ShadingCache
    st, scene = stores(), box_scene()
    st["segmentation"] = (np.arange(N) % 4 * 3 + 7).astype(np.int32)
    ps = make_set(False, 32, st)
    g = torch.Generator().manual_seed(8)
    cache = ShadingCache(N)
    cache.rows.copy_(torch.rand(cache.rows.shape, generator=g))
    ps.attach_cache(cache)
    n = ps.restrict_to_hits(scene, store_positions=True)
    assert n >= 32
    order = ps.kept[torch.randperm(n, generator=g).cuda()]
    s = torch.linspace(0, 1, 64)
    crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (j + 1)) * 0.05 for j in range(3)])).cuda()
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))

    ps.set_order(order)
    loss, g_leaf, g_w = step_loss(ps[0], cache, crf)
    assert bool(torch.isfinite(loss)) and float(loss) > 0 and bool(torch.isfinite(g_leaf).all()) and float(g_leaf.abs().max()) > 0 and float(g_w.abs().max()) > 0

    idx = order[:32]
    ref = whole_views(cameras(False), False, 1)
    plain = dict(idx=idx, rgbs=torch.from_numpy((st["rgb"] / 255.0).astype(np.float32)).cuda()[idx],
                 int_albedo=torch.from_numpy((st["int_albedo"] / 255.0).astype(np.float32)).cuda()[idx],
                 segmentation=torch.from_numpy(st["segmentation"]).cuda().long()[idx], exposure=torch.from_numpy(st["exposure"]).cuda()[idx // HW].reshape(-1, 1),
                 positions=ray_intersect(scene, ref[:, :3].contiguous(), NF.normalize(ref[:, 3:6], dim=-1))[0][idx])
    loss_plain, g_plain, _ = step_loss(plain, cache, crf)
    print(f"step: loss {float(loss):.9g}, from plain indexing {float(loss_plain):.9g}")
    assert torch.equal(loss.view(torch.int32), loss_plain.view(torch.int32)) and torch.equal(g_leaf, g_plain)

    ps.set_order(order)
    again = step_loss(ps[0], cache, crf)
    assert torch.equal(loss.view(torch.int32), again[0].view(torch.int32)) and torch.equal(g_leaf, again[1])
