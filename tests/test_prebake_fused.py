"""The fused view-pooling kernel (iris_amd/csrc/iris_prebake.h, utils/gbuffer.py pool_view) and the pre-bake functions over it, on the box scene of
tests/golden/bake_box.npz (a closed 4 x 3 x 2.6 room, z up, with a light quad under its ceiling: triangles 2, 3 are the ceiling, 12, 13 the light).

Every expectation is a host restatement over ray_intersect's hits: counts, histogram, mask, indices and bounds exact; pooled float means within the
project's tolerance for sums of float atomics (tests/test_prebake.py: rtol 2e-5, atol 1e-6)."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 1e-6
RES, VMIN, VMAX = 24, -0.3, 4.3
CEILING_AND_LIGHT = (2, 3, 12, 13)


def dev():
    return torch.device("cuda:0")


def look(eye, fwd, H, W, up=(0.0, 0.0, 1.0)):
    """a `real` view dict with tools.synth.camera's intrinsics (f = 0.8 W), looking along fwd"""
    fwd = np.asarray(fwd, np.float64) / np.linalg.norm(fwd)
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    K = np.array([[0.8 * W, 0, W / 2.0], [0, 0.8 * W, H / 2.0], [0, 0, 1]], np.float32)
    return {"kind": "real", "K": K, "c2w": np.concatenate([np.stack([right, down, fwd], 1), np.asarray(eye, np.float64)[:, None]], 1).astype(np.float32)}


def synth_view(kind, H, W, v, n=3):
    from tools import synth
    K, c2w = synth.camera(H, W, v, n_views=n)
    return {"kind": "real", "K": K, "c2w": c2w} if kind == "real" else {"kind": "synthetic", "focal": float(K[0, 0]), "c2w": c2w}


@pytest.fixture(scope="module")
def box():
    from iris_amd.utils.path_tracing import Scene
    g = golden("bake_box.npz")
    return Scene(g["verts"], g["faces"], device=dev())


@pytest.fixture(scope="module")
def open_box():
    from iris_amd.utils.path_tracing import Scene
    g = golden("bake_box.npz")
    return Scene(g["verts"], g["faces"][[i for i in range(len(g["faces"])) if i not in CEILING_AND_LIGHT]], device=dev())


def make_crf():
    from iris_amd.model.crf import EmorCRF
    s = torch.linspace(0, 1, 64)
    crf = EmorCRF.from_arrays(s ** 0.45, torch.stack([torch.sin(3.14159 * s * (j + 1)) * 0.05 for j in range(3)]))
    with torch.no_grad():
        crf.weight.copy_(torch.tensor([[0.3, -0.2, 0.1], [0.0, 0.1, 0.0], [-0.1, 0.2, 0.3]]))
    return crf.to(dev())


def rays_of(view, hw):
    from iris_amd.utils import cameras
    return torch.cat(cameras.view_rays(view, hw, dev()), -1)


def hits_of(scene, rays):
    from iris_amd.utils.path_tracing import ray_intersect
    pos, _, _, idx, valid = ray_intersect(scene, rays[:, :3].contiguous(), rays[:, 3:6].contiguous())
    return pos.cpu().numpy(), idx.cpu().numpy(), valid.cpu().numpy()


def voxel_of(P, vmin=VMIN, vmax=VMAX, res=RES):
    """voxel_coord on the host, in float32 as the kernel: ((p - vmin) / (vmax - vmin) * H) truncated and clamped -> (x, y, z) indices"""
    q = (P - np.float32(vmin)) / np.float32(vmax - vmin) * np.float32(res)
    return q.astype(np.int64).clip(0, res - 1)


def full_slf(mask=None):
    from iris_amd.model.slf import VoxelSLF
    mask = torch.ones(RES, RES, RES, dtype=torch.bool) if mask is None else mask
    return VoxelSLF(mask.to(dev()), VMIN, VMAX)


class Sinks:
    """all four sinks of pool_view, fresh"""

    def __init__(self, n_tri=14, mask=None):
        d = dev()
        self.bounds = torch.tensor([1000.0, 0.0], device=d)
        self.hist = torch.zeros(RES, RES, RES, device=d)
        self.vslf = full_slf(mask)
        self.tri_sum, self.tri_count = torch.zeros(n_tri, 3, device=d), torch.zeros(n_tri, device=d)

    def pool(self, scene, **kw):
        from iris_amd.utils.gbuffer import pool_view
        assert pool_view(scene, bounds=self.bounds, hist=self.hist, voxel_range=(VMIN, VMAX), vslf=self.vslf, tri_sum=self.tri_sum, tri_count=self.tri_count, **kw) is None
        return self

    def numpy(self):
        return {k: getattr(self, k).cpu().numpy() for k in ("bounds", "hist", "tri_sum", "tri_count")} | \
               {"v_sum": self.vslf.radiance.cpu().numpy(), "v_count": self.vslf.count.cpu().numpy()}


def mean(total, count):
    return total / np.maximum(count, 1)[:, None]


class Host:
    """the same pooling restated on the host in float64 (np.add.at), over ray_intersect's hits"""

    def __init__(self, n_tri=14, inds=None):
        self.inds = np.arange(RES ** 3).reshape(RES, RES, RES) if inds is None else inds
        n_rows = int(self.inds.max()) + 1
        self.lo, self.hi = np.float32(1000.0), np.float32(0.0)
        self.hist = np.zeros((RES, RES, RES), np.float64)
        self.v_sum, self.v_count = np.zeros((n_rows, 3), np.float64), np.zeros(n_rows, np.int64)
        self.tri_sum, self.tri_count = np.zeros((n_tri, 3), np.float64), np.zeros(n_tri, np.float64)

    def pool(self, pos, idx, valid, radiance):
        P, T, R = pos[valid], idx[valid], np.asarray(radiance, np.float64).reshape(-1, 3)[valid]
        if len(P):
            self.lo, self.hi = min(self.lo, P.min()), max(self.hi, P.max())
        q = voxel_of(P)
        np.add.at(self.hist, (q[:, 2], q[:, 1], q[:, 0]), 1)
        row = self.inds[q[:, 2], q[:, 1], q[:, 0]]
        np.add.at(self.v_sum, row[row >= 0], R[row >= 0]); np.add.at(self.v_count, row[row >= 0], 1)
        np.add.at(self.tri_sum, T, R); np.add.at(self.tri_count, T, 1)
        return self

    def check(self, got):
        assert got["bounds"][0] == self.lo and got["bounds"][1] == self.hi, (got["bounds"], self.lo, self.hi)
        np.testing.assert_array_equal(got["hist"], self.hist)
        np.testing.assert_array_equal(got["v_count"], self.v_count)
        np.testing.assert_array_equal(got["tri_count"], self.tri_count)
        np.testing.assert_allclose(mean(got["v_sum"], got["v_count"]), mean(self.v_sum, self.v_count), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(mean(got["tri_sum"], got["tri_count"]), mean(self.tri_sum, self.tri_count), rtol=RTOL, atol=ATOL)


def photo(hw, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (hw[0], hw[1], 3)).astype(np.uint8))


def decode(u8):
    """np.float32(u / 255.0), the reference's 8-bit decode"""
    return torch.from_numpy((u8.numpy().astype(np.float64) / 255.0).astype(np.float32))


@pytest.mark.parametrize("kind", ["real", "synthetic"])
def test_camera_path_equals_explicit_ray_path(box, kind):
    hw, crf = (48, 64), make_crf()
    tables = (crf.grid, crf.get_inv_crf())
    a, b = Sinks(), Sinks()
    for v in range(2):
        view, img = synth_view(kind, *hw, v), photo(hw, v).to(dev())
        a.pool(box, camera=view, img_hw=hw, image=img, crf_tables=tables, exposure=0.7 + v)
        b.pool(box, rays=rays_of(view, hw), image=img.reshape(-1, 3), crf_tables=tables, exposure=0.7 + v)
    a, b = a.numpy(), b.numpy()
    assert a["hist"].sum() == 2 * hw[0] * hw[1]                                  # closed room: every pixel hits
    for k in ("bounds", "hist", "v_count", "tri_count"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_allclose(mean(a["v_sum"], a["v_count"]), mean(b["v_sum"], b["v_count"]), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(mean(a["tri_sum"], a["tri_count"]), mean(b["tri_sum"], b["tri_count"]), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("case", ["u8_crf", "f32_linear", "u8_crf_exposure_per_pixel"])
def test_against_float64_host_restatement(box, case):
    hw = (48, 64)
    n = hw[0] * hw[1]
    crf = make_crf() if case != "f32_linear" else None
    got, want = Sinks(), Host()
    for v in range(2):
        view = synth_view("real", *hw, v)
        if case == "f32_linear":
            image = torch.from_numpy(np.random.default_rng(v).random((n, 3)).astype(np.float32) * 3.0)
            radiance, kw = image, {}
        else:
            image = photo(hw, 10 + v)
            exposure = 0.6 + 0.3 * v if case == "u8_crf" else torch.from_numpy(np.random.default_rng(5 + v).uniform(0.5, 2.0, n).astype(np.float32)).to(dev())
            radiance = crf.inverse(decode(image).reshape(-1, 3).to(dev()), exposure).cpu()          # the existing per-pixel inverse on u / 255
            kw = {"crf_tables": (crf.grid, crf.get_inv_crf()), "exposure": exposure}
        got.pool(box, camera=view, img_hw=hw, image=image.to(dev()), **kw)
        want.pool(*hits_of(box, rays_of(view, hw)), radiance.numpy())
    want.check(got.numpy())
    assert (want.v_count > 1).any() and want.tri_count.max() > 64                # rows that really accumulate


def test_per_lane_atomics_arm_pools_the_same(box):
    """iris_debug_set('pool_combine', 0), the comparison arm of tools/bench_prebake.py: one set of atomics per hit instead of one per distinct destination of a wave"""
    from iris_amd import _lib as L
    hw = (37, 53)
    view, image = synth_view("real", *hw, 0), photo(hw, 9)
    want = Host().pool(*hits_of(box, rays_of(view, hw)), decode(image).reshape(-1, 3).numpy())
    combined = Sinks().pool(box, camera=view, img_hw=hw, image=image.to(dev())).numpy()
    L.debug_set("pool_combine", 0)
    try:
        per_lane = Sinks().pool(box, camera=view, img_hw=hw, image=image.to(dev())).numpy()
    finally:
        L.debug_set("pool_combine", -1)
    want.check(combined)
    want.check(per_lane)


def test_misses_contribute_to_nothing(open_box):
    hw = (48, 64)
    tilted = look((2.0, 1.5, 1.3), (0.8, 0.6, 0.9), *hw)                         # from inside, partly up through the missing ceiling
    pos, idx, valid = hits_of(open_box, rays_of(tilted, hw))
    assert 0.1 < valid.mean() < 0.9, valid.mean()
    image = torch.from_numpy(np.random.default_rng(1).random((hw[0] * hw[1], 3)).astype(np.float32))
    got = Sinks(n_tri=10).pool(open_box, camera=tilted, img_hw=hw, image=image.to(dev()))
    want = Host(n_tri=10).pool(pos, idx, valid, image.numpy())
    g = got.numpy()
    assert g["hist"].sum() == g["v_count"].sum() == g["tri_count"].sum() == valid.sum()
    assert g["bounds"][0] == pos[valid].min() and g["bounds"][1] == pos[valid].max()
    want.check(g)
    # a view that sees nothing: straight up through the hole
    nothing = look((2.0, 1.5, 2.0), (0.0, 0.0, 1.0), *hw, up=(0.0, 1.0, 0.0))
    assert not hits_of(open_box, rays_of(nothing, hw))[2].any()
    got.pool(open_box, camera=nothing, img_hw=hw, image=image.to(dev()))
    after = got.numpy()
    for k in g:
        np.testing.assert_array_equal(after[k], g[k], err_msg=k)
    fresh = Sinks(n_tri=10).pool(open_box, camera=nothing, img_hw=hw, image=image.to(dev())).numpy()
    assert fresh["bounds"].tolist() == [1000.0, 0.0] and fresh["hist"].sum() == 0 and fresh["v_count"].sum() == 0 and not fresh["tri_sum"].any()


def test_contention_is_exact(box):
    """every hit of the view in ONE voxel and on ONE triangle, radiance whose sums are exact in float32 in any order"""
    from iris_amd.model.slf import VoxelSLF
    from iris_amd.utils.gbuffer import pool_view
    hw = (37, 53)
    n = hw[0] * hw[1]
    down = look((3.0, 0.8, 0.5), (0.0, 0.0, -1.0), *hw, up=(0.0, 1.0, 0.0))       # close above the floor, away from its diagonal
    _, idx, valid = hits_of(box, rays_of(down, hw))
    assert valid.all() and (idx == 0).all()
    value = torch.tensor([0.5, 0.25, 0.125])
    image = value.expand(n, 3).contiguous().to(dev())
    vslf = VoxelSLF(torch.ones(1, 1, 1, dtype=torch.bool, device=dev()), -1.0, 5.0)
    tri_sum, tri_count = torch.zeros(14, 3, device=dev()), torch.zeros(14, device=dev())
    pool_view(box, camera=down, img_hw=hw, image=image, vslf=vslf, tri_sum=tri_sum, tri_count=tri_count)
    exact = (value * n).view(torch.int32)
    assert int(vslf.count[0]) == n and float(tri_count[0]) == n and float(tri_count.sum()) == n
    assert torch.equal(vslf.radiance[0].cpu().view(torch.int32), exact) and torch.equal(tri_sum[0].cpu().view(torch.int32), exact)


@pytest.mark.parametrize("hw", [(37, 53), (1, 1), (64, 1)])
def test_view_shapes(box, hw):
    view = synth_view("real", *hw, 1)
    image = photo(hw, 3)
    got = Sinks().pool(box, camera=view, img_hw=hw, image=image.to(dev()))
    Host().pool(*hits_of(box, rays_of(view, hw)), decode(image).reshape(-1, 3).numpy()).check(got.numpy())


def test_empty_ray_batch_is_a_no_op(box):
    got = Sinks().pool(box, rays=torch.empty(0, 6, device=dev()), image=torch.empty(0, 3, device=dev())).numpy()
    assert got["bounds"].tolist() == [1000.0, 0.0]
    assert not got["hist"].any() and not got["v_count"].any() and not got["tri_sum"].any() and not got["tri_count"].any()


def test_a_camera_without_an_image_size_is_refused(box):
    from iris_amd._lib import IrisError
    from iris_amd.utils.gbuffer import pool_view
    with pytest.raises(IrisError):
        pool_view(box, camera=synth_view("real", 37, 53, 1))


def test_hits_in_an_empty_voxel_are_dropped(box):
    hw = (48, 64)
    view = synth_view("real", *hw, 0)
    pos, idx, valid = hits_of(box, rays_of(view, hw))
    q = voxel_of(pos[valid])
    seen = np.zeros((RES, RES, RES), bool); seen[q[:, 2], q[:, 1], q[:, 0]] = True
    kk, jj, ii = np.where(seen)
    mask = seen.copy(); mask[kk[::3], jj[::3], ii[::3]] = False                   # every third seen voxel leaves the grid
    inds = -np.ones(mask.shape, np.int64); inds[np.where(mask)] = np.arange(mask.sum())
    image = photo(hw, 4)
    got = Sinks(mask=torch.from_numpy(mask)).pool(box, camera=view, img_hw=hw, image=image.to(dev())).numpy()
    want = Host(inds=inds).pool(pos, idx, valid, decode(image).reshape(-1, 3).numpy())
    dropped = int(valid.sum() - want.v_count.sum())
    assert 0 < dropped < valid.sum() and got["v_count"].sum() == valid.sum() - dropped
    want.check(got)


def test_bake_slf_on_camera_batches(box, tmp_path):
    from iris_amd import slf_bake as sb
    from iris_amd.model.emitter import SLFEmitter
    g = golden("bake_box.npz")
    hw, crf = (48, 64), make_crf()
    views = [synth_view("real", *hw, v) for v in range(3)] + [look((2.0, 1.5, 1.0), (0.1, 0.05, 1.0), *hw)]      # the last one looks up at the light
    cam_batches, ray_batches = [], []
    for v, view in enumerate(views):
        rays = rays_of(view, hw)
        _, idx, _ = hits_of(box, rays)
        image = photo(hw, 20 + v).numpy().reshape(-1, 3) // 2                    # at most 127 / 255 ...
        image[idx >= 12] = 250                                                   # ... except on the light quad
        image = torch.from_numpy(image.reshape(*hw, 3))
        cam_batches.append({"camera": view, "img_hw": hw, "image": image, "exposure": 0.5 + 0.25 * v})
        ray_batches.append({"rays": rays, "rgbs": decode(image).reshape(-1, 3), "exposure": 0.5 + 0.25 * v})
    a = sb.bake_slf(box, cam_batches, res_spatial=RES, dataset="real", device=dev(), crf=crf)
    b = sb.bake_slf(box, ray_batches, res_spatial=RES, dataset="real", device=dev(), crf=crf)
    assert a["voxel_min"] == b["voxel_min"] and a["voxel_max"] == b["voxel_max"]
    assert torch.equal(a["mask"], b["mask"]) and int(a["mask"].sum()) > 100
    assert torch.equal(a["weight"]["inds"], b["weight"]["inds"]) and torch.equal(a["weight"]["count"], b["weight"]["count"])
    assert int(a["weight"]["count"].sum()) == len(views) * hw[0] * hw[1]
    np.testing.assert_allclose(a["weight"]["radiance"].numpy(), b["weight"]["radiance"].numpy(), rtol=RTOL, atol=ATOL)
    em = sb.extract_emitters(box, g["verts"], g["faces"], cam_batches, threshold=0.9, device=dev())          # the raw 8-bit values: 250 / 255 > 0.9
    np.testing.assert_array_equal(em["is_emitter"].numpy(), g["is_emitter"])
    ep, sp = str(tmp_path / "emitter.pth"), str(tmp_path / "vslf.npz")
    torch.save(em, ep); torch.save(a, sp)
    emitter = SLFEmitter(ep, sp)
    assert emitter is not None
