"""The texture export stage on the GPU (iris_amd/csrc/iris_texture.h, iris_amd/utils/texture.py, python -m iris_amd.utils.export), bit for bit against the
numpy restatement of its contract (tests/uv_raster_ref.py): ids and mask as integers, bary and xyz by their bit patterns."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import golden
from stub_material import StubMaterial, stub_material_np
import uv_raster_ref as R
from test_texture_cpu import case_square_split, case_triangles_on_centres, centres, corners, decode_png

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _mesh_for(ft, seed=0):
    """a 3-D mesh to interpolate: one random vertex per UV vertex, f = ft"""
    n = int(np.max(ft)) + 1 if np.size(ft) else 1
    return (np.random.default_rng(seed).standard_normal((n, 3)) * 2).astype(np.float32), np.asarray(ft, np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check_against_reference(vt, ft, tex_res, ref=None, modes=(None,)):
    """rasterize_uv == the reference in every output; every raster mode gives the same ids.  -> the reference"""
    from iris_amd.utils import texture as T
    v, f = _mesh_for(ft)
    ref = ref or R.rasterize_uv_ref(vt, ft, v, f, tex_res)
    out = {k: t.cpu().numpy() for k, t in T.rasterize_uv(vt, ft, v, f, tex_res, device=DEV).items()}
    assert out["ids"].dtype == np.int32 and out["mask"].dtype == bool
    assert np.array_equal(out["ids"], ref["ids"]), np.argwhere(out["ids"] != ref["ids"])[:8]
    assert np.array_equal(out["mask"], ref["mask"])
    assert np.array_equal(bits(out["bary"]), bits(ref["bary"]))
    assert np.array_equal(bits(out["xyz"]), bits(ref["xyz"]))
    m = T.UVMesh(vt, ft, v, f, tex_res, device=DEV)
    for mode in modes:
        if mode is not None:
            assert np.array_equal(m.raster(mode).cpu().numpy(), ref["ids"]), mode
    return ref


ALL_MODES = (None, 0, 1, 2, 64)          # iris_uv_raster; iris_debug_uv_raster: default, all small, all large, a class threshold of 64 texels


# ------------------------------------------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("case", [case_triangles_on_centres, case_square_split])
def test_tie_cases(case):
    vt, ft, want = case()
    ref = check_against_reference(vt, ft, 8, modes=ALL_MODES)
    assert np.array_equal(ref["ids"], want)


# --------------------------------------------------------------------------------------------------------------------------------- overlap
def _two_overlapping():
    vt = np.concatenate([corners([(0.5, 0.5), (7.5, 1.0), (1.0, 7.5)]), corners([(7.6, 7.7), (0.2, 6.0), (6.0, 0.3)])])
    return vt, np.arange(6, dtype=np.int32).reshape(2, 3)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
@pytest.mark.parametrize("copies", [0, 500])
def test_overlap_lowest_index_wins(order, copies):
    vt, ft = _two_overlapping()
    ft = np.concatenate([ft[list(order)]] + [ft] * copies)          # the two, then `copies` copies of each: contended atomicMin
    ref = check_against_reference(vt, ft, 8, modes=ALL_MODES)
    both = R.coverage(vt, ft[:2], 8)[0] == 2
    assert both.sum() >= 8 and (ref["ids"][both] == 0).all()          # they do overlap, and face 0 -- whichever triangle that is -- owns the overlap
    assert ref["ids"].max() <= 1


# ------------------------------------------------------------------------------------------------------------------------- coverage extremes
def test_coverage_extremes():
    # zero area (collinear, and a repeated vertex); a sliver thinner than a texel between two columns of centres: nothing
    vt = np.concatenate([corners([(1, 1), (4, 4), (6, 6)]), corners([(2, 2), (2, 2), (5, 3)]), corners([(3.1, 0.2), (3.4, 0.2), (3.25, 7.9)])])
    ft = np.arange(9, dtype=np.int32).reshape(3, 3)
    ref = check_against_reference(vt, ft, 8, modes=ALL_MODES)
    assert not ref["mask"].any()
    # wholly outside [0, 1]^2, on each side and far off
    vt = np.concatenate([corners([(9, 1), (15, 2), (10, 7)]), corners([(-7, 1), (-1, 2), (-3, 7)]), corners([(1, 9), (5, 16), (2, 12)]), corners([(1, -8), (5, -1), (2, -3)])])
    ft = np.arange(12, dtype=np.int32).reshape(4, 3)
    ref = check_against_reference(vt, ft, 8, modes=ALL_MODES)
    assert not ref["mask"].any()
    # partly outside: one case per side, and one that sticks out on all four (UVs within [-1, 2])
    for tri in ([(-3, 2), (4, 1), (3, 6)], [(4, 2), (13, 1), (5, 6)], [(2, -5), (6, 3), (1, 4)], [(2, 4), (6, 3), (5, 15)], [(-8, -8), (16, -7.5), (-7, 16)]):
        vt = corners(tri)
        ref = check_against_reference(vt, np.int32([[0, 1, 2]]), 8, modes=ALL_MODES)
        assert ref["mask"].any() and not ref["mask"].all()
    ref = check_against_reference(corners([(-8, -8), (16, -8), (-8, 16)]), np.int32([[0, 1, 2]]), 8, modes=ALL_MODES)
    assert ref["mask"].sum() == 36 - 8                                # the half below the anti-diagonal c + r + 1 < 8: the diagonal's 8 centres are dropped
    # A < 0 and its mirror image: the same coverage
    tri = [(0.7, 0.9), (7.2, 2.1), (2.6, 7.4)]
    a = check_against_reference(corners(tri), np.int32([[0, 1, 2]]), 8, modes=ALL_MODES)
    b = check_against_reference(corners(tri), np.int32([[0, 2, 1]]), 8, modes=ALL_MODES)
    assert a["mask"].sum() >= 10 and np.array_equal(a["mask"], b["mask"])
    mirrored = check_against_reference(corners([(8 - x, y) for x, y in tri]), np.int32([[0, 1, 2]]), 8, modes=ALL_MODES)
    assert np.array_equal(mirrored["mask"], a["mask"][:, ::-1])       # (no centre of this triangle lies on an edge: the tie rule does not enter)


# ------------------------------------------------------------------------------------------------------------------------------ random soup
SOUP_HW = (48, 64)


@functools.lru_cache(None)
def soup():
    """2 000 triangles at 48 rows x 64 columns; about a tenth of the vertices exactly on texel centres or on the 1 / 256 grid's half-way points (in u, where
    W = 64 makes them exact in float32; in v they land beside them).  The reference covers 54.9 % of the texels with seed 11, 19 % of them more than once (asserted in the test)."""
    H, W = SOUP_HW
    rng = np.random.default_rng(11)
    n = 2000
    centre = rng.uniform(-0.05, 1.05, (n, 1, 2))
    vt = centre + rng.uniform(-1.0, 1.0, (n, 3, 2)) * np.array([2.2 / W, 2.2 / H])
    kind = rng.uniform(size=(n, 3))
    on_centre = (np.floor(vt * [W, H]) + 0.5) / [W, H]
    half_way = (np.floor(vt * [W * 256, H * 256]) + 0.5) / [W * 256, H * 256]
    vt = np.where((kind < 0.05)[..., None], on_centre, np.where((kind > 0.95)[..., None], half_way, vt))
    vt = np.clip(vt, -1, 2).reshape(-1, 2).astype(np.float32)
    ft = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    v, f = _mesh_for(ft)
    return vt, ft, R.rasterize_uv_ref(vt, ft, v, f, SOUP_HW)


def test_random_soup():
    vt, ft, ref = soup()
    share = ref["mask"].mean()
    print("soup coverage: %.3f" % share)
    assert 0.20 <= share <= 0.95, share                               # two empty (or two full) maps would compare equal and show nothing
    assert (ref["count"] >= 2).mean() > 0.1                           # and the overlap rule is exercised
    check_against_reference(vt, ft, SOUP_HW, ref=ref, modes=ALL_MODES)


# ----------------------------------------------------------------------------------------------------------------------------- both classes
def test_both_classes_agree():
    """37 x 70: ragged against a 64-texel row segment (one full segment and 6 texels per row).  Two triangles that cover the texture whole (the large class by
    default) plus 300 small ones in front of them (lower indices)."""
    H, W = 37, 70
    rng = np.random.default_rng(4)
    small = rng.uniform(0, 1, (300, 1, 2)) + rng.uniform(-1, 1, (300, 3, 2)) * np.array([2.5 / W, 2.5 / H])
    walls = np.array([[(-0.5, -0.5), (1.5, -0.5), (1.5, 1.5)], [(-0.5, -0.5), (1.5, 1.5), (-0.5, 1.5)]])
    vt = np.concatenate([small, walls]).reshape(-1, 2).astype(np.float32)
    ft = np.arange(vt.shape[0], dtype=np.int32).reshape(-1, 3)
    ref = check_against_reference(vt, ft, (H, W), modes=ALL_MODES)
    assert ref["mask"].all() and (ref["ids"] >= 300).mean() > 0.3 and (ref["ids"] < 300).mean() > 0.1          # (0.81 and 0.19)


# -------------------------------------------------------------------------------------------------------------------------- resolve on ranges
def test_resolve_on_ranges():
    from iris_amd.utils import texture as T
    vt, ft, ref = soup()
    v, f = _mesh_for(ft)
    m = T.UVMesh(vt, ft, v, f, SOUP_HW, device=DEV)
    ids = m.raster()
    bary, xyz = m.resolve(ids)
    n = SOUP_HW[0] * SOUP_HW[1]
    parts = [m.resolve(ids, t0, min(1000, n - t0)) for t0 in range(0, n, 1000)]          # 3 x 1000 + 72
    assert parts[-1][1].shape[0] == 72
    assert torch.equal(torch.cat([p[0] for p in parts]).view(torch.int32), bary.view(torch.int32))
    assert torch.equal(torch.cat([p[1] for p in parts]).view(torch.int32), xyz.view(torch.int32))
    assert np.array_equal(bits(xyz.cpu().numpy()).reshape(-1), bits(ref["xyz"]).reshape(-1))
    assert m.resolve(ids, 5, 7, bary=False)[0] is None
    with pytest.raises(T.L.IrisError):
        m.resolve(ids, n - 3, 4)


# --------------------------------------------------------------------------------------------------------------------------------- quantise
def test_quantize():
    from iris_amd.utils import texture as T
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    x = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), np.float32([0, 1, -0.0, 1.5, -1, np.nan])]).astype(np.float32)
    n = x.size
    albedo = np.stack([x, np.roll(x, 1), np.roll(x, 2)], 1)
    rough, metal = np.roll(x, 3), np.roll(x, 5)
    ids = np.arange(n, dtype=np.int32)
    ids[::7] = -1                                                        # masked texels
    want_a = R.quantize_ref(albedo); want_a[ids < 0] = 0
    want_rm = np.stack([R.quantize_ref(rough), R.quantize_ref(metal), np.zeros(n, np.uint8)], 1); want_rm[ids < 0] = 0
    assert want_a.max() == 255 and want_a[~(ids < 0)].min() == 0 and len(np.unique(want_a)) == 256
    dev = torch.device(DEV)
    ids_d = torch.from_numpy(ids).to(dev)
    for cuts in ([0, n], [0, 5, 82, 83, 400, n]):                        # one call; ranges that start and end inside a group of four texels
        img_a = torch.full((n, 1, 3), 77, dtype=torch.uint8, device=dev)
        img_rm = torch.full((n, 1, 3), 77, dtype=torch.uint8, device=dev)
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            T.quantize_into(torch.from_numpy(albedo[t0:t1]).to(dev), torch.from_numpy(rough[t0:t1]).to(dev), torch.from_numpy(metal[t0:t1, None]).to(dev),
                            ids_d, t0, img_a, img_rm)
        assert np.array_equal(img_a.cpu().numpy().reshape(n, 3), want_a), cuts
        assert np.array_equal(img_rm.cpu().numpy().reshape(n, 3), want_rm), cuts
    img_a.fill_(77)                                                      # a range inside the texture leaves the rest alone
    T.quantize_into(torch.from_numpy(albedo[9:14]).to(dev), torch.from_numpy(rough[9:14]).to(dev), torch.from_numpy(metal[9:14]).to(dev), ids_d, 9, img_a, img_rm)
    got = img_a.cpu().numpy().reshape(n, 3)
    assert np.array_equal(got[9:14], want_a[9:14]) and (got[:9] == 77).all() and (got[14:] == 77).all()


# ------------------------------------------------------------------------------------------------------------------------------------- bake
BAKE_RES = 64


@functools.lru_cache(None)
def box_bake():
    """the box mesh under grid_atlas at 64 x 64, its reference raster and the expected images under StubMaterial"""
    from iris_amd.utils.texture import grid_atlas
    g = golden("bake_box.npz")
    v, f = g["verts"].astype(np.float32), g["faces"].astype(np.int32)
    vt, ft = grid_atlas(f.shape[0], BAKE_RES)
    ref = R.rasterize_uv_ref(vt, ft, v, f, BAKE_RES)
    mat = stub_material_np(ref["xyz"].reshape(-1, 3))
    mask = ref["mask"].reshape(-1)
    albedo = R.quantize_ref(mat["albedo"]) * mask[:, None].astype(np.uint8)
    rm = np.concatenate([R.quantize_ref(mat["roughness"]), R.quantize_ref(mat["metallic"]), np.zeros((mask.size, 1), np.uint8)], 1) * mask[:, None].astype(np.uint8)
    return g, v, f, vt, ft, ref, albedo.reshape(BAKE_RES, BAKE_RES, 3), rm.reshape(BAKE_RES, BAKE_RES, 3)


@pytest.mark.parametrize("chunk_size", [1000, BAKE_RES * BAKE_RES, 160000])
def test_bake_textures_stub_material(chunk_size):
    from iris_amd.utils.texture import bake_textures
    g, v, f, vt, ft, ref, want_albedo, want_rm = box_bake()
    assert 0.2 < ref["mask"].mean() < 0.95 and np.array_equal(np.unique(ref["ids"][ref["mask"]]), np.arange(f.shape[0]))
    albedo, rm = bake_textures(StubMaterial(), vt, ft, v, f, BAKE_RES, chunk_size=chunk_size, device=DEV)
    assert albedo.dtype == torch.uint8 and albedo.is_cuda and tuple(albedo.shape) == (BAKE_RES, BAKE_RES, 3) == tuple(rm.shape)
    assert np.array_equal(albedo.cpu().numpy(), want_albedo)
    assert np.array_equal(rm.cpu().numpy(), want_rm)
    assert want_albedo.max() > 150 and (rm.cpu().numpy()[..., 2] == 0).all()


@pytest.mark.parametrize("params", ["init", "wide"])
def test_bake_textures_ngpbrdf_equals_the_network_on_the_covered_texels_alone(params):
    """init: the network as init_parameters(1337) leaves it (outputs near 0.5 everywhere); wide: every parameter uniform in +-0.5, so that the outputs vary
    from texel to texel"""
    from iris_amd.model.brdf import NGPBRDF
    from iris_amd.utils.texture import bake_textures
    g, v, f, vt, ft, ref, _, _ = box_bake()
    dev = torch.device(DEV)
    net = NGPBRDF(float(g["voxel_min"]), float(g["voxel_max"])).init_parameters(seed=1337)
    if params == "wide":
        with torch.no_grad():
            net.mlp.params.copy_((torch.rand(net.mlp.params.numel(), generator=torch.Generator().manual_seed(5)) * 2 - 1) * 0.5)
    net = net.to(dev)
    albedo, rm = bake_textures(net, vt, ft, v, f, BAKE_RES, chunk_size=1000, device=dev)
    mask = ref["mask"]
    with torch.no_grad():
        mat = {k: t.cpu().numpy() for k, t in net(torch.from_numpy(ref["xyz"][mask]).to(dev)).items()}
    want_albedo = np.zeros((BAKE_RES, BAKE_RES, 3), np.uint8); want_rm = np.zeros((BAKE_RES, BAKE_RES, 3), np.uint8)
    want_albedo[mask] = R.quantize_ref(mat["albedo"])
    want_rm[mask] = np.concatenate([R.quantize_ref(mat["roughness"]), R.quantize_ref(mat["metallic"]), np.zeros((int(mask.sum()), 1), np.uint8)], 1)
    assert np.array_equal(albedo.cpu().numpy(), want_albedo) and np.array_equal(rm.cpu().numpy(), want_rm)
    assert want_albedo[mask].max() > 0
    if params == "wide":
        assert len(np.unique(want_albedo[mask])) > 20 and len(np.unique(want_rm[mask][:, :2])) > 20


# -------------------------------------------------------------------------------------------------------------------------------------- CLI
def test_export_cli_end_to_end(tmp_path):
    from iris_amd.utils import export as E
    g, v, f, vt, ft, ref, want_albedo, want_rm = box_bake()
    with open(tmp_path / "scene.obj", "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p) for p in v) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in f))
    bake = tmp_path / "bake"; bake.mkdir()
    torch.save({"mask": torch.from_numpy(g["slf_mask"]), "voxel_min": float(g["voxel_min"]), "voxel_max": float(g["voxel_max"])}, str(bake / "vslf.npz"))
    out = tmp_path / "texture"
    argv = ["--mesh", str(tmp_path / "scene.obj"), "--emitter_path", str(bake), "--dir_save", str(out), "--material", "stub_material:material", "--tex_res", str(BAKE_RES),
            "--chunk_size", "1500", "--device", DEV]
    E.main(argv + ["--atlas", "grid", "--write_obj"])
    assert sorted(os.listdir(out)) == ["albedo.png", "ft.npy", "mesh.mtl", "mesh.obj", "rm.png", "vt.npy"]
    assert np.array_equal(np.load(out / "vt.npy"), vt) and np.array_equal(np.load(out / "ft.npy"), ft)
    assert np.array_equal(decode_png(str(out / "albedo.png")), want_albedo) and np.array_equal(decode_png(str(out / "rm.png")), want_rm)
    first = {n: open(out / n, "rb").read() for n in ("albedo.png", "rm.png")}
    os.remove(out / "albedo.png"); os.remove(out / "rm.png")
    E.main(argv + ["--atlas", "auto"])                                   # picks the saved .npy files up
    assert {n: open(out / n, "rb").read() for n in ("albedo.png", "rm.png")} == first
