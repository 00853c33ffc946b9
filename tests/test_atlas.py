"""The area-proportional atlas and the seam dilation on the GPU (iris_amd/csrc/iris_atlas.h, iris_amd.utils.texture.area_atlas / dilate_into,
python -m iris_amd.utils.export --atlas area --dilate N): bit for bit against the numpy restatement of their contract (tests/atlas_ref.py).  Nothing here has
a tolerance: vt by its bit patterns, ft, j and the histogram as integers, the images as bytes."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import golden
import atlas_ref as A
from stub_material import StubMaterial
from test_atlas_cpu import CASES, LARGE_CASES, mesh, soup
from test_texture_cpu import decode_png

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@functools.lru_cache(None)
def reference(kind, F, res):
    v, f = mesh(kind, F)
    return (v, f) + A.area_atlas_ref(v, f, res)


def same_atlas(got, want_vt, want_ft, want_rep):
    vt, ft, rep = got
    assert vt.is_cuda and ft.is_cuda and vt.dtype == torch.float32 and ft.dtype == torch.int32 and tuple(ft.shape) == want_ft.shape
    assert np.array_equal(bits(vt.cpu().numpy()), bits(want_vt)), np.argwhere(bits(vt.cpu().numpy()) != bits(want_vt))[:8]
    assert np.array_equal(ft.cpu().numpy(), want_ft)
    assert rep == want_rep                                      # j, D_j, the histogram, used and the clamped counts: integers and exact float64


@pytest.mark.parametrize("kind, F, res", CASES + LARGE_CASES)
def test_area_atlas_equals_the_restatement(kind, F, res):
    from iris_amd.utils.texture import area_atlas
    v, f, want_vt, want_ft, want_rep = reference(kind, F, res)
    same_atlas(area_atlas(v, f, res, device=DEV), want_vt, want_ft, want_rep)


@pytest.mark.parametrize("kind, F, res", [("soup", 65, 64), ("degenerate", 12, 16), ("soup", 4099, 512)])
def test_device_tensors_and_a_second_call_give_the_same(kind, F, res):
    from iris_amd.utils.texture import area_atlas
    v, f, want_vt, want_ft, want_rep = reference(kind, F, res)
    dev = torch.device(DEV)
    v_d, f_d = torch.from_numpy(v).to(dev), torch.from_numpy(np.ascontiguousarray(f)).to(dev)          # (f keeps its dtype: the degenerate mesh's is int64)
    first = area_atlas(v_d, f_d, res)
    same_atlas(first, want_vt, want_ft, want_rep)
    same_atlas(area_atlas(v_d, f_d, res), want_vt, want_ft, want_rep)
    same_atlas(area_atlas(v.astype(np.float64), f.astype(np.int64), (res, res), device=dev), want_vt, want_ft, want_rep)
    assert first[0].device == dev


def test_nothing_is_launched_when_the_arguments_are_refused(monkeypatch):
    from iris_amd.utils import texture as T

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(T.L, "lib", no_library)
    monkeypatch.setattr(T, "_upload", lambda *a: no_library())
    v, f = soup(33, seed=2)
    dev = torch.device(DEV)
    for args in ((v, f, 16), (torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), 16), (v, f, (16, 32)), (v, f, 24), (v, f, 2), (v[:, :2], f, 64), (v, f[:0], 64)):
        with pytest.raises(T.L.IrisError, match="area_atlas"):
            T.area_atlas(*args, device=dev)
    with pytest.raises(T.L.IrisError, match="requires grad"):
        T.area_atlas(torch.from_numpy(v).to(dev).requires_grad_(), f, 64)
    ids = torch.zeros(4, 4, dtype=torch.int32, device=dev)
    img = torch.zeros(4, 4, 3, dtype=torch.uint8, device=dev)
    for n in (5, -1):
        with pytest.raises(T.L.IrisError, match="dilate"):
            T.dilate_into(ids, img, img.clone(), n)
    with pytest.raises(T.L.IrisError, match="dilate"):
        T.dilate_into(ids, img, img[:2], 1)
    with pytest.raises(T.L.IrisError, match="same image"):
        T.dilate_into(ids, img, img, 1)


def test_a_mesh_the_ladder_cannot_hold_is_refused():
    """one face near the top of float32 beside ordinary ones: even the lowest density asks for more texels than there are (the restatement refuses it too)"""
    from iris_amd.utils import texture as T
    v, f = np.float32([[0, 0, 0], [3e38, 0, 0], [0, 3e38, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[0, 1, 2], [0, 3, 4], [0, 4, 3]])
    with pytest.raises(A.AtlasError, match="lowest density"):
        A.area_atlas_ref(v, f, 16)
    with pytest.raises(T.L.IrisError, match="lowest density"):
        T.area_atlas(v, f, 16, device=DEV)


@pytest.mark.parametrize("kind, F, res", [("soup", 65, 64), ("soup", 1023, 512), ("equal", 65, 64)])
def test_the_rasteriser_gives_every_face_a_texel(kind, F, res):
    from iris_amd.utils import texture as T
    v, f = mesh(kind, F)
    vt, ft, _ = T.area_atlas(v, f, res, device=DEV)
    out = T.rasterize_uv(vt, ft, v, f, res)                     # the device tensors go in as they are
    ids = out["ids"].cpu().numpy()
    assert np.array_equal(np.unique(ids[ids >= 0]), np.arange(F))
    per_face = np.bincount(ids[ids >= 0], minlength=F)
    k = A.classes(A.measure(v, f)[0], reference(kind, F, res)[4]["j"], res.bit_length() - 1)[0].astype(np.int64)
    assert (per_face <= 4 ** k // 2).all() and (per_face >= 4 ** k // 8).all()          # between an eighth and a half of its cell's texels (margin and gap)


# ---------------------------------------------------------------------------------------------------------------------------------- dilation
@pytest.mark.parametrize("n", [0, 1, 2, 4])
@pytest.mark.parametrize("shape", [(5, 7), (16, 16), (33, 65)])
def test_dilate_into_equals_the_restatement(shape, n):
    from iris_amd.utils.texture import dilate_into
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    ids = np.where(rng.uniform(size=shape) < 0.15, rng.integers(0, 50, shape), -1).astype(np.int32)          # sparse: many texels have nothing within reach
    ids[H // 2:, : W // 3] = -1
    ids[0, 0], ids[0, 1] = 3, -1                                # at least one texel to take from, and one beside it to fill
    albedo, rm = rng.integers(0, 256, shape + (3,), dtype=np.uint8), rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    want_a, want_rm = A.dilate_ref(ids, albedo, rm, n)
    dev = torch.device(DEV)
    ids_d, a_d, rm_d = torch.from_numpy(ids).to(dev), torch.from_numpy(albedo).to(dev), torch.from_numpy(rm).to(dev)
    dilate_into(ids_d, a_d, rm_d, n)
    got_a, got_rm = a_d.cpu().numpy(), rm_d.cpu().numpy()
    assert np.array_equal(got_a, want_a) and np.array_equal(got_rm, want_rm)
    assert np.array_equal(ids_d.cpu().numpy(), ids)
    assert np.array_equal(got_a[ids >= 0], albedo[ids >= 0]) and np.array_equal(got_rm[ids >= 0], rm[ids >= 0])
    changed = (got_a != albedo).any(-1) | (got_rm != rm).any(-1)
    if n == 0:
        assert not changed.any()
    else:
        assert changed[0, 1] and (shape != (33, 65) or not changed[24:29, 5:12].any())          # some filled; the middle of the empty block is out of reach


# -------------------------------------------------------------------------------------------------------------------------------------- CLI
BAKE_RES = 64


def test_export_cli_area_atlas_and_dilation(tmp_path):
    from iris_amd.utils import export as E
    from iris_amd.utils.path_tracing import load_mesh
    g = golden("bake_box.npz")
    v, f = g["verts"].astype(np.float32), g["faces"].astype(np.int32)
    with open(tmp_path / "scene.obj", "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p) for p in v) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in f))
    bake = tmp_path / "bake"; bake.mkdir()
    torch.save({"mask": torch.from_numpy(g["slf_mask"]), "voxel_min": float(g["voxel_min"]), "voxel_max": float(g["voxel_max"])}, str(bake / "vslf.npz"))
    plain, dilated = tmp_path / "plain", tmp_path / "dilated"
    argv = ["--mesh", str(tmp_path / "scene.obj"), "--emitter_path", str(bake), "--material", "stub_material:material", "--tex_res", str(BAKE_RES),
            "--chunk_size", "1500", "--device", DEV, "--atlas", "area"]
    E.main(argv + ["--dir_save", str(plain), "--dilate", "0"])
    E.main(argv + ["--dir_save", str(dilated), "--dilate", "2", "--write_obj"])
    assert sorted(os.listdir(dilated)) == ["albedo.png", "ft.npy", "mesh.mtl", "mesh.obj", "rm.png", "vt.npy"]
    want_vt, want_ft, _ = A.area_atlas_ref(v, f, BAKE_RES)
    for out in (plain, dilated):
        got_vt, got_ft = np.load(out / "vt.npy"), np.load(out / "ft.npy")
        assert got_vt.dtype == np.float32 and got_ft.dtype == np.int32 and np.array_equal(bits(got_vt), bits(want_vt)) and np.array_equal(got_ft, want_ft)
    import uv_raster_ref as R
    ids = R.coverage(want_vt, want_ft, BAKE_RES)[1]
    a0, m0 = decode_png(str(plain / "albedo.png")), decode_png(str(plain / "rm.png"))
    a2, m2 = decode_png(str(dilated / "albedo.png")), decode_png(str(dilated / "rm.png"))
    covered = ids >= 0
    assert 0.3 < covered.mean() < 0.95 and not a0[~covered].any() and a0[covered].max() > 0            # the plain run leaves the uncovered texels black
    assert np.array_equal(a2[covered], a0[covered]) and np.array_equal(m2[covered], m0[covered])
    want_a, want_m = A.dilate_ref(ids, a0, m0, 2)
    assert np.array_equal(a2, want_a) and np.array_equal(m2, want_m) and not np.array_equal(a2, a0)
    lv, lf = load_mesh(str(dilated / "mesh.obj"))                                                     # the project's own reader takes the textured OBJ
    assert np.array_equal(lv, v) and np.array_equal(lf, f)


def test_bake_textures_dilate_argument():
    from iris_amd.utils import texture as T
    g = golden("bake_box.npz")
    v, f = g["verts"].astype(np.float32), g["faces"].astype(np.int32)
    vt, ft, _ = T.area_atlas(v, f, BAKE_RES, device=DEV)
    a0, m0 = T.bake_textures(StubMaterial(), vt, ft, v, f, BAKE_RES, device=DEV)
    a1, m1 = T.bake_textures(StubMaterial(), vt, ft, v, f, BAKE_RES, device=DEV, dilate=1)
    ids = T.UVMesh(vt, ft, v, f, BAKE_RES, device=DEV).raster()
    want_a, want_m = A.dilate_ref(ids.cpu().numpy(), a0.cpu().numpy(), m0.cpu().numpy(), 1)
    assert np.array_equal(a1.cpu().numpy(), want_a) and np.array_equal(m1.cpu().numpy(), want_m) and not torch.equal(a0, a1)
