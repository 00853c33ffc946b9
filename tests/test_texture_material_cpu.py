"""The texture material on the CPU: the two restatements (tests/closest_ref64.py, tests/texmat_ref.py) on cases with known answers, what
BakedTextureBRDF.from_export and the stages refuse before a device is touched, and --verify's point generator."""
import numpy as np
import pytest
import torch

import closest_ref64 as C
import texmat_ref as T

TRI_V = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float64)
TRI_F = np.array([[0, 1, 2]])


@pytest.mark.parametrize("point, want", [
    ((0.5, 0.5, 3.0), 3.0),                         # above the interior
    ((1.0, -2.0, 0.0), 2.0),                        # beyond the edge p0 p1, in the plane
    ((1.0, -3.0, 4.0), 5.0),                        # beyond that edge and above it
    ((3.0, -1.0, 0.0), 2.0 ** 0.5),                 # beyond the vertex p1
    ((-2.0, -2.0, 1.0), 3.0),                       # beyond the vertex p0
    ((2.0, 2.0, 0.0), 2.0 ** 0.5),                  # in the plane, outside: the hypotenuse x + y = 2
    ((0.25, 0.25, 0.0), 0.0),                       # on the triangle
])
def test_point_triangle_distance_known_answers(point, want):
    r = C.closest_ref(TRI_V, TRI_F, [point], slack=0.0)
    assert abs(r["dist"][0] - want) <= 1e-15 * max(want, 1.0) and r["argmin"][0] == 0 and r["runner_up"][0] == np.inf


def test_reference_argmin_near_set_and_zero_area():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [0.2, 0.2, 0.4], [0.3, 0.3, 0.4]], np.float64)
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 6, 7], [6, 7, 7]])           # z = 0, z = 1, and two zero-area faces nearer to the points than either
    r = C.closest_ref(v, f, [(0.2, 0.2, 0.45), (0.2, 0.2, 0.5), (0.2, 0.2, 0.75)], slack=0.1)
    assert r["argmin"].tolist() == [0, 0, 1] and np.allclose(r["dist"], [0.45, 0.5, 0.25]) and np.allclose(r["runner_up"], [0.55, 0.5, 0.75])
    assert r["near"].tolist() == [[True, True, False, False], [True, True, False, False], [False, True, False, False]]
    p = C.rebuild(v, f, [0, 1], [[0.25, 0.5], [0.0, 1.0]])
    assert np.allclose(p, [[0.25, 0.5, 0.0], [0.0, 1.0, 1.0]])


# one quad of two faces over the whole UV square; a 3 x 4 image with the column in red, the row in green
QUAD_VT = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
QUAD_FT = np.array([[0, 1, 2], [0, 2, 3]])


def _index_images(H, W):
    a = np.zeros((H, W, 3), np.uint8)
    a[..., 0] = np.arange(W)[None, :] * 10
    a[..., 1] = np.arange(H)[:, None] * 20
    a[..., 2] = 255
    rm = np.zeros((H, W, 3), np.uint8)
    rm[..., 0] = np.arange(W)[None, :] * 50 + 40
    rm[..., 1] = np.arange(H)[:, None] * 60
    return a, rm


def _uv_to_bary(u, v):
    """face 0 of the quad: uv = b1 (1, 0) + b2 (1, 1) -> b2 = v, b1 = u - v (needs u >= v)"""
    return np.array([[u - v, v]], np.float32)


def test_fetch_texel_centres_midpoints_and_clamps():
    H, W = 3, 4
    a, rm = _index_images(H, W)
    for r in range(H):
        for c in range(r * W // H + 1, W):                             # texel centres with u >= v: inside face 0
            out = T.fetch([0], _uv_to_bary((c + 0.5) / W, (r + 0.5) / H), QUAD_FT, QUAD_VT, a, rm)
            assert np.allclose(out["albedo"][0] * 255, [c * 10, r * 20, 255], atol=1e-4), (r, c)
            assert np.allclose([out["roughness"][0, 0] * 255, out["metallic"][0, 0] * 255], [c * 50 + 40, r * 60], atol=1e-4)
    mid = T.fetch([0], _uv_to_bary(3.0 / W, 0.5 / H), QUAD_FT, QUAD_VT, a, rm)            # between columns 2 and 3 of row 0
    assert np.allclose(mid["albedo"][0] * 255, [25.0, 0.0, 255.0], atol=1e-4)
    mid = T.fetch([0], _uv_to_bary(3.5 / W, 1.0 / H), QUAD_FT, QUAD_VT, a, rm)            # between rows 0 and 1 of column 3
    assert np.allclose(mid["albedo"][0] * 255, [30.0, 10.0, 255.0], atol=1e-4)
    vt = QUAD_VT * 3 - 1                                                                     # UVs from -1 to 2: u < 0 and u > 1 clamp to the border texels
    lo = T.fetch([1], np.array([[0.0, 1.0]], np.float32), QUAD_FT, vt, a, rm)                # vertex 3: uv = (-1, 2)
    assert np.allclose(lo["albedo"][0] * 255, [0.0, (H - 1) * 20, 255.0], atol=1e-4)
    hi = T.fetch([0], np.array([[1.0, 0.0]], np.float32), QUAD_FT, vt, a, rm)                # vertex 1: uv = (2, -1)
    assert np.allclose(hi["albedo"][0] * 255, [(W - 1) * 10, 0.0, 255.0], atol=1e-4)
    none = T.fetch([-1], np.zeros((1, 2), np.float32), QUAD_FT, QUAD_VT, a, rm)
    assert none["albedo"].tolist() == [[0, 0, 0]] and none["roughness"][0, 0] == 0.02 and none["metallic"][0, 0] == 0
    rm[...] = 0
    assert T.fetch([0], _uv_to_bary(0.6, 0.3), QUAD_FT, QUAD_VT, a, rm)["roughness"][0, 0] == 0.02      # the network's floor, put back


# ---- refusals before the device
def _export_dir(path, H=8, W=8, F=2, n_vt=4, mode="RGB", rm_size=None, ft=None, vt=None):
    from PIL import Image
    path.mkdir(parents=True, exist_ok=True)
    np.save(path / "ft.npy", QUAD_FT.astype(np.int32)[:F] if ft is None else ft)
    np.save(path / "vt.npy", QUAD_VT[:n_vt] if vt is None else vt)
    shape = (H, W, 3) if mode == "RGB" else (H, W)
    Image.fromarray(np.zeros(shape, np.uint8), mode).save(path / "albedo.png")
    hr, wr = rm_size or (H, W)
    Image.fromarray(np.zeros((hr, wr, 3), np.uint8), "RGB").save(path / "rm.png")
    return str(path)


QUAD_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
QUAD_F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def test_from_export_refuses_before_the_device(tmp_path, monkeypatch):
    from iris_amd import _lib as L
    from iris_amd.model import texture as M
    from iris_amd.utils import path_tracing as PT

    def no_scene(*a, **k):
        raise AssertionError("a Scene was built: the device was touched")
    monkeypatch.setattr(PT, "Scene", no_scene)
    bad_vt = QUAD_VT.copy(); bad_vt[2, 1] = np.nan
    big = M.MAX_TEX_RES + 1
    cases = {
        "sizes": (dict(rm_size=(8, 4)), "differ in size"),
        "grey": (dict(mode="L"), "8-bit RGB"),
        "faces": (dict(F=1), "the mesh has 2 faces"),
        "index": (dict(ft=np.array([[0, 1, 2], [0, 2, 4]], np.int32)), "outside the 4 UV vertices"),
        "nan": (dict(vt=bad_vt), "non-finite"),
        "side": (dict(H=1, W=big), f"at most {M.MAX_TEX_RES}"),
    }
    for name, (kw, text) in cases.items():
        with pytest.raises(L.IrisError, match=text):
            M.BakedTextureBRDF.from_export(_export_dir(tmp_path / name, **kw), QUAD_V, QUAD_F, "cuda")
    (tmp_path / "empty").mkdir()
    with pytest.raises(L.IrisError, match="ft.npy not found"):
        M.BakedTextureBRDF.from_export(str(tmp_path / "empty"), QUAD_V, QUAD_F, "cuda")
    # the same checks on arrays, and what the files cannot express
    a = np.zeros((4, 4, 3), np.uint8)
    assert M.check_texture_inputs(QUAD_FT, QUAD_VT, a, a, n_faces=2) == (4, 4)
    for kw, text in ((dict(albedo_img=a.astype(np.uint16)), "8-bit RGB"), (dict(albedo_img=a[..., :2]), "8-bit RGB"), (dict(ft=QUAD_FT.astype(np.float32)), "integer"),
                     (dict(vt=QUAD_VT.astype(np.int32)), "floating-point"), (dict(ft=QUAD_FT - 1), "outside")):
        args = dict(ft=QUAD_FT, vt=QUAD_VT, albedo_img=a, rm_img=a)
        args.update(kw)
        with pytest.raises(L.IrisError, match=text):
            M.check_texture_inputs(**args, n_faces=2)
    with pytest.raises(L.IrisError, match="requires grad"):
        M._Textures(QUAD_FT, torch.from_numpy(QUAD_VT).requires_grad_(True), a, a, "cuda")


@pytest.mark.parametrize("module, parser", [("render", "build_cli_parser"), ("render_video", "build_parser"), ("render_relight", "build_video_parser")])
def test_textures_with_material_is_refused_before_the_device(module, parser, monkeypatch):
    import importlib
    from iris_amd import _lib as L
    from iris_amd.utils import stage
    mod = importlib.import_module("iris_amd." + module)

    def no_device(*a, **k):
        raise AssertionError("the device was opened")
    monkeypatch.setattr(stage, "open_device", no_device)
    base = ["--experiment_name", "e", "--emitter_path", "b"] + (["--light_cfg", "l.yaml"] if module == "render_relight" else [])
    args = getattr(mod, parser)().parse_args(base + ["--textures", "out/texture"])
    assert args.textures == "out/texture" and args.material is None
    assert getattr(mod, parser)().parse_args(base).textures is None                     # off by default: the stage runs as it did
    with pytest.raises(L.IrisError, match="--textures and --material"):
        mod.main(base + ["--textures", "out/texture", "--material", "stub_material:material"])


def test_refine_shading_keeps_material_only():
    from iris_amd import refine_shading
    with pytest.raises(SystemExit):
        refine_shading.build_parser().parse_args(["--scene", "s", "--slf_path", "a", "--emitter_path", "b", "--output", "o", "--textures", "t"])


def test_verify_points_are_reproducible():
    from iris_amd import _lib as L
    from iris_amd.utils import export as E
    rng = np.random.default_rng(5)
    v = rng.normal(size=(30, 3)).astype(np.float32)
    f = rng.integers(0, 30, size=(17, 3)).astype(np.int32)
    face, bary, pos = E.verify_points(v, f, 100)
    face2, bary2, pos2 = E.verify_points(v.copy(), f.copy(), 100)
    assert np.array_equal(face, face2) and np.array_equal(bary, bary2) and np.array_equal(pos, pos2)
    assert face.tolist() == [i * 17 // 100 for i in range(100)]
    u = torch.rand(100, 2, generator=torch.Generator().manual_seed(0)).numpy()
    fold = u.sum(1) > 1
    assert fold.any() and (~fold).any()
    assert np.array_equal(bary, np.where(fold[:, None], np.float32(1) - u, u))
    assert (bary >= 0).all() and (bary.sum(1) <= 1 + 1e-6).all() and bary.dtype == np.float32 and pos.dtype == np.float32
    assert np.abs(C.rebuild(v, f, face, bary) - pos).max() <= 8 * 2.0 ** -24 * np.abs(v).max()
    assert E.verify_points(v, f, 7)[0].tolist() == [0, 2, 4, 7, 9, 12, 14]
    with pytest.raises(L.IrisError):
        E.verify_points(v, f, 0)
    cli = E.build_parser(area_atlas=True, verify=True)
    assert cli.parse_args([]).verify == 0 and cli.parse_args(["--verify", "4096"]).verify == 4096
    with pytest.raises(SystemExit):
        E.build_parser(area_atlas=True).parse_args(["--verify", "5"])
