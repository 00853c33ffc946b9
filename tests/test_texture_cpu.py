"""The texture export stage without a device: the numpy restatement of the rasteriser's contract (tests/uv_raster_ref.py) against hand-derived cases, the
grid atlas, the PNG and OBJ writers, the host checks, the command line's atlas rule and the new entry points' declarations."""
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import REPO
import uv_raster_ref as R


def centres(points, res=8):
    """UVs of points given in texel-index coordinates (c, r): the centre of texel (r, c) is (c, r)"""
    return ((np.asarray(points, np.float64) + 0.5) / res).astype(np.float32)


def corners(points, res=8):
    """UVs of points given in texel-corner coordinates: (c, r) is the corner shared by texels (r - 1, c - 1) and (r, c)"""
    return (np.asarray(points, np.float64) / res).astype(np.float32)


# The two hand-derived cases, shared with tests/test_texture.py ------------------------------------------------------------------------------------------
def case_triangles_on_centres():
    """8 x 8.  Face 0: centres (1,1), (5,1), (1,5) (as (c, r)).  Its edge r = 1 has the interior on the +y side and no x in its normal: it keeps its centres.
    Its edge c = 1 has the interior on the +x side: kept.  Its hypotenuse c + r = 6 has the interior on the -x side: dropped, and the vertices (5,1), (1,5)
    with it.  Face 1: centres (5,5), (1,5), (5,1), the other half: its hypotenuse has the interior on the +x side (kept), its edges r = 5 (interior on -y) and
    c = 5 (interior on -x) are dropped, and all three vertices with them."""
    vt = centres([(1, 1), (5, 1), (1, 5), (5, 5), (1, 5), (5, 1)])
    ft = np.arange(6, dtype=np.int32).reshape(2, 3)
    want = np.full((8, 8), -1, np.int32)
    for r in range(8):
        for c in range(8):
            if c >= 1 and r >= 1 and c + r < 6:
                want[r, c] = 0
            elif c + r >= 6 and c < 5 and r < 5:
                want[r, c] = 1
    return vt, ft, want


def case_square_split():
    """8 x 8.  The square of the texel corners (1,1)..(5,5) holds the 16 centres c, r in 1..4; its diagonal from corner (1,1) to corner (5,5) runs through the
    centres c == r.  Face 0 = (1,1), (5,1), (5,5) is the half with c > r: the interior lies on the +x side of the diagonal, so face 0 owns the diagonal's
    centres.  Face 1 = (1,1), (5,5), (1,5) gets c < r."""
    vt = corners([(1, 1), (5, 1), (5, 5), (1, 5)])
    ft = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    want = np.full((8, 8), -1, np.int32)
    for r in range(1, 5):
        for c in range(1, 5):
            want[r, c] = 0 if c >= r else 1
    return vt, ft, want


def test_reference_triangles_with_vertices_on_texel_centres():
    vt, ft, want = case_triangles_on_centres()
    count, ids = R.coverage(vt, ft, 8)
    assert np.array_equal(ids, want)
    assert (want == 0).sum() == 10 and (want == 1).sum() == 6
    assert want[1, 1] == 0 and want[1, 5] == -1 and want[5, 1] == -1 and want[5, 5] == -1          # the vertex centres
    assert count.max() == 1                                                                        # the shared hypotenuse belongs to exactly one face
    for order in ([0, 2, 1], [1, 0, 2]):                                                           # the other winding, another first vertex: the same coverage
        assert np.array_equal(R.coverage(vt, ft[:, order], 8)[1], want)
    out = R.rasterize_uv_ref(vt, ft, np.eye(3, dtype=np.float32)[[0, 1, 2, 0, 1, 2]], ft, 8)
    # with v = unit vectors, xyz = (b0, b1, b2): texel (r 2, c 2) of face 0 sits 1/4 along both legs
    assert np.array_equal(out["bary"][2, 2], np.float32([0.5, 0.25])) and np.array_equal(out["xyz"][2, 2], np.float32([0.5, 0.25, 0.25]))
    assert np.array_equal(out["bary"][1, 1], np.float32([1, 0]))


def test_reference_square_split_along_a_diagonal_through_centres():
    vt, ft, want = case_square_split()
    count, ids = R.coverage(vt, ft, 8)
    assert np.array_equal(ids, want)
    assert np.array_equal(count, (want >= 0).astype(np.int32))                                     # every centre of the square exactly once, none outside
    count2, ids2 = R.coverage(vt, ft[::-1], 8)                                                     # ownership does not depend on the face order
    assert np.array_equal(count2, count) and np.array_equal(ids2 >= 0, ids >= 0) and np.array_equal(ids2[want == 0], np.ones(10, np.int32))


@pytest.mark.parametrize("F, tex_res", [(1, 4), (2, 5), (7, 8), (7, (9, 13)), (50, 20), (50, 23), (51, (31, 24)), (1000, 96)])
def test_grid_atlas(F, tex_res):
    from iris_amd.utils.texture import grid_atlas
    vt, ft = grid_atlas(F, tex_res)
    assert vt.shape == (3 * F, 2) and vt.dtype == np.float32 and ft.dtype == np.int32 and np.array_equal(ft, np.arange(3 * F).reshape(F, 3))
    assert vt.min() >= 0.0 and vt.max() <= 1.0
    G = int(np.ceil(np.sqrt((F + 1) // 2)))
    H, W = (tex_res, tex_res) if np.isscalar(tex_res) else tex_res
    assert min(H, W) / G >= 4                                                                      # the case is one the property is promised for
    count, ids = R.coverage(vt, ft, tex_res)
    assert count.max() == 1                                                                        # no texel centre inside two faces
    assert np.array_equal(np.unique(ids[ids >= 0]), np.arange(F))                                  # every face covers a texel


def _png_chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        out.append((tag, body))
        pos += 12 + n
    return out


def decode_png(path):
    """8-bit RGB, filter 0 only: what write_png writes"""
    chunks = _png_chunks(open(path, "rb").read())
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(H, 1 + 3 * W)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(H, W, 3)


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (64, 33)])
def test_write_png_round_trip(tmp_path, shape):
    from iris_amd.utils.texture import write_png
    img = np.random.default_rng(3).integers(0, 256, shape + (3,), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    write_png(path, img)
    assert np.array_equal(decode_png(path), img)
    try:
        from PIL import Image
    except ImportError:
        return
    pil = np.asarray(Image.open(path))
    assert pil.shape == img.shape and np.array_equal(pil, img)


def test_write_png_rejects_other_images(tmp_path):
    from iris_amd._lib import IrisError
    from iris_amd.utils.texture import write_png
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32)):
        with pytest.raises(IrisError):
            write_png(str(tmp_path / "b.png"), bad)


def test_write_textured_obj_parses_back(tmp_path):
    from iris_amd.utils.path_tracing import load_mesh
    from iris_amd.utils.texture import grid_atlas, write_textured_obj
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((9, 3)) * 3).astype(np.float32)
    f = rng.integers(0, 9, (7, 3)).astype(np.int32)
    vt, ft = grid_atlas(7, 32)
    write_textured_obj(str(tmp_path), v, f, vt, ft)
    pv, pvt, pf, pft = [], [], [], []
    for line in open(tmp_path / "mesh.obj"):
        tok = line.split()
        if tok[0] == "v":
            pv.append([np.float32(x) for x in tok[1:]])
        elif tok[0] == "vt":
            pvt.append([np.float32(x) for x in tok[1:]])
        elif tok[0] == "f":
            pf.append([int(t.split("/")[0]) - 1 for t in tok[1:]])
            pft.append([int(t.split("/")[1]) - 1 for t in tok[1:]])
    assert np.array_equal(np.float32(pv), v) and np.array_equal(np.float32(pvt), vt) and np.array_equal(pf, f) and np.array_equal(pft, ft)
    lv, lf = load_mesh(str(tmp_path / "mesh.obj"))                                                 # the project's own reader takes it too
    assert np.array_equal(lv, v) and np.array_equal(lf, f)
    assert "mtllib mesh.mtl" in open(tmp_path / "mesh.obj").read() and "map_Kd albedo.png" in open(tmp_path / "mesh.mtl").read()


def test_host_checks_raise_without_a_device():
    from iris_amd._lib import IrisError
    from iris_amd.utils.texture import bake_textures, rasterize_uv
    vt = np.float32([[0.1, 0.1], [0.9, 0.1], [0.1, 0.9]])
    ft = np.int32([[0, 1, 2]])
    v = np.eye(3, dtype=np.float32)
    f = np.int32([[0, 1, 2]])

    def bad(**kw):
        a = dict(vt=vt, ft=ft, v=v, f=f, tex_res=8)
        a.update(kw)
        with pytest.raises(IrisError):
            rasterize_uv(a["vt"], a["ft"], a["v"], a["f"], a["tex_res"])
        with pytest.raises(IrisError):
            bake_textures(lambda x: None, a["vt"], a["ft"], a["v"], a["f"], a["tex_res"])
    for value in (np.nan, np.inf, -np.inf):                                                        # non-finite UVs
        w = vt.copy(); w[1, 0] = value
        bad(vt=w)
    for value in (-1.0001, 2.0001):                                                                # UVs outside [-1, 2]
        w = vt.copy(); w[2, 1] = value
        bad(vt=w)
    for res in (0, -1, 8193, (8, 0), (8193, 8), 7.5):                                              # tex_res outside [1, 8192]
        bad(tex_res=res)
    bad(ft=np.int32([[0, 1, 3]])); bad(ft=np.int32([[0, -1, 2]]))                                  # ft out of range
    bad(f=np.int32([[0, 1, 3]])); bad(f=np.int32([[-1, 1, 2]]))                                    # f out of range
    bad(ft=np.int32([[0, 1, 2], [0, 1, 2]]))                                                       # ft.shape != f.shape
    # the limits themselves pass the checks
    from iris_amd.utils.texture import check_inputs
    assert check_inputs(np.float32([[-1, -1], [2, -1], [-1, 2]]), ft, v, f, 8192) == (8192, 8192)
    assert check_inputs(vt, ft, v, f, (1, 3)) == (1, 3)


def test_inputs_that_require_grad_raise():
    import torch
    from iris_amd._lib import IrisError
    from iris_amd.utils.texture import rasterize_uv
    v = torch.eye(3, requires_grad=True)
    with pytest.raises(IrisError, match="requires grad"):
        rasterize_uv(torch.rand(3, 2), torch.tensor([[0, 1, 2]], dtype=torch.int32), v, torch.tensor([[0, 1, 2]], dtype=torch.int32), 8)


def test_cli_atlas_auto_without_files_exits_with_the_message(tmp_path):
    with open(tmp_path / "m.obj", "w") as fh:
        fh.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, os.path.join(REPO, "tests")]))
    p = subprocess.run([sys.executable, "-m", "iris_amd.utils.export", "--mesh", str(tmp_path / "m.obj"), "--emitter_path", str(tmp_path), "--dir_save",
                        str(tmp_path / "out"), "--material", "stub_material:material", "--tex_res", "16"], env=env, cwd=str(tmp_path), capture_output=True, text=True)
    assert p.returncode != 0
    for word in ("--atlas grid", "ft.npy", "vt.npy"):
        assert word in p.stderr, p.stderr
    assert not os.path.exists(tmp_path / "out" / "albedo.png") and not os.path.exists(tmp_path / "out" / "vt.npy")


def test_texture_entry_points_are_declared_exported_and_bound():
    from iris_amd import _lib as L
    exported = set(re.findall(r" T (iris_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()))
    headers = {"iris_hip.h": ("iris_uv_raster_workspace_bytes", "iris_uv_raster", "iris_uv_resolve", "iris_texture_quantize"),
               "iris_hip_debug.h": ("iris_debug_uv_raster",)}
    for header, names in headers.items():
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
        for name in names:
            m = re.search(r"IRIS_API\s+(?:int|uint64_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
            assert m, name + " is not declared in include/" + header
            assert len(m.group(1).split(",")) == len(L.PROTOTYPES[name]), name
            assert name in exported, name
            assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name]
    # the debug entry point is the public one plus the class selector, and the public header has no such knob
    assert len(L.PROTOTYPES["iris_debug_uv_raster"]) == len(L.PROTOTYPES["iris_uv_raster"]) + 1
    assert L.lib().iris_uv_raster_workspace_bytes(-1) == 0 and L.lib().iris_uv_raster_workspace_bytes(10) >= 16 + 12 * 10
    src = open(os.path.join(REPO, "iris_amd", "csrc", "iris_texture.h")).read()
    assert "atomicMin" in src and not re.search(r"atomic\w*\s*\(\s*\(?\s*float", src) and "atomicAdd(float" not in src          # integer atomics only
