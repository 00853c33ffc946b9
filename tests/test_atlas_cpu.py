"""The area-proportional atlas and the seam dilation without a device: properties of the numpy restatement of their contract (tests/atlas_ref.py) on random
and constructed meshes, with the rasteriser's restatement (tests/uv_raster_ref.py) for coverage; the host checks of the package; the declarations of the new
entry points.  The meshes are shared with tests/test_atlas.py, which holds the device to the restatement bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
import atlas_ref as A
import uv_raster_ref as R


# ------------------------------------------------------------------------------------------------------------------------------------ meshes
def soup(F, seed=0, octaves=24):
    """F triangles with vertices of their own, areas log-uniform over `octaves` octaves (edge lengths over half as many), the vertex order shuffled"""
    rng = np.random.default_rng(seed)
    scale = 2.0 ** rng.uniform(-octaves / 4, octaves / 4, (F, 1, 1))
    v = (rng.uniform(-3, 3, (F, 1, 3)) + rng.standard_normal((F, 3, 3)) * scale).reshape(-1, 3)
    perm = rng.permutation(3 * F)
    out = np.zeros_like(v)
    out[perm] = v
    return out.astype(np.float32), perm.reshape(F, 3).astype(np.int32)


def equal_areas(F):
    """one triangle translated by whole numbers: every S is the same float64"""
    base = np.float32([[0, 0, 0], [1.5, 0, 0], [0.25, 1, 0.5]])
    off = np.stack([np.arange(F) % 7, np.arange(F) // 7, np.arange(F) % 3], 1).astype(np.float32)
    return (base[None] + off[:, None]).reshape(-1, 3), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def threshold_triangles():
    """8 right triangles with legs 2^p and 2^-p: S = 1 for each, exactly.  At R = 16 they take 4 cells, which fit as 8 x 8 cells (4 * 64 = 256 texels) and not as
    16 x 16 ones: the largest step with 4 * 16^3 >= 1 * D_j is D_j = 2^14, j = 28, where the rule holds with EQUALITY.  A rule that sent equality to k + 1 would
    not fit there and would choose j = 27.  The right angle sits at corner 0, 1 and 2 in turn (the hypotenuse is the longest edge)."""
    tris = []
    for n, p in enumerate((0, 1, 2, -1, -2, 3, 0, 1)):
        a, b = 2.0 ** p, 2.0 ** -p
        tri = np.float32([[0, 0, 0], [a, 0, 0], [0, b, 0]]) + np.float32([3 * n, n, -n])
        tris.append(np.roll(tri, n % 3, 0))                     # the right angle moves to corner n % 3
    return np.concatenate(tris).astype(np.float32), np.arange(24, dtype=np.int32).reshape(8, 3)


def degenerate():
    """12 faces: sound ones among a collinear face, a face repeating a vertex, indices out of range (too large, negative, and one only int64 holds), a NaN and an
    infinite vertex, and a face of coordinates near 1e20.  Finite float32 coordinates cannot overflow S in float64 (|c| < 2^258, S < 2^518); an infinite one is
    what makes S not finite.  The 1e20 face (S near 1e80) drives the chosen j far down the ladder and leaves the others at KMIN."""
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 3], [np.nan, 1, 1], [np.inf, 0, 0], [1e20, 0, 0], [0, 1e20, 0], [0.5, 0.5, 0.5]])
    f = np.int64([[0, 1, 2], [0, 1, 3], [0, 1, 1], [0, 1, 10], [0, -1, 2], [0, 1, 2 ** 40 + 2], [0, 5, 2], [0, 6, 2], [0, 7, 8], [1, 2, 4], [4, 9, 3], [2, 4, 0]])
    return v, f


def ties():
    """face 0: l0 == l1 > l2 (corner 0, the first maximum); face 1: l1 == l2 > l0 (corner 1); face 2: equilateral in exact arithmetic (corner 0);
    face 3: l2 alone is the longest (corner 2)"""
    v = np.float32([[0, 0, 0], [1, 0, 0], [0.5, 1, 0],
                    [0.5, 1, 1], [0, 0, 1], [1, 0, 1],
                    [1, 0, 2], [0, 1, 2], [0, 0, 3],
                    [0, 0, 4], [3, 0, 4], [1, 0.5, 4]])
    return v, np.arange(12, dtype=np.int32).reshape(4, 3)


def dip():
    """7 right triangles with unit legs (S = 1) and one with legs 1 and 0.75 (S = 0.5625) at R = 16, where the texel sum is NOT monotone in j: up to j = 20 all
    are of class 2 (4 cells, 64 texels); at j = 21 the seven are of class 3 and the small one still of class 2 (4 * 64 + 16 = 272 > 256: no fit); at j = 22 it
    joins them in the free half of their fourth cell (256: fits again), until j = 29 sends the seven to class 4."""
    v, f = equal_areas(8)
    v = (np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])[None] + v.reshape(8, 3, 3)[:, :1] * 2).astype(np.float32)
    v[5, 2, 1] -= 0.25
    return v.reshape(-1, 3), f


CASES = [("dip", 8, 16), ("soup", 1, 4), ("soup", 2, 4), ("soup", 3, 16), ("soup", 64, 64), ("soup", 65, 64), ("equal", 65, 64), ("equal", 2, 16), ("soup", 1, 512),
         ("threshold", 8, 16), ("degenerate", 12, 16), ("degenerate", 12, 64), ("ties", 4, 16)]
LARGE_CASES = [("soup", 262401, 2048), ("soup", 1023, 512), ("soup", 4099, 512), ("equal", 1023, 512), ("soup", 65, 512), ("degenerate", 12, 512)]          # the device tests add these


def mesh(kind, F):
    v, f = {"soup": lambda: soup(F, seed=F), "equal": lambda: equal_areas(F), "threshold": threshold_triangles, "degenerate": degenerate, "ties": ties, "dip": dip}[kind]()
    assert f.shape == (F, 3)
    return v, f


# -------------------------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("kind, F, res", CASES + [("soup", 1023, 128)])
def test_atlas_properties(kind, F, res):
    v, f = mesh(kind, F)
    vt, ft, rep = A.area_atlas_ref(v, f, res)
    assert vt.shape == (3 * F, 2) and vt.dtype == np.float32 and ft.dtype == np.int32 and np.array_equal(ft, np.arange(3 * F).reshape(F, 3))
    assert vt.min() >= 0.0 and vt.max() <= 1.0
    assert np.array_equal(vt * res * 4, np.rint(vt * res * 4))                                       # quarter texels, exactly
    total = np.zeros((res, res), np.int32)
    for face in range(F):                                                                            # each face ALONE: the lowest-index rule cannot hide an overlap
        count, _ = R.coverage(vt, ft[face:face + 1], res)
        assert count.max() == 1 and count.sum() >= 1, face                                           # it covers a texel centre
        total += count
    assert total.max() == 1                                                                          # pairwise disjoint
    # the chosen step fits, the next does not
    S, corner = A.measure(v, f)
    kmax = res.bit_length() - 1
    assert A.fits(S, rep["j"], res, kmax) and (rep["j"] == A.JMAX or not A.fits(S, rep["j"] + 1, res, kmax))
    k, hist, at_min, at_max = A.classes(S, rep["j"], kmax)
    assert rep["histogram"] == hist.tolist() and sum(rep["histogram"]) == F and not any(rep["histogram"][:A.KMIN])
    assert rep["used"] == A.texels_needed(hist) / res ** 2 <= 1.0 and rep["D_j"] == A.density(rep["j"])
    assert (rep["clamped_min"], rep["clamped_max"]) == (at_min, at_max) and at_min >= int((S == 0).sum())
    # the chart of a face of class k lies inside one 2^k x 2^k cell of the grid of such cells
    tex = vt.reshape(F, 3, 2).astype(np.float64) * res
    size = 2.0 ** k.astype(np.float64)
    cell = np.floor(tex.min(1) / size[:, None])
    assert np.array_equal(cell, np.floor(np.nextafter(tex.max(1), 0) / size[:, None]))
    # the longest edge is on the diagonal: the vertex opposite it sits at the right angle, where both of its edges run along an axis
    for face in range(F):
        c = int(corner[face])
        a, b = tex[face, (c + 1) % 3] - tex[face, c], tex[face, (c + 2) % 3] - tex[face, c]
        assert a[1] == 0 and b[0] == 0 and a[0] * b[1] > 0, face                                     # P1 - P0 along x, P2 - P0 along y, winding kept (a x b > 0)


def test_unclamped_faces_get_half_to_twice_their_share():
    v, f = soup(200, seed=3, octaves=6)
    vt, ft, rep = A.area_atlas_ref(v, f, 512)
    S, _ = A.measure(v, f)
    k = A.classes(S, rep["j"], 9)[0].astype(np.float64)
    p = S * rep["D_j"]
    free = (p > 64.0) & (p <= 4 * 16.0 ** 9)                                                         # faces whose class neither limit changed
    assert free.sum() == 200 - rep["clamped_min"] - rep["clamped_max"] >= 150
    half_cell = 0.5 * 4.0 ** k[free]                                                                 # texels of half a cell
    want = np.sqrt(rep["D_j"]) * np.sqrt(S[free]) / 2                                                # sqrt(D_j) * area
    assert (half_cell >= want * 0.4999999).all() and (half_cell < want * 2.000001).all()             # 4 16^k >= S D > 4 16^(k - 1)  <=>  want / 2 <= 4^k / 2 < 2 want


def test_class_rule_at_equality():
    v, f = threshold_triangles()
    S, corner = A.measure(v, f)
    assert np.array_equal(S, np.ones(8)) and corner.tolist() == [n % 3 for n in range(8)]
    vt, ft, rep = A.area_atlas_ref(v, f, 16)
    assert rep["j"] == 28 and rep["D_j"] == 2.0 ** 14 and S[0] * rep["D_j"] == 4 * 16 ** 3           # equality, exactly
    assert rep["histogram"] == [0, 0, 0, 8, 0] and rep["used"] == 1.0                                # class 3, not 4
    assert A.classes(S, 28, 4)[0].tolist() == [3] * 8 and A.classes(S, 29, 4)[0].tolist() == [4] * 8
    # the clamp counters at their own equalities: 64 >= S D counts as clamped at KMIN, 4 16^KMAX >= S D does not count as clamped at KMAX
    assert A.classes(np.float64([64.0, 65.0, 4 * 16.0 ** 4, 4 * 16.0 ** 4 + 1, 0.0]), 0, 4)[2:] == (2, 1)


def test_the_stated_bisection_is_the_contract_where_the_sum_dips():
    """two faces share a cell, so the texel sum is not monotone in j (dip()); what holds is what the bisection guarantees, and the bisection is stated exactly"""
    v, f = dip()
    S, _ = A.measure(v, f)
    assert sorted(S.tolist()) == [0.5625] + [1.0] * 7
    fit = [A.fits(S, j, 16, 4) for j in range(15, 35)]
    assert fit == [True] * 6 + [False] + [True] * 7 + [False] * 6                                    # fits up to 20, not at 21, again from 22 to 28
    need = [A.texels_needed(A.classes(S, j, 4)[1]) for j in (20, 21, 22)]
    assert need == [64, 272, 256]                                                                    # the sum goes DOWN from j = 21 to 22
    lo, hi, mids = A.JMIN, A.JMAX + 1, []                                                            # the bisection, step by step
    while hi - lo > 1:
        mids.append((lo + hi) // 2)
        lo, hi = (mids[-1], hi) if A.fits(S, mids[-1], 16, 4) else (lo, mids[-1])
    assert mids == [0, 400, 200, 100, 50, 25, 37, 31, 28, 29] and lo == A.choose_j(S, 16, 4) == A.area_atlas_ref(v, f, 16)[2]["j"] == 28
    assert A.fits(S, 28, 16, 4) and not A.fits(S, 29, 16, 4)


def test_longest_edge_and_ties():
    v, f = ties()
    S, corner = A.measure(v, f)
    assert corner.tolist() == [0, 1, 0, 2] and (S > 0).all()
    v, f = degenerate()
    S, corner = A.measure(v, f)
    assert not S[1:8].any() and not corner[1:8].any() and (S[[0, 8, 9, 10, 11]] > 0).all() and np.isfinite(S).all()          # faces 1 .. 7 are the unsound ones
    assert S[0] == 1.0 and 1e79 < S[8] < 1e81


def test_capacity():
    from iris_amd._lib import IrisError
    from iris_amd.utils.texture import area_atlas, atlas_min_res, check_atlas_inputs
    v, f = equal_areas(33)
    vt, ft, rep = A.area_atlas_ref(v[:96], f[:32], 16)                                               # 16 cells of 4 x 4: full
    assert rep["histogram"] == [0, 0, 32, 0, 0] and rep["used"] == 1.0
    assert check_atlas_inputs(v[:96], f[:32], 16) == (16, 4, 96, 32)
    with pytest.raises(A.AtlasError, match="32"):
        A.area_atlas_ref(v, f, 16)
    with pytest.raises(IrisError, match=r"smallest tex_res that holds them is 32\b"):
        area_atlas(v, f, 16)
    assert [atlas_min_res(F) for F in (1, 2, 3, 32, 33, 128, 129)] == [4, 4, 8, 16, 32, 32, 64] == [A.min_res(F) for F in (1, 2, 3, 32, 33, 128, 129)]
    with pytest.raises(A.AtlasError, match="lowest density"):                                        # one face near the top of float32 beside an ordinary one
        A.area_atlas_ref(np.float32([[0, 0, 0], [3e38, 0, 0], [0, 3e38, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[0, 1, 2], [0, 3, 4], [0, 4, 3]]), 16)


@pytest.mark.parametrize("res", [4, 16, 512])
def test_one_face_fills_the_texture(res):
    v, f = soup(1, seed=9)
    vt, ft, rep = A.area_atlas_ref(v, f, res)
    _, corner = A.measure(v, f)
    P = np.float64([[0.25, 0.25], [res - 0.5, 0.25], [0.25, res - 0.5]]) / res
    assert np.array_equal(vt[(int(corner[0]) + np.arange(3)) % 3], P.astype(np.float32))
    assert rep["j"] == A.JMAX and rep["histogram"][-1] == 1 and rep["used"] == 1.0 and rep["clamped_max"] == 1


def test_refused_sizes_raise_on_the_host(tmp_path):
    """(no device here: an IrisError that is not 'needs a GPU' came from the host checks)"""
    from iris_amd._lib import IrisError
    from iris_amd.utils import export as E, texture as T
    v, f = soup(2, seed=1)
    for res in ((8, 16), (16, 8), (8, 8, 8), 12, 100, 2, 1, 0, -4, 16384, 7.5, True, "16"):
        with pytest.raises(IrisError, match="tex_res"):
            T.area_atlas(v, f, res)
        with pytest.raises(A.AtlasError):
            A.area_atlas_ref(v, f, res)
    assert T.check_atlas_inputs(v, f, (8, 8))[:2] == (8, 3) and A.check_res((8, 8)) == (8, 3) and T.check_atlas_inputs(v, f, 8192)[:2] == (8192, 13)
    for bad_v, bad_f in ((v[:, :2], f), (v.astype(np.int32), f), (v, f.astype(np.float32)), (v, f[:, :2]), (v, f[:0])):
        with pytest.raises(IrisError, match="area_atlas"):
            T.area_atlas(bad_v, bad_f, 16)
    for n in (5, -1, 1.5, True, None):
        with pytest.raises(IrisError, match="dilate"):
            T.check_dilate(n)
        with pytest.raises(IrisError, match="dilate"):
            T.bake_textures(lambda x: None, np.float32([[0.1, 0.1], [0.9, 0.1], [0.1, 0.9]]), np.int32([[0, 1, 2]]), np.eye(3, dtype=np.float32), np.int32([[0, 1, 2]]), 8,
                            dilate=n)
    assert [T.check_dilate(n) for n in range(5)] == list(range(5))
    for n in ("5", "-1"):                                                                            # the command line, before the mesh is even read
        with pytest.raises(IrisError, match="dilate"):
            E.main(["--mesh", str(tmp_path / "none.obj"), "--emitter_path", str(tmp_path), "--dir_save", str(tmp_path / "out"), "--atlas", "area", "--dilate", n])
    assert not os.path.exists(tmp_path / "out")
    with pytest.raises(A.AtlasError):
        A.dilate_ref(np.zeros((2, 2), np.int32), np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 3), np.uint8), 5)


def test_cli_knows_the_area_atlas(tmp_path):
    from iris_amd._lib import IrisError
    from iris_amd.utils import export as E
    from test_stage_setup_cpu import PARSERS, _table
    cli = E.build_parser(area_atlas=True)                                                            # the parser main() runs
    args = cli.parse_args(["--atlas", "area", "--dilate", "2"])
    assert args.atlas == "area" and args.dilate == 2 and cli.parse_args([]).dilate == 0 and cli.parse_args([]).atlas == "auto"
    # its whole option table: the first version's, which tests/test_stage_setup_cpu.py pins for build_parser(), with one more choice and one more option
    want = dict(PARSERS["export"], atlas=(("--atlas",), str, "auto", ("auto", "files", "grid", "area"), False, None), dilate=(("--dilate",), int, 0, None, False, None))
    assert _table(cli) == want and _table(E.build_parser()) == PARSERS["export"]
    with pytest.raises(SystemExit):                                                                  # the first version's parser knows neither
        E.build_parser().parse_args(["--atlas", "area"])
    with pytest.raises(IrisError, match="--atlas area"):                                            # auto still fails without files, and now names the way out
        E.load_atlas("auto", str(tmp_path), 1, 16)
    with pytest.raises(IrisError, match="pass v and f"):
        E.load_atlas("area", str(tmp_path), 1, 16)
    with open(tmp_path / "m.obj", "w") as fh:
        fh.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with pytest.raises(IrisError, match="tex_res"):                                                  # a size the area atlas refuses: before the device is opened
        E.main(["--mesh", str(tmp_path / "m.obj"), "--emitter_path", str(tmp_path), "--dir_save", str(tmp_path / "out"), "--atlas", "area", "--tex_res", "48"])
    assert not os.path.exists(tmp_path / "out" / "vt.npy")


# ---------------------------------------------------------------------------------------------------------------------------------- dilation
def _images(H, W, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 256, (H, W, 3), dtype=np.uint8), rng.integers(1, 256, (H, W, 3), dtype=np.uint8)


def test_dilation_restatement_on_simple_masks():
    H, W = 6, 7
    a, m = _images(H, W)
    for n in range(5):
        for ids in (np.full((H, W), -1, np.int32), np.zeros((H, W), np.int32)):                      # nothing to take from; nothing to fill
            da, dm = A.dilate_ref(ids, a, m, n)
            assert np.array_equal(da, a) and np.array_equal(dm, m)
    ids = np.full((H, W), -1, np.int32); ids[1, 5] = 3                                               # one covered texel: a clipped (2 n + 1)^2 block takes its bytes
    for n in range(5):
        da, dm = A.dilate_ref(ids, a, m, n)
        block = np.zeros((H, W), bool); block[max(0, 1 - n):1 + n + 1, max(0, 5 - n):5 + n + 1] = True
        assert (da[block] == a[1, 5]).all() and (dm[block] == m[1, 5]).all() and np.array_equal(da[~block], a[~block]) and np.array_equal(dm[~block], m[~block])
    rr, cc = np.mgrid[:H, :W]
    ids = np.where((rr + cc) % 2 == 0, 7, -1).astype(np.int32)                                       # checkerboard: four neighbours at distance 1; the smallest row
    da, dm = A.dilate_ref(ids, a, m, 2)                                                              # wins (the one above), on row 0 the one to the left
    for r in range(H):
        for c in range(W):
            src = (r, c) if ids[r, c] >= 0 else (r - 1, c) if r > 0 else (r, c - 1)
            assert np.array_equal(da[r, c], a[src]) and np.array_equal(dm[r, c], m[src]), (r, c)
    ids = np.full((5, 5), -1, np.int32); ids[0, 4] = ids[4, 0] = ids[2, 4] = 1                       # distance before row: (2, 2) takes (2, 4) at 4, not (0, 4) at 8
    a, m = _images(5, 5, 1)
    da, _ = A.dilate_ref(ids, a, m, 2)
    assert np.array_equal(da[2, 2], a[2, 4]) and np.array_equal(da[2, 1], a[4, 0]) and np.array_equal(A.dilate_ref(ids, a, m, 1)[0][2, 2], a[2, 2])


# ------------------------------------------------------------------------------------------------------------------------------ declarations
def test_atlas_entry_points_are_declared_exported_and_bound():
    from iris_amd import _lib as L
    assert os.path.exists(L.LIB_PATH), "libiris_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    exported = set(re.findall(r" T (iris_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH]).decode()))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "iris_hip.h")).read(), flags=re.S)
    for name in ("iris_atlas_measure", "iris_atlas_density", "iris_atlas_classes", "iris_atlas_place", "iris_texture_dilate"):
        m = re.search(r"IRIS_API\s+(?:int|double)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name + " is not declared in include/iris_hip.h"
        assert len(m.group(1).split(",")) == len(L.PROTOTYPES[name]) and name in exported, name
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name]
    # the ladder is a host function: the library's steps are the restatement's, bit for bit, and 0 outside the range
    lib = L.lib()
    assert all(lib.iris_atlas_density(j) == A.density(j) for j in range(A.JMIN, A.JMAX + 1))
    assert lib.iris_atlas_density(A.JMIN - 1) == 0.0 and lib.iris_atlas_density(A.JMAX + 1) == 0.0 and lib.iris_atlas_density(1) == 1.4142135623730951
    src = open(os.path.join(REPO, "iris_amd", "csrc", "iris_atlas.h")).read()
    assert "atomicAdd(hist" in src and not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", src)          # integer atomics only
    assert "sqrt" not in src.split("#pragma once")[1]                                                        # no square root anywhere
