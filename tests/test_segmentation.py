"""The segmentation fusion on the GPU (iris_amd/csrc/iris_labels.h, utils/segmentation.py, python -m iris_amd.fuse_segmentation) on the box scene of
tests/golden/bake_box.npz (14 triangles; 2, 3 the ceiling, 12, 13 the light).

Every expectation is the numpy restatement of tests/segmentation_ref.py over ray_intersect's own hits, and every comparison is == on integers.  Views are
37 x 53: 1961 pixels, a multiple of neither 64 nor the block size."""
import os

import numpy as np
import pytest
import torch

import segmentation_ref as ref
from conftest import golden
from test_prebake_fused import CEILING_AND_LIGHT, dev, hits_of, look, rays_of, synth_view
from test_segmentation_cpu import H, N_CAPTURES, W, write_real_scene

pytestmark = pytest.mark.gpu

HW = (H, W)
N = H * W
F = 14
UP = look((2.0, 1.5, 0.4), (1.0, 0.3, 1.0), H, W, up=(0.0, 1.0, 0.0))           # half a wall, half the open box's missing ceiling
HIST_DTYPES = [torch.int32] + ([torch.uint32] if hasattr(torch, "uint32") else [])


@pytest.fixture(scope="module")
def box():
    from iris_amd.utils.path_tracing import Scene
    g = golden("bake_box.npz")
    return Scene(g["verts"], g["faces"], device=dev())


@pytest.fixture(scope="module")
def open_box():
    from iris_amd.utils.path_tracing import Scene
    g = golden("bake_box.npz")
    return Scene(g["verts"], g["faces"][[i for i in range(F) if i not in CEILING_AND_LIGHT]], device=dev())


_HITS = {}


def hits(scene, view):
    """(idx, valid) of ray_intersect over the view's pixel-centre rays, computed once per (scene, view) and left unchanged"""
    key = (id(scene), view["kind"], view["c2w"].tobytes())
    if key not in _HITS:
        _, idx, valid = hits_of(scene, rays_of(view, HW))
        idx.setflags(write=False); valid.setflags(write=False)
        _HITS[key] = (idx, valid)
    return _HITS[key]


def ray_kw(view, form):
    """the ray arguments of a call: the camera, or explicit rays with a row stride of 12"""
    if form == "camera":
        return {"camera": view, "img_hw": HW}
    rays = rays_of(view, HW)
    return {"rays": torch.cat([rays, torch.full((N, 6), 7.0, device=dev())], -1)}


def per_lane(fn):
    """fn() under iris_debug_set("pool_combine", 0)"""
    from iris_amd import _lib as L
    L.debug_set("pool_combine", 0)
    try:
        return fn()
    finally:
        L.debug_set("pool_combine", -1)


def voted(scene, views, maps, n_labels, form="camera", combine=True, dtype=torch.int32):
    from iris_amd.utils.segmentation import vote_view
    hist = torch.zeros(scene.n_triangles, n_labels, dtype=torch.int32, device=dev()).view(dtype)

    def run():
        for view, m in zip(views, maps):
            assert vote_view(scene, hist, m, **ray_kw(view, form)) is None
    run() if combine else per_lane(run)
    return hist.view(torch.int32).cpu().numpy().view(np.uint32).astype(np.int64)


def expected(scene, views, maps, n_labels):
    hist = np.zeros((scene.n_triangles, n_labels), np.int64)
    for view, m in zip(views, maps):
        idx, valid = hits(scene, view)
        ref.vote(idx, valid, m.cpu().numpy(), scene.n_triangles, n_labels, hist)
    return hist


def id_maps(n_views, top, seed=5):
    g = np.random.default_rng(seed)
    return [torch.from_numpy(g.integers(0, top + 1, N).astype(np.float32)).to(dev()) for _ in range(n_views)]


# ---- vote_view
@pytest.mark.parametrize("combine", [True, False], ids=["combined", "per_lane"])
@pytest.mark.parametrize("kind,form", [("real", "camera"), ("synthetic", "camera"), ("real", "rays12")])
def test_three_views_vote_into_one_histogram(box, kind, form, combine):
    views = [synth_view(kind, H, W, v) for v in range(3)]
    maps = id_maps(3, 6)
    got, want = voted(box, views, maps, 7, form, combine), expected(box, views, maps, 7)
    assert want.sum() > 2 * N and (want.sum(1) > 0).sum() >= 8                    # (the views see most of the room)
    assert np.array_equal(got, want)
    assert not got[:, 0].any()                                                    # column 0 stays zero: the maps hold zeros, nothing counts them


@pytest.mark.parametrize("combine", [True, False], ids=["combined", "per_lane"])
def test_misses_vote_for_nothing(open_box, combine):
    idx, valid = hits(open_box, UP)
    assert 100 < valid.sum() < N - 100
    maps = id_maps(1, 6, seed=6)
    got = voted(open_box, [UP], maps, 7, combine=combine)
    assert np.array_equal(got, expected(open_box, [UP], maps, 7)) and got.sum() == (valid & (maps[0].cpu().numpy() >= 1)).sum()


@pytest.mark.parametrize("combine", [True, False], ids=["combined", "per_lane"])
def test_what_is_no_id_is_dropped(box, combine):
    n_labels = 7
    view = synth_view("real", H, W, 1)
    cycle = np.array([0, -3, np.nan, n_labels, n_labels + 7, 2.9, 3.0, 1, 6, -0.5, np.inf, 2], np.float32)
    m = cycle[np.arange(N) % len(cycle)]
    idx, valid = hits(box, view)
    got = voted(box, [view], [torch.from_numpy(m).to(dev())], n_labels, combine=combine)
    assert np.array_equal(got, expected(box, [view], [torch.from_numpy(m)], n_labels))
    # the same said directly: per triangle, 2.9 and 2 count as 2, 3.0 as 3, and only ids 1, 2, 3, 6 are ever counted
    for t in range(F):
        mine = m[valid & (idx == t)]
        assert got[t, 2] == (mine == np.float32(2.9)).sum() + (mine == 2).sum() and got[t, 3] == (mine == 3).sum()
    assert not got[:, [0, 4, 5]].any() and got.sum() == np.isin(m[valid], np.array([2.9, 3.0, 1, 6, 2], np.float32)).sum()


def test_a_uint8_map_votes_as_its_float_copy(box):
    view = synth_view("synthetic", H, W, 2)
    u8 = torch.from_numpy(np.random.default_rng(8).integers(0, 256, N).astype(np.uint8)).to(dev())
    u8[::5] = 3
    a, b = voted(box, [view], [u8.reshape(H, W)], 7), voted(box, [view], [u8.float()], 7)
    assert np.array_equal(a, b) and np.array_equal(a, expected(box, [view], [u8], 7)) and a.sum() > N // 6


@pytest.mark.parametrize("combine", [True, False], ids=["combined", "per_lane"])
@pytest.mark.parametrize("n_labels", [2, 65, 130])
def test_rows_beside_and_beyond_one_wave(box, n_labels, combine):
    """1 + (pixel index mod (n_labels - 1)): neighbouring lanes at one triangle carry different ids, so a wave holds up to 64 distinct keys"""
    view = synth_view("real", H, W, 0)
    m = torch.from_numpy((1 + np.arange(N) % (n_labels - 1)).astype(np.float32)).to(dev())
    for dtype in HIST_DTYPES:
        got = voted(box, [view], [m], n_labels, combine=combine, dtype=dtype)
        assert np.array_equal(got, expected(box, [view], [m], n_labels)) and got.sum() == hits(box, view)[1].sum()


def test_bad_arguments_are_refused(box):
    from iris_amd._lib import IrisError
    from iris_amd.utils.segmentation import label_view, triangle_labels, vote_view
    view = synth_view("real", H, W, 0)
    m = torch.ones(N, device=dev())
    good = torch.zeros(F, 7, dtype=torch.int32, device=dev())
    for hist, labels in ((torch.zeros(F, 7, dtype=torch.int64, device=dev()), m), (torch.zeros(F + 1, 7, dtype=torch.int32, device=dev()), m),
                         (torch.zeros(F, 14, dtype=torch.int32, device=dev())[:, ::2], m), (torch.zeros(F, 7, dtype=torch.int32), m),
                         (good, m[:-1]), (good, m.long()), (good, m.cpu())):
        with pytest.raises(IrisError):
            vote_view(box, hist, labels, camera=view, img_hw=HW)
    with pytest.raises(IrisError):
        vote_view(box, good, m)                                                   # neither camera nor rays
    with pytest.raises(IrisError):
        triangle_labels(good.float())
    with pytest.raises(IrisError):
        label_view(box, torch.zeros(F + 1, dtype=torch.int32, device=dev()), camera=view, img_hw=HW)
    with pytest.raises(IrisError):
        label_view(box, torch.zeros(F, dtype=torch.int32, device=dev()), camera=view, img_hw=HW, dtype=torch.int32)
    assert not good.any()


# ---- triangle_labels
def argmax_rows(n_rows, n_labels, seed):
    """(n_rows, n_labels) uint32 with counts 0..3 everywhere (ties between lanes and, from 66 columns on, within a lane's stride), and on top of them, by
    row % 6: a unique maximum in the first / the last / a middle column; two equal maxima 64 columns apart (one lane's stride) where the row is that
    wide, else side by side; an all-zero row; 2^31 + 5 in a higher column than 2^31 - 1.  Column 0 holds 2^32 - 1: it must not be read."""
    g = np.random.default_rng(seed)
    h = g.integers(0, 4, (n_rows, n_labels)).astype(np.uint32)
    last = n_labels - 1
    for r in range(n_rows):
        kind = r % 6
        if kind == 0:
            h[r, 1] = 9
        elif kind == 1:
            h[r, last] = 9
        elif kind == 2:
            h[r, (1 + last) // 2] = 9
        elif kind == 3:
            a = 1 + r % max(1, last - 64) if last > 64 else max(1, last - 1)
            h[r, a] = 7; h[r, min(last, a + 64) if last > 64 else last] = 7
        elif kind == 4:
            h[r] = 0
        else:
            h[r, max(1, last // 2)] = 2 ** 31 - 1; h[r, last] = 2 ** 31 + 5
    h[:, 0] = 2 ** 32 - 1
    return h


@pytest.mark.parametrize("n_rows", [1, 5, 259])
@pytest.mark.parametrize("n_labels", [2, 64, 65, 130])
def test_triangle_labels(n_labels, n_rows):
    from iris_amd.utils.segmentation import triangle_labels
    for seed in range(6 if n_rows == 1 else 1):                                   # (one row: each of the six kinds in turn)
        h = np.roll(argmax_rows(max(n_rows, 6), n_labels, seed), -seed, 0)[:n_rows] if n_rows == 1 else argmax_rows(n_rows, n_labels, seed)
        want = ref.triangle_labels(h)
        for dtype in HIST_DTYPES:
            t = torch.from_numpy(h.view(np.int32)).to(dev()).view(dtype)
            got = triangle_labels(t)
            assert got.dtype == torch.int32 and tuple(got.shape) == (n_rows,)
            assert np.array_equal(got.cpu().numpy(), want), (n_labels, n_rows, seed, dtype)
    if n_rows == 259:
        kinds = np.arange(n_rows) % 6
        assert (want[kinds == 4] == 0).all() and (want[kinds == 5] == n_labels - 1).all() and (want[kinds == 0] == 1).all()
        if n_labels == 130:
            assert all(want[r] == 1 + r % 65 and h[r, want[r]] == h[r, want[r] + 64] == 7 for r in np.nonzero(kinds == 3)[0])     # the lower of one lane's two


# ---- label_view
@pytest.mark.parametrize("miss", [0, -1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["float32", "uint8"])
@pytest.mark.parametrize("form", ["camera", "rays12"])
def test_label_view(box, open_box, dtype, miss, form):
    from iris_amd.utils.segmentation import label_view
    low = (lambda a: a & 0xFF) if dtype == torch.uint8 else (lambda a: a)
    for scene, view in ((box, synth_view("real", H, W, 0)), (box, synth_view("synthetic", H, W, 1)), (open_box, UP)):
        idx, valid = hits(scene, view)
        table = 301 + np.arange(scene.n_triangles)                                # (no entry equals a miss value, as a number or as a low byte)
        most = np.bincount(idx[valid]).argmax()
        table[most] = 300                                                         # 300 -> 44 as uint8
        got = label_view(scene, torch.from_numpy(table.astype(np.int32)).to(dev()), miss=miss, dtype=dtype, **ray_kw(view, form))
        assert got.dtype == dtype and tuple(got.shape) == (N,)
        got = got.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, low(ref.label_view(idx, valid, table, miss)))
        assert np.array_equal(got == low(np.int64(miss)), ~valid)                 # the misses carry the miss value and nothing else does
        assert (got[valid & (idx == most)] == (44 if dtype == torch.uint8 else 300)).all() and (got == (44 if dtype == torch.uint8 else 300)).sum() > 100
        if scene is open_box:
            assert 100 < (~valid).sum() < N - 100


# ---- view shapes and the empty batch, for both label kernels
@pytest.mark.parametrize("combine", [True, False], ids=["combined", "per_lane"])
@pytest.mark.parametrize("hw", [(1, 1), (64, 1)])
def test_view_shapes(box, hw, combine):
    """a single lane; and exactly one wave, with nothing behind it in the vote's workgroup-bounded loop"""
    from iris_amd.utils.segmentation import label_view, vote_view
    n, n_labels = hw[0] * hw[1], 7
    view = synth_view("real", *hw, 1)
    _, idx, valid = hits_of(box, rays_of(view, hw))
    assert valid.any()
    m = torch.from_numpy((1 + np.arange(n) % (n_labels - 1)).astype(np.float32)).to(dev())
    table = 301 + np.arange(F)

    def run():
        hist = torch.zeros(F, n_labels, dtype=torch.int32, device=dev())
        assert vote_view(box, hist, m, camera=view, img_hw=hw) is None
        return hist.cpu().numpy().astype(np.int64), label_view(box, torch.from_numpy(table.astype(np.int32)).to(dev()), camera=view, img_hw=hw, miss=-1)
    hist, painted = run() if combine else per_lane(run)
    assert np.array_equal(hist, ref.vote(idx, valid, m.cpu().numpy(), F, n_labels)) and hist.sum() == valid.sum()
    assert painted.dtype == torch.float32 and tuple(painted.shape) == (n,)
    assert np.array_equal(painted.cpu().numpy().astype(np.int64), ref.label_view(idx, valid, table, -1))


def test_empty_ray_batch_is_a_no_op(box):
    from iris_amd.utils.segmentation import label_view, vote_view
    rays = torch.empty(0, 6, device=dev())
    before = torch.arange(1, 1 + F * 7, dtype=torch.int32).reshape(F, 7)
    hist = before.to(dev())
    assert vote_view(box, hist, torch.empty(0, device=dev()), rays=rays) is None
    assert torch.equal(hist.cpu(), before)
    table = torch.zeros(F, dtype=torch.int32, device=dev())
    for dtype in (torch.float32, torch.uint8):
        out = label_view(box, table, rays=rays, dtype=dtype)
        assert tuple(out.shape) == (0,) and out.dtype == dtype


# ---- fuse
TRUTH = 1 + np.arange(F) % 5


def noisy_maps(scene, views):
    """each view's map: the truth at its hit triangle (0 on a miss), every third pixel set to another id in range"""
    maps = []
    for view in views:
        idx, valid = hits(scene, view)
        m = np.where(valid, TRUTH[np.where(valid, idx, 0)], 0)
        m[::3] = m[::3] % 5 + 1
        maps.append(m.astype(np.float32))
    return maps


def restated_fusion(scene, views, maps, n_labels):
    hist = np.zeros((scene.n_triangles, n_labels), np.int64)
    for view, m in zip(views, maps):
        ref.vote(*hits(scene, view), m, scene.n_triangles, n_labels, hist)
    labels = ref.triangle_labels(hist)
    return hist, labels, [ref.label_view(*hits(scene, view), labels, 0) for view in views]


def test_fuse_on_three_views(box):
    from iris_amd.utils.segmentation import fuse
    views = [synth_view("real", H, W, v) for v in range(3)]
    maps = noisy_maps(box, views)
    seg_num = int(max(m.max() for m in maps))
    assert seg_num == TRUTH.max() == 5                                            # the largest id in the files is some triangles' true label
    upload = lambda ms: [torch.from_numpy(np.asarray(m, np.float32)).to(dev()) for m in ms]
    tri_label, fused = fuse(box, views, HW, upload(maps), seg_num + 1)
    hist, want_labels, want_maps = restated_fusion(box, views, maps, seg_num + 1)
    assert tri_label.dtype == torch.int32 and np.array_equal(tri_label.cpu().numpy(), want_labels)
    assert len(fused) == 3 and all(f.dtype == torch.float32 and np.array_equal(f.cpu().numpy(), w) for f, w in zip(fused, want_maps))
    seen = hist.sum(1) >= 8
    assert seen.sum() >= 6 and seen[TRUTH == 5].any() and np.array_equal(want_labels[seen], TRUTH[seen])      # the vote repairs the noise
    again_label, again = fuse(box, views, HW, fused, seg_num + 1)                 # a fixed point
    assert torch.equal(again_label, tri_label) and all(torch.equal(a, b) for a, b in zip(again, fused))
    # rows as wide as the reference's: the largest id never wins
    compat_label, compat = fuse(box, views, HW, upload(maps), seg_num)
    _, want_compat, want_compat_maps = restated_fusion(box, views, maps, seg_num)
    assert np.array_equal(compat_label.cpu().numpy(), want_compat) and all(np.array_equal(f.cpu().numpy(), w) for f, w in zip(compat, want_compat_maps))
    differs = compat_label.cpu().numpy() != tri_label.cpu().numpy()
    assert np.array_equal(differs[seen], (TRUTH == 5)[seen]) and differs[seen].any() and not (compat_label.cpu().numpy() == 5).any()


# ---- the command line
def test_the_command_line_on_a_real_layout_scene(box, tmp_path, capsys):
    from iris_amd import fuse_segmentation as fs
    from iris_amd.utils import cameras
    from iris_amd.utils.dataset.files import load_training_files
    from iris_amd.utils.exr import read_exr
    from iris_amd.utils.segmentation import fuse
    from iris_amd.utils.texture import write_png
    os.makedirs(tmp_path / "probe")
    probe = write_real_scene(tmp_path / "probe", [np.zeros(HW)] * N_CAPTURES)     # (camera files only: the views the maps are made for)
    ids, views = fs.load_split("real", str(probe), "all", HW)
    maps = noisy_maps(box, views)
    assert int(max(m.max() for m in maps)) == 5
    os.makedirs(tmp_path / "run")
    scene = write_real_scene(tmp_path / "run", [m.reshape(HW) for m in maps])
    tri_label, fused = fuse(box, views, HW, [torch.from_numpy(m).to(dev()) for m in maps], 6)
    fused = [f.cpu().numpy().reshape(HW) for f in fused]
    before = {n: open(scene / "segmentation" / n, "rb").read() for n in sorted(os.listdir(scene / "segmentation"))}
    assert len(before) == N_CAPTURES

    # --output: written there, nothing renamed
    out = tmp_path / "fused"
    assert fs.cli(["--scene", str(scene), "--dataset", "real", "--output", str(out)]) == 0
    line = capsys.readouterr().out
    assert "12 views" in line and "14 triangles" in line and "n_labels 6" in line and "%d triangles labelled" % int((tri_label > 0).sum()) in line
    assert sorted(os.listdir(out)) == sorted(before)
    for i in ids:
        a = read_exr(str(out / ("%03d.exr" % i)))
        assert a.dtype == np.float32 and a.shape == (H, W, 3)
        assert np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 1], a[..., 2]) and np.array_equal(a[..., 0], fused[i])
    assert {n: open(scene / "segmentation" / n, "rb").read() for n in sorted(os.listdir(scene / "segmentation"))} == before
    assert not (scene / "segmentation-old").exists() and not (scene / "segmentation-new").exists()

    # the default: the folders swapped, and the trainers' loader reads the new files
    assert fs.cli(["--scene", str(scene), "--dataset", "real", "--compression", "none"]) == 0
    capsys.readouterr()
    assert {n: open(scene / "segmentation-old" / n, "rb").read() for n in sorted(os.listdir(scene / "segmentation-old"))} == before
    assert sorted(os.listdir(scene / "segmentation")) == sorted(before) and not (scene / "segmentation-new").exists()
    assert all(np.array_equal(read_exr(str(scene / "segmentation" / ("%03d.exr" % i)))[..., 2], fused[i]) for i in ids)
    os.makedirs(scene / "ldr" / "albedo"); os.makedirs(scene / "ldr" / "cam")
    train = cameras.real_split_ids(N_CAPTURES, "train")
    for i in train:
        write_png(scene / "ldr" / ("%03d_0001.png" % i), np.zeros((H, W, 3), np.uint8))
        write_png(scene / "ldr" / "albedo" / ("%03d_0001.png" % i), np.zeros((H, W, 3), np.uint8))
    np.save(scene / "ldr" / "cam" / "exposure.npy", np.ones(N_CAPTURES, np.float32))
    files = load_training_files("real", str(scene), "ldr")
    assert len(files["segmentation"]) == len(train) and all(np.array_equal(s, fused[i].reshape(-1)) for i, s in zip(train, files["segmentation"]))

    # --split train on the swapped scene: only the train captures are written, and the stage says so
    out2 = tmp_path / "train_only"
    assert fs.cli(["--scene", str(scene), "--dataset", "real", "--split", "train", "--output", str(out2)]) == 0
    assert "validation" in capsys.readouterr().out and sorted(os.listdir(out2)) == ["%03d.exr" % i for i in train]
