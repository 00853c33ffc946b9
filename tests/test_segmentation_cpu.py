"""The segmentation fusion without a GPU: the numpy restatement of its contract (tests/segmentation_ref.py) on a hand-written case and against a literal
transcription of the reference's flat scatter_add; the views of --split all on a `real` layout; and every refusal of python -m iris_amd.fuse_segmentation
(status 2, one line on stderr, before the device is opened)."""
import os

import numpy as np
import pytest

import segmentation_ref as ref
from conftest import golden

H, W = 37, 53                      # 1961 pixels: a multiple of neither 64 nor the block size
N_CAPTURES = 12                    # captures 0 and 10 validate (cameras.real_split_ids)


def capture_cameras(n=N_CAPTURES):
    """n distinct (origin, lookat, up) rows for cam.txt inside the box room of tests/golden/bake_box.npz (4 x 3 x 2.6, z up): horizontal looks around the
    room, the last two tilted"""
    cams = []
    for i in range(n):
        th = 2.0 * np.pi * i / n + 0.1
        origin = np.array([2.0 + 0.3 * np.cos(3 * th), 1.5 + 0.2 * np.sin(2 * th), 1.2 + 0.02 * i])
        at = np.array([np.cos(th), np.sin(th), 0.0])
        up = np.array([0.0, 0.0, 1.0])
        if i >= n - 2:                                  # looking up (towards the ceiling and the light) and down
            at = np.array([0.3 * np.cos(th), 0.3 * np.sin(th), 1.0 if i == n - 2 else -1.0])
            at /= np.linalg.norm(at)
            up = np.cross(at, np.array([-np.sin(th), np.cos(th), 0.0]))
        cams.append((origin, origin + at, up))
    return cams


def write_real_scene(root, seg_maps, hw=(H, W), faces=None):
    """a `real`-layout scene: the box mesh as scene.obj, cam.txt and K_list.txt for len(seg_maps) captures, no Image/000_0001.exr, and
    segmentation/{capture id:03d}.exr holding seg_maps[i] ((H, W) array) in three equal channels.  -> the scene's folder"""
    from iris_amd.utils.exr import write_exr
    g = golden("bake_box.npz")
    faces = g["faces"] if faces is None else faces
    scene = root / "scene"
    os.makedirs(scene / "segmentation")
    cams = capture_cameras(len(seg_maps))
    with open(scene / "cam.txt", "w") as fh:
        fh.write("%d\n" % len(cams) + "".join("%.9g %.9g %.9g\n" % tuple(row) for cam in cams for row in cam))
    with open(scene / "K_list.txt", "w") as fh:
        fh.write("%d\n" % len(cams) + "".join("%g 0 %g\n0 %g %g\n0 0 1\n" % (0.8 * hw[1], hw[1] / 2.0, 0.8 * hw[1], hw[0] / 2.0) for _ in cams))
    with open(scene / "scene.obj", "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(v) for v in g["verts"]) + "".join("f %d %d %d\n" % tuple(f + 1) for f in faces))
    for i, m in enumerate(seg_maps):
        m = np.asarray(m, np.float32)
        write_exr(scene / "segmentation" / ("%03d.exr" % i), np.repeat(m.reshape(*m.shape[:2], 1), 3, 2))
    return scene


def random_maps(n=N_CAPTURES, hw=(H, W), top=5):
    g = np.random.default_rng(11)
    return [g.integers(0, top + 1, hw).astype(np.float32) for _ in range(n)]


# ---- the restatement
def hand_case():
    """(tri, valid, ids, F, seg_num): triangle 0 a tie between ids 1 and 2 plus three votes for id 4; triangle 1 no vote; triangle 2 votes for id 0 only;
    triangle 3 -- the last -- id 3 twice and id 1 once; and a miss carrying id 2"""
    votes = [(0, 1), (0, 2), (0, 2), (0, 1), (0, 4), (0, 4), (0, 4), (2, 0), (2, 0), (3, 3), (3, 1), (3, 3)]
    tri = np.array([t for t, _ in votes] + [1], np.int64)
    ids = np.array([i for _, i in votes] + [2], np.float32)
    valid = np.array([True] * len(votes) + [False])
    return tri, valid, ids, 4, 4


def test_the_restatement_on_a_hand_written_case():
    tri, valid, ids, F, seg_num = hand_case()
    # rows as wide as the reference's (n_labels = seg_num): id 3 = n_labels - 1 is counted, id 4 = n_labels is dropped
    hist = ref.vote(tri, valid, ids, F, seg_num)
    assert hist.tolist() == [[0, 2, 2, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 2]]
    labels = ref.triangle_labels(hist)
    assert labels.tolist() == [1, 0, 0, 3]              # the tie goes to the lower id; no vote -> 0; only id 0 -> 0; the last column wins
    # ... and that is the reference's own arithmetic wherever it stays in range (its votes for id 4 land in triangle 1's unread column 0)
    assert ref.reference_flat(tri, valid, ids, F, seg_num).tolist() == labels.tolist()
    # rows one wider (the default): the largest id can win
    wide = ref.vote(tri, valid, ids, F, seg_num + 1)
    assert wide[:, 0].tolist() == [0] * F and wide[0].tolist() == [0, 2, 2, 0, 3]
    assert ref.triangle_labels(wide).tolist() == [4, 0, 0, 3]
    # the reference's failure: the largest id on the last triangle is out of range there, dropped here
    tri2, valid2, ids2 = np.append(tri, 3), np.append(valid, True), np.append(ids, np.float32(4))
    with pytest.raises(IndexError):
        ref.reference_flat(tri2, valid2, ids2, F, seg_num)
    assert ref.triangle_labels(ref.vote(tri2, valid2, ids2, F, seg_num)).tolist() == labels.tolist()
    # the painted view
    assert ref.label_view(tri, valid, labels, miss=0).tolist() == [1] * 7 + [0, 0, 3, 3, 3, 0]
    assert ref.label_view(tri, valid, labels, miss=-1)[-1] == -1


def test_the_restatement_drops_what_is_no_id():
    ids = np.array([0, -3, np.nan, 5, 12, 2.9, 3.0, 1.0, -0.5, np.inf], np.float32)
    tri = np.zeros(len(ids), np.int64)
    hist = ref.vote(tri, np.ones(len(ids), bool), ids, 2, 5)
    assert hist.tolist() == [[0, 1, 1, 1, 0], [0, 0, 0, 0, 0]]                   # 2.9 -> 2, 3.0 -> 3, 1.0 -> 1; the rest votes for nothing
    assert ref.vote(tri, np.ones(len(ids), bool), np.array([0, 253, 255, 5, 12, 2, 3, 1, 0, 0], np.uint8), 2, 5).tolist() == hist.tolist()
    assert ref.vote(np.array([2, -1, 0]), np.ones(3, bool), np.array([1, 1, 1]), 2, 5).sum() == 1   # a triangle outside [0, F) votes for nothing
    assert ref.triangle_labels(np.zeros((3, 1), np.int64)).tolist() == [0, 0, 0]
    big = np.array([[0, 2 ** 31 - 1, 2 ** 31 + 5]], np.uint32)
    assert ref.triangle_labels(big).tolist() == [2]


# ---- the ray arguments of pool_view, vote_view and label_view
class _SceneStandIn:
    device = "the scene's device"


def _views():
    c2w = np.array([[1, 0, 0, 2.0], [0, 0, 1, 1.5], [0, -1, 0, 1.2]], np.float32)
    K = np.array([[0.8 * W, 0, W / 2.0], [0, 0.7 * W, H / 2.0], [0, 0, 1]], np.float32)
    return [{"kind": "real", "K": K, "c2w": c2w}, {"kind": "synthetic", "focal": 41.5, "c2w": c2w}]


@pytest.mark.parametrize("view", _views(), ids=["real", "synthetic"])
def test_the_ray_arguments_of_a_camera(view):
    import ctypes as C
    from iris_amd import _lib as L
    from iris_amd.utils.dataset.pixel_set import camera_table
    from iris_amd.utils.gbuffer import view_rays_args
    synthetic = view["kind"] == "synthetic"
    a, keep, scene = L.PoolViewArgs(), [], _SceneStandIn()
    assert view_rays_args("pool_view", a.rays, keep, scene, view, (H, W), None) == (H * W, scene.device)
    assert (a.rays.H, a.rays.W, a.rays.synthetic) == (H, W, int(synthetic))
    assert not a.rays.rays_o and not a.rays.rays_d and a.rays.ray_stride == 0 and not a.rgb          # (the rest of the structure is left alone)
    row = camera_table([view], synthetic)[0]
    assert row.shape == (24,) and row.dtype == np.float32 and row.any()
    assert np.array_equal(np.ctypeslib.as_array(C.cast(a.rays.camera, C.POINTER(C.c_float)), (24,)), row)
    assert any(isinstance(k, np.ndarray) and k.ctypes.data == a.rays.camera for k in keep)


def test_the_ray_arguments_that_are_refused():
    import torch
    from iris_amd import _lib as L
    from iris_amd.utils.gbuffer import view_rays_args
    view = _views()[0]
    for camera, img_hw, rays in ((view, (H, W), torch.zeros(4, 6)), (None, (H, W), None), (view, None, None), (None, None, torch.zeros(4, 6))):
        keep = []
        with pytest.raises(L.IrisError):
            view_rays_args("label_view", L.LabelViewArgs().rays, keep, _SceneStandIn(), camera, img_hw, rays)
        assert not keep


# ---- the stage's host half
def test_split_all_of_a_real_layout_is_every_capture_in_order(tmp_path):
    from iris_amd import fuse_segmentation as fs
    from iris_amd.utils import cameras
    scene = write_real_scene(tmp_path, random_maps())
    ids, views = fs.load_split("real", str(scene), "all", (H, W))
    assert ids == list(range(N_CAPTURES)) and len(views) == N_CAPTURES
    halves = {}
    for split in ("train", "val"):
        _, vs = cameras.load_real(str(scene), img_hw=(H, W), split=split)
        halves.update(zip(cameras.real_split_ids(N_CAPTURES, split), vs))
    assert sorted(halves) == ids and cameras.real_split_ids(N_CAPTURES, "val") == [0, 10]
    for i, view in zip(ids, views):
        assert view["kind"] == "real"
        assert np.array_equal(view["K"], halves[i]["K"]) and np.array_equal(view["c2w"], halves[i]["c2w"])
    assert len({view["c2w"].tobytes() for view in views}) == N_CAPTURES            # (distinct cameras: the order is checked, not only the count)
    ids, views = fs.load_split("real", str(scene), "train", (H, W))
    assert ids == [1, 2, 3, 4, 5, 6, 7, 8, 9, 11]
    assert all(np.array_equal(v["c2w"], halves[i]["c2w"]) for i, v in zip(ids, views))


def test_the_host_half_reads_the_ids_and_sizes_the_rows(tmp_path):
    from iris_amd import fuse_segmentation as fs
    from iris_amd.utils.exr import write_exr
    maps = random_maps(top=5)
    scene = write_real_scene(tmp_path, maps)
    # a file whose channels differ: the ids are its B channel (cv2's channel 0)
    rgb = np.stack([np.full((H, W), 9, np.float32), np.full((H, W), 8, np.float32), maps[3]], -1)
    write_exr(scene / "segmentation" / "003.exr", rgb)
    common = ["--scene", str(scene), "--dataset", "real"]
    (_, faces), img_hw, ids, views, host_maps, n_labels, seg_num, seg_dir, out_dir, swap = fs.open_fusion(fs.parser().parse_args(common))
    assert img_hw == (H, W) and ids == list(range(N_CAPTURES)) and len(faces) == 14
    assert all(np.array_equal(a, b) for a, b in zip(host_maps, maps)) and host_maps[0].dtype == np.float32
    assert (seg_num, n_labels, swap) == (5, 6, True) and out_dir == str(scene / "segmentation-new") and seg_dir == str(scene / "segmentation")
    out = fs.open_fusion(fs.parser().parse_args(common + ["--compat", "reference", "--output", str(tmp_path / "o"), "--split", "train"]))
    assert out[5] == 5 and out[2] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 11] and out[8] == str(tmp_path / "o") and out[9] is False


def test_refusals_come_before_the_device_is_opened(tmp_path, capsys, monkeypatch):
    from iris_amd import fuse_segmentation as fs
    from iris_amd.utils import stage
    from iris_amd.utils.exr import write_exr

    def opened(*a, **k):
        pytest.fail("a refused command opened the device")
    monkeypatch.setattr(stage, "open_device", opened)

    def refused(scene, *extra, dataset="real"):
        capsys.readouterr()
        assert fs.cli(["--scene", str(scene), "--dataset", dataset] + list(extra)) == 2
        err = capsys.readouterr().err
        assert err.startswith("fuse_segmentation: ") and err.endswith("\n") and err.count("\n") == 1, err
        return err

    os.makedirs(tmp_path / "a")
    scene = write_real_scene(tmp_path / "a", random_maps())
    os.remove(scene / "segmentation" / "007.exr")                                # a missing segmentation file
    assert "007.exr" in refused(scene)
    write_exr(scene / "segmentation" / "007.exr", np.zeros((H, W + 1, 3), np.float32))          # a file of another size
    err = refused(scene)
    assert "007.exr" in err and "%d x %d" % (H, W + 1) in err
    write_exr(scene / "segmentation" / "007.exr", np.ones((H, W, 3), np.float32))
    os.makedirs(scene / "segmentation-old")                                      # an existing segmentation-old
    assert "segmentation-old" in refused(scene)
    os.rmdir(scene / "segmentation-old")
    os.makedirs(scene / "segmentation-new")
    assert "segmentation-new" in refused(scene)
    os.rmdir(scene / "segmentation-new")
    err = refused(scene, "--max_hist_gb", "1e-7")                               # 14 triangles x 6 ids x 4 bytes = 336 bytes > 107 bytes
    assert "max_hist_gb" in err and "14 triangles x 6 ids" in err
    assert "scannetpp" in refused(scene, dataset="scannetpp")                    # the scannetpp layout is not built for this stage
    assert sorted(os.listdir(scene)) == ["K_list.txt", "cam.txt", "scene.obj", "segmentation"]       # nothing was written or renamed
