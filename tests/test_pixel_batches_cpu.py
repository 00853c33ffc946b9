"""PixelSet's argument validation (iris_amd/utils/dataset/pixel_set.py): everything here is decided on the host, before a device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

H, W = 5, 7


def views(n=3, kind="real"):
    c2w = np.hstack([np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32)])
    if kind == "synthetic":
        return [dict(kind="synthetic", focal=3.0 + v, c2w=c2w) for v in range(n)]
    return [dict(kind="real", K=np.array([[3.0 + v, 0, 3.5], [0, 3.0, 2.5], [0, 0, 1]], np.float32), c2w=c2w) for v in range(n)]


def test_prototype_is_bound():
    from iris_amd import _lib as L
    p = L.PROTOTYPES["iris_pixel_batch"]
    assert len(p) == 22 and p[0] is C.c_void_p and p[1] is C.c_int64 and p[3] is C.c_int64 and p[-1] is C.c_void_p
    assert [t for t in p if t is C.c_int] == [C.c_int] * 6          # H, W, ray_diff, synthetic and the two 8-bit flags


def test_cpu_device_and_cpu_tensors_are_rejected():
    from iris_amd import _lib as L
    from iris_amd.utils.dataset import PixelSet
    n = 3 * H * W
    rgb = np.zeros((n, 3), np.uint8)
    with pytest.raises(L.IrisError):
        PixelSet(views(), (H, W), rgb, batch_size=8, device="cpu")
    with pytest.raises(L.IrisError):
        PixelSet(views(), (H, W), torch.zeros(n, 3, dtype=torch.uint8), batch_size=8, device="cuda")
    with pytest.raises(L.IrisError):
        PixelSet(views(), (H, W), rgb, segmentation=torch.zeros(n, dtype=torch.int32), batch_size=8, device="cuda")


def test_mismatched_shapes_and_types_are_rejected():
    from iris_amd.utils.dataset import PixelSet
    n = 3 * H * W
    rgb = np.zeros((n, 3), np.uint8)
    bad = [dict(rgb=rgb[:-1]), dict(rgb=rgb.astype(np.float64)), dict(rgb=[rgb[:H * W], rgb[:H * W]]), dict(rgb=rgb, int_albedo=np.zeros((n, 4), np.uint8)),
           dict(rgb=rgb, segmentation=np.zeros(n + 1, np.int32)), dict(rgb=rgb, exposure=np.ones(2, np.float32)), dict(rgb=rgb, batch_size=0),
           dict(rgb=rgb, synthetic=True), dict(rgb=rgb, cameras=views(kind="synthetic")), dict(rgb=rgb, cameras=[])]
    for kw in bad:
        kw = dict(dict(cameras=views(), img_hw=(H, W), batch_size=8, device="cuda"), **kw)
        with pytest.raises(ValueError):
            PixelSet(**kw)


def test_ids_are_bounded_on_the_host():
    from iris_amd.utils.dataset.pixel_set import check_ids
    n = 3 * H * W
    ok = check_ids(np.array([0, n - 1, 5, 5]), n)
    assert ok.dtype == torch.int64 and ok.tolist() == [0, n - 1, 5, 5]
    assert check_ids(torch.zeros(0, dtype=torch.int64), n).shape == (0,)
    for bad in ([0, n], [-1, 3], [2 ** 40]):
        with pytest.raises(ValueError):
            check_ids(torch.tensor(bad), n)
    with pytest.raises(ValueError):
        check_ids(torch.tensor([0.0, 1.0]), n)
    with pytest.raises(ValueError):
        check_ids(torch.zeros(2, 2, dtype=torch.int64), n)


def test_cache_length_and_batch_count():
    from iris_amd.utils.dataset.pixel_set import batch_count, check_cache_length

    class Rows:
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n
    check_cache_length(Rows(105), 105)
    with pytest.raises(ValueError):
        check_cache_length(Rows(104), 105)
    assert [batch_count(n, 16) for n in (0, 1, 16, 17, 105)] == [0, 1, 1, 2, 7]
    assert batch_count(2 ** 33 + 1, 8192) == 2 ** 20 + 1
    with pytest.raises(ValueError):
        batch_count(10, 0)


def test_camera_table_layout():
    from iris_amd.utils.dataset.pixel_set import CAM_FLOATS, camera_table
    t = camera_table(views(), False)
    assert t.shape == (3, CAM_FLOATS) and t.dtype == np.float32
    assert t[1, 0] == 4.0 and t[1, 2] == 3.5 and t[1, 5] == 2.5 and list(t[1, 9:21]) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] and t[1, 21] == 1.0
    s = camera_table(views(kind="synthetic"), True)
    assert s[2, 21] == 5.0 and not s[:, :9].any() and not s[:, 22:].any()
