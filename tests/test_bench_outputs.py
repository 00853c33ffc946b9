"""bench.py --dump-outputs on the CPU: what dump_outputs writes for a view of the benchmark's size (no GPU call)."""
import os
import sys

import numpy as np
import torch

from conftest import REPO


def test_dump_outputs_is_a_fixed_sample_within_the_budget(tmp_path):
    """13 maps of a 1920x1080 view: one float32 file per map plus the pixel ids, at most 64 MB together, the same rows in every run, each row the
    map's value at the pixel pixel_index names."""
    sys.path.insert(0, REPO)
    import bench
    n = 1920 * 1080
    pix = torch.arange(n) * 2 + 1                                                  # image pixel ids of the rows (a rank's stripes need not be 0..n-1)
    maps = (pix.float()[None, :, None] + torch.arange(13).float()[:, None, None] * 1e6).expand(13, n, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), maps, pix, [0, 1, 2, 3, 4, 5, 6])
    names = ["lobe0_Ld"] + [f"lobe{l}_Ls{k}" for l in range(1, 7) for k in (0, 1)]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(x + ".npy" for x in names + ["pixel_index"])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    ids = np.load(tmp_path / "a" / "pixel_index.npy")
    assert ids.dtype == np.float64 and 0.1 * n < len(ids) < n and np.all(np.diff(ids) > 0)
    assert np.array_equal(ids, np.load(tmp_path / "b" / "pixel_index.npy"))
    for m, name in enumerate(names):
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == (len(ids), 3)
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy")))
        assert np.array_equal(a[:, 0].astype(np.float64), ids + m * 1e6)
