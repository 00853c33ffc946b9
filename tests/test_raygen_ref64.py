"""The HIP ray generator against the float64 restatement of tests/raygen_ref64.py, through the public calls iris_amd.utils.dataset.real_ldr
(get_direction / to_world) and synthetic_ldr (get_ray_directions / get_rays), with and without ray differentials: every pixel of every case inside the
derived bound (K_D = 6, K_N = 3.5; raygen_ref64's docstring), rays_o and the differentials bit for bit.  The cases, the bound and the float64 run are those
of tests/test_raygen_ref64_cpu.py, which holds the oracle and the float32 restatement to them.  The 1025 x 1031 view is 8 199 pixels past one pass of the
kernel's grid-stride loop; a few hundred of its pixels, on both sides of the pass boundary, are also asked of the pixel-batch kernel, whose rows are the
whole-view rows bit for bit.  Ids outside the table -- the documented zero-row branch of pixel_batch_kernel -- go through the C ABI with all six outputs.

Worst |err| / tol on an MI355X over all cases: 0.36 un-normalised, 0.25 normalised (the oracle's figures on the CPU: the kernel's bits).
"""
import numpy as np
import pytest
import torch

import raygen_ref64 as R

pytestmark = pytest.mark.gpu

OUTPUTS = ("rays", "rgbs", "int_albedo", "segmentation", "exposure", "positions")


class Hip:
    name = "hip"

    def rays(self, cam, H, W, ray_diff):
        from iris_amd.utils.dataset import real_ldr, synthetic_ldr
        if cam["kind"] == "real":
            out = real_ldr.to_world(real_ldr.get_direction(cam["K"], (H, W)), cam["c2w"], ray_diff, device="cuda:0")
        else:
            out = synthetic_ldr.get_rays(synthetic_ldr.get_ray_directions(H, W, cam["focal"]), cam["c2w"], focal=cam["focal"] if ray_diff else None,
                                         device="cuda:0")
        return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("case", R.cases(), ids=R.case_id)
def test_rays(case):
    R.check_view(Hip(), case)


def pixel_batch(ids, cams, H, W, ray_diff, stores=None, want=("rays",)):
    """iris_pixel_batch called directly -> {name: tensor} of the outputs in `want` (prefilled with -7: a row the kernel skipped would show)"""
    from iris_amd import _lib as L
    from iris_amd.utils.dataset.pixel_set import camera_table
    dev = ids.device
    synthetic = cams[0]["kind"] == "synthetic"
    table = torch.from_numpy(camera_table(cams, synthetic)).to(dev)
    d = {k: torch.from_numpy(v).to(dev) for k, v in (stores or {}).items()}
    B = ids.shape[0]
    shapes = dict(rays=((B, 12), torch.float32), rgbs=((B, 3), torch.float32), int_albedo=((B, 3), torch.float32), segmentation=((B,), torch.int64),
                  exposure=((B, 1), torch.float32), positions=((B, 3), torch.float32))
    out = {k: torch.full(shapes[k][0], -7, device=dev, dtype=shapes[k][1]) for k in want}
    p = lambda k: L.ptr(out[k]) if k in out else None
    s = lambda k: L.ptr(d[k]) if k in d else None
    L.check(L.lib().iris_pixel_batch(L.ptr(ids), B, L.ptr(table), len(cams), H, W, int(ray_diff), int(synthetic), s("rgb"), 1, s("int_albedo"), 1,
                                     s("segmentation"), s("positions"), s("exposure"), p("rays"), p("rgbs"), p("int_albedo"), p("segmentation"),
                                     p("exposure"), p("positions"), L.stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("ray_diff", [False, True], ids=["unit", "diff"])
def test_pixel_batch_rows_are_the_whole_view_rows_past_one_pass(ray_diff):
    H, W = R.LARGE
    cam = R.cameras()["real-zero-entries-far"]
    whole = Hip().rays(cam, H, W, ray_diff)
    whole = np.concatenate(list(whole) + [np.zeros((H * W, 3), np.float32)] * (4 - len(whole)), 1)
    ids = R.spread_ids(H * W)
    assert (ids >= R.ONE_PASS).sum() >= 100 and (ids < R.ONE_PASS).sum() >= 100
    rows = pixel_batch(torch.from_numpy(ids).cuda(), [cam], H, W, ray_diff)["rays"].cpu().numpy()
    assert np.array_equal(rows.view(np.int32), whole[ids].view(np.int32))


@pytest.mark.parametrize("kind", ["real", "synthetic"])
def test_ids_outside_the_table_give_zero_rows(kind):
    """ids -1, V H W, 2^40 and INT64_MIN among valid ones, all six outputs: zero rows, segment -1, exposure 0 -- and every valid row as without them.
    (The kernel tests the id before it reads anything: iris_batch.h, `ok`.)"""
    H, W = 5, 7
    names = [n for n, c in R.cameras().items() if c["kind"] == kind]
    cams = [R.cameras()[n] for n in (names + names)[:3]]
    V = len(cams)
    N = V * H * W
    g = np.random.default_rng(9)
    stores = dict(rgb=g.integers(1, 256, (N, 3)).astype(np.uint8), int_albedo=g.integers(1, 256, (N, 3)).astype(np.uint8),
                  segmentation=g.integers(1, 1000, N).astype(np.int32), exposure=(0.5 + g.random(V)).astype(np.float32),
                  positions=(1 + g.random((N, 3))).astype(np.float32))
    valid = g.permutation(N)[:70].astype(np.int64)
    outside = np.array([-1, N, 2 ** 40, np.iinfo(np.int64).min, N + 1, -N], np.int64)
    ids = np.concatenate([valid, np.repeat(outside, 3)])
    ids = ids[g.permutation(len(ids))]
    bad = (ids < 0) | (ids >= N)
    assert bad.sum() == 18 and set(outside.tolist()) <= set(ids[bad].tolist())
    for ray_diff in (1, 0):
        got = pixel_batch(torch.from_numpy(ids).cuda(), cams, H, W, ray_diff, stores, OUTPUTS)
        ref = pixel_batch(torch.from_numpy(ids[~bad]).cuda(), cams, H, W, ray_diff, stores, OUTPUTS)
        for k in OUTPUTS:
            a, r = got[k].cpu().numpy(), ref[k].cpu().numpy()
            assert np.array_equal(a[~bad], r), k                                                  # every valid row unchanged
            want = -1 if k == "segmentation" else 0
            assert (a[bad] == want).all(), k
        r = ref["rays"].cpu().numpy()                                                             # (and the valid rows are rays: no zero row among them)
        assert (np.abs(r[:, 3:6]).sum(-1) > 0).all() and (ref["segmentation"] > 0).all() and (ref["exposure"] > 0).all()
