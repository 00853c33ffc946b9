"""The step losses without a GPU (iris_amd/utils/losses.py): validation happens before any device work, the float64 restatement (tests/losses_ref64.py)
agrees with the reference's scale_invariant_mse, and detaching the scale -- what the reference's .item() does and the kernels copy -- changes nothing."""
import pytest
import torch

from losses_ref64 import LA, albedo_restatement, case, scale_invariant_mse, segment_mean


def _batch(n=5):
    g = torch.Generator().manual_seed(0)
    mat = dict(albedo=torch.rand(n, 3, generator=g), metallic=torch.rand(n, 1, generator=g), roughness=torch.rand(n, 1, generator=g))
    kw = dict(cache=None, idx=torch.arange(n), crf=None, exposure=1.0, rgbs_gt=torch.rand(n, 3, generator=g), segmentation=torch.arange(n) // 2,
              positions=torch.rand(n, 3, generator=g), albedo_prior=torch.rand(n, 3, generator=g), la=LA)
    return mat, kw


def test_wrong_entry_counts_name_the_argument():
    from iris_amd.utils.losses import brdf_crf_loss, initialize_loss, segment_albedo_loss
    a, t, seg = torch.rand(5, 3), torch.rand(5, 3), torch.arange(5)
    with pytest.raises(ValueError, match="albedo_prior"):
        segment_albedo_loss(a, t[:4], seg)
    with pytest.raises(ValueError, match="albedo has"):
        segment_albedo_loss(a[:, :2], t, seg)
    for name in ("rgbs_gt", "positions", "albedo_prior", "idx"):
        mat, kw = _batch()
        kw[name] = kw[name][:4]
        with pytest.raises(ValueError, match=name + " has"):
            brdf_crf_loss(mat, **kw)
    for name in ("albedo", "metallic", "roughness"):
        mat, kw = _batch()
        mat[name] = mat[name][:4]
        with pytest.raises(ValueError, match=name + " has"):
            brdf_crf_loss(mat, **kw)
    mat, kw = _batch()
    for name in ("L", "rgbs_gt", "albedo_prior"):
        args = dict(L=torch.rand(5, 3), rgbs_gt=kw["rgbs_gt"], albedo_prior=kw["albedo_prior"])
        args[name] = args[name][:4]
        with pytest.raises(ValueError, match=name + " has"):
            initialize_loss(mat["albedo"], args.pop("L"), crf=None, exposure=1.0, segmentation=kw["segmentation"], **args)


def test_cpu_tensors_raise():
    """no CPU fallback: the shapes are right, the tensors are on the host; cache and crf are never reached"""
    from iris_amd._lib import IrisError
    from iris_amd.utils.losses import brdf_crf_loss, initialize_loss, segment_albedo_loss
    mat, kw = _batch()
    with pytest.raises(IrisError):
        segment_albedo_loss(mat["albedo"], kw["albedo_prior"], kw["segmentation"])
    with pytest.raises(IrisError):
        brdf_crf_loss(mat, **kw)
    with pytest.raises(IrisError):
        initialize_loss(mat["albedo"], torch.rand(5, 3), crf=None, exposure=1.0, rgbs_gt=kw["rgbs_gt"], albedo_prior=kw["albedo_prior"],
                        segmentation=kw["segmentation"])


def test_albedo_term_needs_its_prior():
    from iris_amd.utils.losses import brdf_crf_loss
    mat, kw = _batch()
    kw["albedo_prior"] = None
    with pytest.raises(ValueError, match="albedo_prior"):
        brdf_crf_loss(mat, **kw)


def test_restatement_against_the_reference_function():
    """the restatement's scale-invariant mode = la * scale_invariant_mse(mean_albedo_tgt, albedo) (train_brdf_crf.py:305-306) in float64, to 1e-15 relative"""
    g = torch.Generator().manual_seed(4)
    for n, nseg in ((1, 1), (7, 3), (500, 11)):
        seg = torch.randint(0, nseg, (n,), generator=g) * 13 + 2
        a = torch.rand(n, 3, generator=g, dtype=torch.float64)
        t = torch.randint(0, 256, (n, 3), generator=g).double() / 255.0 + 1.0 / 510.0
        loss, _, k = albedo_restatement(a, t, seg, torch.float64, True, LA)
        tbar = segment_mean(t, seg)
        want = LA * scale_invariant_mse(tbar, a)
        assert abs(float(loss) - float(want)) <= 1e-15 * abs(float(want))
        assert abs(k - float(torch.dot(tbar.reshape(-1), a.reshape(-1)) / torch.dot(tbar.reshape(-1), tbar.reshape(-1)))) <= 1e-15 * abs(k)
        mse, _, one = albedo_restatement(a, t, seg, torch.float64, False)
        assert one == 1.0 and abs(float(mse) - float(((a - tbar) ** 2).mean())) <= 1e-15 * float(mse)


def test_detaching_the_scale_is_harmless():
    """k is the least-squares scale: d loss / d k = 2 mean(tbar (k tbar - a)) = 0 at that k, so the term the reference drops with .item() vanishes.
    The gradients with the scale detached and attached differ by less than 1e-12 of max |g| in float64."""
    for name in ("small", "multi"):
        d, _ = case(name)
        _, g_det, k0 = albedo_restatement(d["albedo"], d["prior"], d["seg"], torch.float64, True, LA, detach_scale=True)
        _, g_att, k1 = albedo_restatement(d["albedo"], d["prior"], d["seg"], torch.float64, True, LA, detach_scale=False)
        dev, top = float((g_det - g_att).abs().max()), float(g_det.abs().max())
        print(f"{name}: max |g_detached - g_attached| {dev:.3g}, max |g| {top:.3g}, k {k0:.6f}")
        assert k0 == k1 and top > 0 and dev < 1e-12 * top
