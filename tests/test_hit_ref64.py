"""The HIP closest hit (iris_amd.utils.path_tracing.Scene / ray_intersect, both node layouts) against exact float64 geometry and against its exact
symmetries: the inputs, the checks and the constants of tests/hit_ref64.py, which tests/test_hit_ref64_cpu.py holds the oracle and the float32
restatement to.  That file vouches for the inputs and the caps; the constants C = 4 E are measured here again from the restatement alone.

ray_intersect returns no t.  Soundness of t is carried by p and uv (p = o + t d lies in the plane and at the barycentrics of the reported
triangle); in the completeness bound the t of the reported triangle's plane stands in for it (hit_ref64.check_hits).  The symmetry tests compare
idx, valid, uv, p and n.  Every result is also held to the oracle's bits, as test_hip_parity.py does on its inputs: here at offsets of 64 and 1024.

One Scene per (input, layout), the transformed problems of the symmetry tests as Scenes of their own; the largest launch is 20 000 rays against
1 280 triangles.
"""
import numpy as np
import pytest
import torch

import hit_ref64 as R

pytestmark = pytest.mark.gpu

LAYOUTS = ("BVH4_Q8", "BVH4_F32")


def run(layout, v, f, o, d):
    from iris_amd import _lib as L
    from iris_amd.utils.path_tracing import Scene, ray_intersect
    dev = torch.device("cuda:0")
    sc = Scene(v, f, device=dev, layout=getattr(L, layout))
    assert sc.info()["layout"] == getattr(L, layout)
    p, n, uv, idx, valid = ray_intersect(sc, torch.from_numpy(np.array(o)).to(dev), torch.from_numpy(np.array(d)).to(dev))
    return dict(idx=idx.cpu().numpy(), valid=valid.cpu().numpy(), t=None, uv=uv.cpu().numpy(), p=p.cpu().numpy(), n=n.cpu().numpy())


_cache = {}


def result(layout, name):
    if (layout, name) not in _cache:
        v, f, o, d, _ = R.scene(name)
        _cache[layout, name] = run(layout, v, f, o, d)
    return _cache[layout, name]


def assert_is_oracle(oracle_mod, res, v, f, o, d, name):
    op, on, ouv, oidx, ovalid = oracle_mod.Scene(v, f).ray_intersect(o, d)
    np.testing.assert_array_equal(res["idx"], oidx, err_msg=name)
    np.testing.assert_array_equal(res["valid"], ovalid, err_msg=name)
    np.testing.assert_array_equal(res["uv"], ouv, err_msg=name)
    np.testing.assert_array_equal(res["p"], op, err_msg=name)
    np.testing.assert_array_equal(res["n"], on, err_msg=name)


@pytest.mark.parametrize("name", list(R.INPUTS))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_closest_hit_is_exact(oracle_mod, layout, name):
    res = result(layout, name)
    out = R.check_input(name, res)
    print(name, layout, out)
    v, f, o, d, _ = R.scene(name)
    assert_is_oracle(oracle_mod, res, v, f, o, d, name)


@pytest.mark.parametrize("kz", (0, 1, 2))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_edge_function_zero_takes_the_exact_sign(layout, kz):
    v, f, o, d, want = R.exact_sign_cases(kz)
    R.check_exact_signs(run(layout, v, f, o, d), want, f"kz = {kz}")


@pytest.mark.parametrize("kz", (0, 1, 2))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_vertices_and_edges_of_the_scene_box_are_hit(layout, kz):
    v, f, o, d, idx, uv, p = R.boundary_cases(kz)
    R.check_boundary(run(layout, v, f, o, d), idx, uv, p, f"kz = {kz}")


@pytest.mark.parametrize("name", R.SYMMETRY_INPUTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_scaling_by_a_power_of_two_is_exact(layout, name):
    v, f, o, d, _ = R.scene(name)
    res = result(layout, name)
    for k in R.SCALES:
        vk, ok = R.scaled(v, o, k)
        R.assert_scaled(res, run(layout, vk, f, ok, d), k, f"{name} 2^{k}")


@pytest.mark.parametrize("name", R.SYMMETRY_INPUTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_axis_permutation_and_mirror_image(layout, name):
    v, f, o, d, _ = R.scene(name)
    res = result(layout, name)
    rows = R.unique_major_axis(d)
    rp = run(layout, R.permuted(v), f, R.permuted(o), R.permuted(d))
    R.assert_isometry(res, rp, rows, lambda a: a[:, [2, 0, 1]], f"{name} permuted")
    rm = run(layout, R.mirrored(v), f, R.mirrored(o), R.mirrored(d))
    R.assert_isometry(res, rm, np.ones(len(o), bool), R.mirrored, f"{name} mirrored")
