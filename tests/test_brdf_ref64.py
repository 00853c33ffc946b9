"""The HIP BRDF samplers and GGX evaluation against the float64 reference of tests/brdf_ref64.py, through the public surface: BaseBRDF.sample_diffuse /
sample_specular (one roughness, and one per row) / eval_brdf / sample_brdf, SLFEmitterLearn.sample_emitter, ops.angle2xyz, ops.get_normal_space and
ops.lerp_specular.  The case tables and the checks are those of tests/test_brdf_ref64_cpu.py, which holds the same tables against the oracle in both modes
and against the float32 run of the restatement: that file vouches for the inputs, the caps and the direction bound 2 E (E: the larger direction error of
the libm oracle and of the float32 restatement on the same table, measured when the test runs; its values are in that file's docstring).

Every table has 2^15 rows (128 blocks of 256 threads), odd edge rows at shuffled positions; a call takes well under a millisecond of GPU time.
"""
import functools

import numpy as np
import pytest
import torch

import brdf_ref64 as R

pytestmark = pytest.mark.gpu


class Hip:
    """the package's public calls, numpy in / numpy out"""
    name = "hip"

    def __init__(self, tmp):
        from iris_amd.model.brdf import BaseBRDF
        from iris_amd.utils import ops
        self.dev = torch.device("cuda:0")
        self.brdf, self.ops, self.tmp, self._em = BaseBRDF(), ops, tmp, {}

    def T(self, a):
        return torch.from_numpy(np.array(a)).to(self.dev)                    # (a copy: the shared tables are read-only)

    @staticmethod
    def N(*ts):
        return tuple(t.detach().cpu().numpy() for t in ts)

    def _mat(self, albedo, rough, metal):
        return {"albedo": self.T(albedo), "roughness": self.T(rough).reshape(-1, 1), "metallic": self.T(metal).reshape(-1, 1)}

    def sample_diffuse(self, u2, n):
        return self.N(*self.brdf.sample_diffuse(self.T(u2), self.T(n)))

    def sample_specular(self, u2, wo, n, rough):
        return self.N(*self.brdf.sample_specular(self.T(u2), self.T(wo), self.T(n), float(rough)))

    def sample_specular_v(self, u2, wo, n, rough):
        return self.N(*self.brdf.sample_specular(self.T(u2), self.T(wo), self.T(n), self.T(rough).reshape(-1, 1)))

    def eval_brdf(self, wi, wo, n, albedo, rough, metal):
        return self.N(*self.brdf.eval_brdf(self.T(wi), self.T(wo), self.T(n), self._mat(albedo, rough, metal)))

    def sample_brdf(self, s1, u2, wo, n, albedo, rough, metal):
        return self.N(*self.brdf.sample_brdf(self.T(s1), self.T(u2), self.T(wo), self.T(n), self._mat(albedo, rough, metal)))

    def _emitter(self, em):
        from iris_amd.model.emitter import SLFEmitterLearn
        from iris_amd.model.slf import VoxelSLF
        key = em["key"]
        if key not in self._em:
            K = em["K"]
            mask = torch.ones(2, 2, 2, dtype=torch.bool)
            slf = VoxelSLF(mask, -1.0, 1.0)
            ep, sp = str(self.tmp / f"emitter{len(self._em)}.pth"), str(self.tmp / f"vslf{len(self._em)}.npz")
            torch.save({"is_emitter": torch.from_numpy(em["is_emitter"]), "emitter_vertices": torch.from_numpy(em["verts"]),
                        "emitter_area": torch.from_numpy(em["area"]), "emitter_normal": torch.zeros(K, 3), "emitter_radiance": torch.ones(K, 3)}, ep)
            torch.save({"mask": mask, "voxel_min": -1.0, "voxel_max": 1.0, "weight": slf.state_dict()}, sp)
            m = SLFEmitterLearn(ep, sp).to(self.dev)
            np.testing.assert_array_equal(m.emitter_cdf.cpu().numpy(), em["cdf"])             # the table's cdf is the model's
            assert float(m.emitter_pdf[0]) == float(em["emitter_pdf"])
            self._em[key] = m
        return self._em[key]

    def sample_emitter(self, em, s1, s2, pos):
        return self.N(*self._emitter(em).sample_emitter(self.T(s1), self.T(s2), self.T(pos)))

    def angle2xyz(self, theta, phi):
        return self.N(self.ops.angle2xyz(self.T(theta), self.T(phi)))[0]

    def get_normal_space(self, n):
        return self.N(self.ops.get_normal_space(self.T(n)))[0]

    def lerp_specular(self, spec, rough):
        return self.N(self.ops.lerp_specular(self.T(spec), self.T(rough).reshape(-1, 1)))[0]


@functools.lru_cache(maxsize=None)
def emitter(K, zero):
    """the emitter tables with the cdf built as the model builds it (model/emitter.py:168-170)"""
    em = R.emitter_tables(K, zero)
    em["cdf"] = torch.nn.functional.normalize(torch.ones(K), dim=-1, p=1).cumsum(-1).numpy().copy()
    return em


@pytest.fixture(scope="module")
def bounds(oracle_mod):
    return R.Bounds(oracle_mod)


@pytest.fixture(scope="module")
def back(tmp_path_factory):
    return Hip(tmp_path_factory.mktemp("brdf_ref64"))


def test_sample_diffuse(back, bounds):
    R.check_sample_diffuse(back, bounds)


@pytest.mark.parametrize("rough", R.ROUGH_LEVELS, ids=[f"r{float(r):.3g}" for r in R.ROUGH_LEVELS])
def test_sample_specular(back, bounds, rough):
    R.check_sample_specular(back, bounds, rough)


def test_sample_specular_per_row_roughness(back, bounds):
    R.check_sample_specular_rows(back, bounds)


def test_eval_brdf(back):
    R.check_eval_brdf(back)


def test_sample_brdf(back, bounds):
    R.check_sample_brdf(back, bounds)


@pytest.mark.parametrize("K,zero", R.EMITTER_CONFIGS, ids=[f"K{k}" + ("" if z is None else "-area0") for k, z in R.EMITTER_CONFIGS])
def test_sample_emitter(back, bounds, K, zero):
    R.check_sample_emitter(back, bounds, emitter(K, zero))


def test_get_normal_space(back):
    R.check_get_normal_space(back)


@pytest.mark.parametrize("levels", [1, 2, 6])
def test_lerp_specular(back, levels):
    R.check_lerp_specular(back, levels)


def test_angle2xyz(back, bounds):
    R.check_angle2xyz(back, bounds)
