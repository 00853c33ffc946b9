"""The HIP voxel radiance cache against the literal float32 index of tests/voxel_ref.py, through the public surface: VoxelSLF.spatial_idx / forward /
scatter_add, gbuffer.voxel_histogram and SLFEmitter.eval_emitter with a roughness array.  Six grids from H = 1 to the H = 256 the reference stages run at
(16.7 M cells: eight passes of the kernel that narrows a device-built grid), each built from a host mask (iris_slf_create) and from a device mask
(iris_slf_create_dev): the two handles give the same answer everywhere.  Tables of 1, 63, 64, 65 and 2 097 155 rows (one pass of the lookup is 8192 x 256
points) with every grid plane and its float neighbours, the box's ends, zeros, a subnormal, 1e30, the infinities, NaN and, on the (2, 0, 1) grid, the
coordinates around 2^31 and 2^63, at shuffled positions.  The index, the radiance rows, the counts, the histogram and eval_emitter's outputs are exact;
scatter_add's sums stay within K u sum |addend| per voxel.  tests/test_voxel_slf_cpu.py holds the oracle and the restatement to the same tables.

Every position is safe to run: voxel_coord clamps whatever integer the conversion yields, so no index leaves the grid.

On an MI355X: everything exact; scatter_add worst |err| / tol 0.61, 0.60, 0.50 and 0.44 for H = 31, 32, 64 and 256, and below 0.001 on the one- and two-cell grids (their bound grows with the count, up to 2^15).
"""
import numpy as np
import pytest
import torch

import voxel_ref as V

pytestmark = pytest.mark.gpu

GRID_IDS = [V.grid_id(g) for g in range(len(V.GRIDS))]


class Hip:
    """the package's public calls, numpy in / numpy out"""
    name = "hip"
    HANDLES = ("host", "device")

    def __init__(self, tmp):
        self.dev, self.tmp, self._slf, self._em = torch.device("cuda:0"), tmp, {}, None

    def T(self, a):
        return torch.from_numpy(np.array(a)).to(self.dev)                  # (a copy: the shared tables are read-only)

    def slf(self, gi, handle):
        """handle 'host': the module stays on the CPU, so its tables go through iris_slf_create; 'device': built from a mask on the GPU, iris_slf_create_dev"""
        from iris_amd.model.slf import VoxelSLF
        if (gi, handle) not in self._slf:
            H, lo, hi = V.GRIDS[gi]
            t = V.grid_tables(gi)
            mask = torch.from_numpy(np.array(t["mask"]))
            s = VoxelSLF(mask if handle == "host" else mask.to(self.dev), lo, hi)
            assert s.inds.device.type == ("cpu" if handle == "host" else "cuda")
            assert np.array_equal(s.inds.cpu().numpy(), t["inds"])
            s.radiance.copy_(torch.from_numpy(np.array(t["radiance"])))
            self._slf[gi, handle] = s
        return self._slf[gi, handle]

    def lookup(self, gi, x, handle):
        s, xt = self.slf(gi, handle), self.T(x)
        return s.spatial_idx(xt).cpu().numpy(), s(xt)["rgb"].cpu().numpy()

    def scatter_add(self, gi, x, rgb):
        from iris_amd.model.slf import VoxelSLF
        H, lo, hi = V.GRIDS[gi]
        s = VoxelSLF(torch.from_numpy(np.array(V.grid_tables(gi)["mask"])).to(self.dev), lo, hi)
        half = len(x) // 2                                                 # two calls: the buffers accumulate
        s.scatter_add(self.T(x[:half]), self.T(rgb[:half]))
        s.scatter_add(self.T(x[half:]), self.T(rgb[half:]))
        return s.radiance.cpu().numpy(), s.count.cpu().numpy()

    def histogram(self, gi, x):
        from iris_amd.utils.gbuffer import voxel_histogram
        H, lo, hi = V.GRIDS[gi]
        return voxel_histogram(self.T(x), lo, hi, H).cpu().numpy()

    def eval_emitter(self, gi, x, tri, rough, trace_roughness):
        from iris_amd.model.emitter import SLFEmitter
        from iris_amd.model.slf import VoxelSLF
        if self._em is None:
            em = V.emitter_tables()
            one = torch.ones(1, 1, 1, dtype=torch.bool)
            ep, sp = str(self.tmp / "emitter.pth"), str(self.tmp / "vslf.npz")
            torch.save({"is_emitter": torch.from_numpy(V.IS_EMITTER.copy()), "emitter_vertices": torch.from_numpy(np.array(em["verts"])),
                        "emitter_area": torch.from_numpy(np.array(em["area"])), "emitter_normal": torch.zeros(len(em["area"]), 3),
                        "emitter_radiance": torch.from_numpy(np.array(em["radiance"]))}, ep)
            torch.save({"mask": one, "voxel_min": 0.0, "voxel_max": 1.0, "weight": VoxelSLF(one, 0.0, 1.0).state_dict()}, sp)
            self._em = SLFEmitter(ep, sp).to(self.dev)
        self._em.slf = self.slf(gi, "device")                              # the emitter over the grid under test
        Le, pdf, vn = self._em.eval_emitter(self.T(x), None, self.T(tri), self.T(rough).reshape(-1, 1), trace_roughness)
        return Le.cpu().numpy(), pdf.cpu().numpy(), vn.cpu().numpy()


@pytest.fixture(scope="module")
def back(tmp_path_factory):
    return Hip(tmp_path_factory.mktemp("voxel_slf"))


@pytest.mark.parametrize("gi", range(len(V.GRIDS)), ids=GRID_IDS)
def test_lookup(back, gi):
    x, rand = V.main_table(gi)
    V.check_float64_agreement(gi, x, rand)
    V.check_lookup(back, gi, x)


@pytest.mark.parametrize("n", V.LENGTHS)
@pytest.mark.parametrize("gi", range(len(V.GRIDS)), ids=GRID_IDS)
def test_lookup_lengths(back, gi, n):
    V.check_lookup(back, gi, V.table(gi, n)[0])


@pytest.mark.parametrize("gi", range(len(V.GRIDS)), ids=GRID_IDS)
def test_scatter_add(back, gi):
    V.check_scatter_add(back, gi)


@pytest.mark.parametrize("gi", range(len(V.GRIDS)), ids=GRID_IDS)
def test_voxel_histogram(back, gi):
    V.check_histogram(back, gi)


@pytest.mark.parametrize("gi", range(len(V.GRIDS)), ids=GRID_IDS)
def test_eval_emitter(back, gi):
    V.check_eval_emitter(back, gi)


@pytest.mark.parametrize("entry", ["kv", "kv+5", "-2", "int64-min"])
@pytest.mark.parametrize("path", ["host", "device"])
def test_creation_refuses_an_index_outside_the_table(path, entry):
    """iris_slf_create and iris_slf_create_dev alike: an `inds` entry >= kv or < -1 is an IrisError, not a table"""
    from iris_amd import _lib as L
    from iris_amd.model.slf import VoxelSLF
    dev = torch.device("cuda:0")
    mask = torch.from_numpy(np.array(V.grid_tables(2)["mask"]))                # H = 31
    s = VoxelSLF(mask if path == "host" else mask.to(dev), -0.37, 4.21)
    kv = s.radiance.shape[0]
    x = torch.from_numpy(np.array(V.table(2, 64)[0])).to(dev)
    assert s.spatial_idx(x).shape == (64,)                                     # a good table first: the refusal below is the entry's doing
    s.inds[30, 17, 5] = {"kv": kv, "kv+5": kv + 5, "-2": -2, "int64-min": V.INT64_MIN}[entry]
    with pytest.raises(L.IrisError):
        s.spatial_idx(x)
