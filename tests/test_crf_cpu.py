"""The camera response model without a GPU (iris_amd/model/crf.py; reference crf/model_crf.py, crf/emor.py).

tests/golden/crf_emor.npz holds the reference's own EmorCRF run on the CPU in float32 (tools/make_crf_golden.py) with the project's interpolator
(tools/crf_restatement.py) in the place of torch_interpolations.  Checked here:
  - the parser, on a file of the published layout written by the test;
  - the methods kept in plain torch (get_crf, the regularisers, the weight fit, load_state_dict with the reference's keys) against the golden, to the
    rounding of their sums: K 2^-24 sum |terms| for K addends (the summation order is the BLAS's and the vector width's), relative to the value itself
    where the terms have one sign; no slack beyond that, so a golden value of zero has to be met exactly;
  - that the restatement -- our statement of the model, the GPU tests' yardstick -- reproduces the reference's outputs bit for bit from the golden's
    tables (same operations in the same order, one rounding each), up to the sign of a zero;
  - the refusals: CPU tensors, a missing EMoR file.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from iris_amd import _lib as L
from iris_amd.model.crf import EmorCRF, parse_emor_file
from tools import crf_restatement as R

U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def fixture():
    g = golden("crf_emor.npz")
    return {k: (torch.from_numpy(g[k]) if g[k].dtype == np.float32 else g[k]) for k in g.files}


def same_bits(a, b):
    """bitwise equality up to the sign of a zero (x + 0 turns -0 into +0)"""
    return torch.equal((a + 0.0).view(torch.int32), (b + 0.0).view(torch.int32))


def model_of(f, k):
    m = EmorCRF.from_arrays(f["f0"][0], f["basis"])
    m.load_state_dict({"f0": f["f0"], "basis": f["basis"], "weight": f[f"weight_{k}"]})        # the model_crf.* keys of a reference checkpoint
    return m


def test_parser_reads_the_published_layout(tmp_path):
    rng = np.random.default_rng(0)
    vectors = rng.random((3, 1024)).astype(np.float32)
    vectors[0] = np.linspace(0, 1, 1024, dtype=np.float32)
    names = ["E", "f0", "h(1)"]
    with open(tmp_path / "emor.txt", "w") as f:
        for name, v in zip(names, vectors):
            f.write(f"{name} = \n" if name != "h(1)" else "h(1)=\n")
            for row in v.reshape(256, 4):
                f.write("   ".join(f"{x:.9e}" for x in row) + "\n")
    got_names, got = parse_emor_file(tmp_path / "emor.txt")
    assert list(got_names) == names
    assert got.dtype == np.float32 and got.shape == (3, 1024)
    np.testing.assert_array_equal(got, vectors)                   # nine significant digits round-trip a float32
    with pytest.raises(ValueError):
        (tmp_path / "bad.txt").write_text("1.0 2.0\nE =\n0.5\n")
        parse_emor_file(tmp_path / "bad.txt")


def test_constructor_reads_crf_emor_txt_under_the_working_directory(tmp_path, monkeypatch):
    f = fixture()
    (tmp_path / "crf").mkdir()
    blocks = [("E", np.linspace(0, 1, 1024, dtype=np.float32)), ("f0", f["f0"][0].numpy())] + [(f"h({k + 1})", f["basis"][k].numpy()) for k in range(11)]
    with open(tmp_path / "crf" / "emor.txt", "w") as out:
        for name, v in blocks:
            out.write(f"{name} = \n")
            for row in v.reshape(256, 4):
                out.write("   ".join(f"{x:.9e}" for x in row) + "\n")
    monkeypatch.chdir(tmp_path)
    m = EmorCRF(dim=5)
    assert m.dim == 5 and sorted(m.state_dict()) == ["basis", "f0", "weight"]
    assert torch.equal(m.f0, f["f0"]) and torch.equal(m.basis, f["basis"][:5]) and float(m.weight.detach().abs().max()) == 0.0 and m.weight.shape == (3, 5)
    with pytest.raises(ValueError):
        EmorCRF(dim=12)                                           # the file holds eleven basis curves


@pytest.mark.parametrize("k", [0, 1, 2])
def test_torch_side_methods_equal_the_golden(k):
    f = fixture()
    m = model_of(f, k)
    table, w, basis = f[f"table_{k}"], f[f"weight_{k}"], f["basis"]
    crf = m.get_crf()
    assert crf.shape == (3, 1024) and m.weight.requires_grad
    bound = 12 * U * (f["f0"].abs() + w.abs() @ basis.abs()) + 1e-30                 # 11 products and the sum with f0
    assert bool(((crf.detach() - table).abs() <= bound).all())
    dt = (crf.detach() - table).abs().double()                                        # measured, bounded above; 0 where both sides ran the same matmul
    d = (table[:, 1:] - table[:, :-1]).double()
    s = (table[:, :-2] + table[:, 2:] - 2 * table[:, 1:-1]).double()
    regs = f[f"regs_{k}"].double()
    got = torch.stack([m.reg_weight(), m.reg_monotonically_increasing(), m.reg_smoothness()]).detach().double()
    # float32 sums of 33, 3069 and 3066 non-negative terms (three more roundings per term): relative to the value itself, terms * 2^-24.  The last two
    # are functions of the table, so what the table itself deviates by (dt) is carried through them: |relu(a) - relu(b)| <= |a - b|, and
    # |a^2 - b^2| <= (2 |a| + |a - b|) |a - b|.  With dt = 0 a zero golden value has to be met exactly.
    carried_d = dt[:, 1:] + dt[:, :-1]
    carried_s = dt[:, :-2] + dt[:, 2:] + 2 * dt[:, 1:-1]
    tol = torch.stack([(33 + 3) * U * regs[0], (3069 + 3) * U * regs[1] + carried_d.sum(), (3066 + 6) * U * regs[2] + ((2 * s.abs() + carried_s) * carried_s).mean()])
    print(f"case {k}: table deviation {float(dt.max()):.3g}; regs {got.tolist()} golden {regs.tolist()} tolerance {tol.tolist()}")
    assert bool(((got - regs).abs() <= tol).all())
    assert float(torch.relu(-d).sum()) == pytest.approx(float(regs[1]), rel=1e-5, abs=1e-12)     # the golden agrees with its own table
    # the weight fit.  The basis is orthonormal to rounding (cond of its Gram matrix printed below), so the golden's float32 normal equations are, per
    # entry, a 1024-term float32 dot product of a unit basis row with r = crf - f0: its error is at most 1024 * 2^-24 * sum |b_j r_j| <= 1024 * 2^-24 * |r|_2
    # (Cauchy-Schwarz), times cond for the solve; 64 more units for the subtraction, the 11 x 11 inverse and the product with it.  The fit under test
    # is solved in float64 and rounded once.  A zero curve has to give exactly zero.
    basis64 = basis.double()
    cond = float(torch.linalg.cond(basis64 @ basis64.T))
    fit = m.cal_weight_fitting_crf(table.numpy())
    assert isinstance(fit, np.ndarray) and fit.shape == (3, 11) and fit.dtype == np.float32
    r_norm = (table - f["f0"]).double().norm(dim=1)
    fit_dev = (torch.from_numpy(fit).double() - f[f"fit_{k}"].double()).abs().max(dim=1).values
    fit_tol = (1024 + 64) * U * cond * r_norm
    # and against the weights the table was made from: the table's own rounding (bound) seen through the orthonormal basis, |b . delta| <= |delta|_2
    back_dev = (torch.from_numpy(fit).double() - w.double()).abs().max(dim=1).values
    back_tol = cond * bound.double().norm(dim=1) + U * w.abs().max(dim=1).values
    print(f"case {k}: cond {cond:.9g}; fit against the golden {fit_dev.tolist()} (tolerance {fit_tol.tolist()}); against the weights {back_dev.tolist()} (tolerance {back_tol.tolist()})")
    assert cond < 1.001
    assert bool((fit_dev <= fit_tol).all()) and bool((back_dev <= back_tol).all())
    m2 = model_of(f, 0)
    m2.initialize_weight(table.numpy())
    assert isinstance(m2.weight, torch.nn.Parameter) and m2.weight.dtype == torch.float32 and m2.weight.shape == (3, 11) and m2.weight.requires_grad
    assert torch.equal(m2.weight.detach(), torch.from_numpy(fit))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_restatement_reproduces_the_reference_bit_for_bit(k):
    f = fixture()
    x, e_pixel, block = f["x"], f["e_pixel"], f["block"]
    table = f[f"table_{k}"].clone().requires_grad_(True)
    h = x.clone().requires_grad_(True)
    ldr = R.by_block(lambda rows, e: R.forward(table, rows, e), h, e_pixel, block)
    g_hdr, g_table = torch.autograd.grad((ldr * R.cotangent(len(x))).sum(), (h, table))
    assert same_bits(ldr.detach(), f[f"ldr_{k}"])
    assert same_bits(g_hdr, f[f"ghdr_{k}"])
    inv = R.inv_table(table.detach())
    assert same_bits(inv, f[f"inv_{k}"])
    assert same_bits(R.by_block(lambda rows, e: R.inverse(f[f"inv_{k}"], rows, e), x, e_pixel, block), f[f"hdr_{k}"])
    # weight.grad = g_table @ basis^T: 1024 addends in the BLAS's order
    gw = g_table @ f["basis"].T
    bound = 1024 * U * (g_table.abs() @ f["basis"].abs().T)
    assert bool(((gw - f[f"gweight_{k}"]).abs() <= bound).all())
    regs = torch.stack(R.regularisers(f[f"table_{k}"], f[f"weight_{k}"]))
    np.testing.assert_allclose(regs.numpy(), f[f"regs_{k}"].numpy(), rtol=3069 * U, atol=1e-12)


def test_golden_covers_the_gap_branch_and_the_plain_one():
    f = fixture()
    mins = [float((f[f"table_{k}"][:, 1:] - f[f"table_{k}"][:, :-1]).min()) for k in range(int(f["n_cases"]))]
    assert min(mins) < 0 <= max(mins), mins
    knots = torch.stack([R.knots_of(f["table_2"][c]) for c in range(3)])
    assert bool((knots[:, 1:] == knots[:, :-1]).any()), "the gap makes the smallest difference zero: a repeated knot"
    assert bool((knots[:, 1:] >= knots[:, :-1]).all())


def test_refusals(tmp_path):
    f = fixture()
    m = model_of(f, 1)
    with pytest.raises(L.IrisError, match="no CPU path"):
        m(torch.rand(4, 3), 1.0)
    with pytest.raises(L.IrisError, match="no CPU path"):
        m.inverse(torch.rand(4, 3), 1.0)
    missing = tmp_path / "nowhere" / "emor.txt"
    with pytest.raises(FileNotFoundError) as err:
        EmorCRF(emor_path=missing)
    assert str(missing) in str(err.value) and "from_arrays" in str(err.value)
    with pytest.raises(ValueError):
        EmorCRF.from_arrays(np.zeros(2048, np.float32), np.zeros((3, 2048), np.float32))        # more knots than the kernels keep in LDS
