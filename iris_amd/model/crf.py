"""The learned camera response model (reference: crf/model_crf.py:32-122, crf/emor.py:19-38) with its lookups as fused HIP kernels.

EmorCRF keeps the reference's surface -- constructor, ``forward(hdr, exposure)``, ``inverse(ldr, exposure)``, ``get_crf``, ``get_inv_crf``, the three
regularisers, ``initialize_weight`` / ``cal_weight_fitting_crf`` and the ``state_dict`` keys f0, basis, weight -- so that the stages that use it
(train_brdf_crf.py:206, initialize.py:183, train_emitter.py:192, slf_bake.py:129, slf_refine.py:97, extract_emitter_ldr.py) swap an import.

    model_crf = EmorCRF(dim=11)                          # reads crf/emor.txt under the working directory, as the reference does
    model_crf = EmorCRF.from_arrays(f0, basis)           # for callers that hold the EMoR basis already
    rgbs_ldr = model_crf(L, exposure)                    # differentiable in L and in model_crf.weight
    radiance = model_crf.inverse(rgbs, exposure)         # no gradient

The reference interpolates with torch_interpolations, which has no ROCm build; the interpolator here is the project's own contract (include/iris_hip.h,
iris_amd/csrc/iris_crf.h): parity with that package is unpinned.  The EMoR file is data the user brings; the package ships none of it.  What acts on the
3 x n table (get_crf, the regularisers, the weight fit) is plain torch and works on the CPU too; forward and inverse need a HIP device.
"""
import os

import numpy as np
import torch

from .. import _lib as L

MAX_KNOTS = 1024          # the kernels keep the tables in LDS


def parse_emor_file(path):
    """-> (names, vectors): the blocks of an EMoR file (emor.txt / invemor.txt), each a ``name =`` line followed by lines of numbers (256 lines of four
    in the published files).  names: numpy array of str; vectors: (blocks, length) float32.  Block 0 is the grid E, 1 is f0, 2.. are the basis h(k)."""
    names, blocks = [], []
    with open(path, "r") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if "=" in line:
                head, tail = line.split("=", 1)
                names.append(head.strip())
                blocks.append(tail.split())
            elif not blocks:
                raise ValueError(f"{path}: numbers before the first 'name =' line")
            else:
                blocks[-1].extend(line.split())
    if not blocks:
        raise ValueError(f"{path}: no 'name =' block found")
    lengths = {len(b) for b in blocks}
    if len(lengths) != 1 or 0 in lengths:
        raise ValueError(f"{path}: blocks of different or zero length {sorted(lengths)}")
    return np.array(names), np.stack([np.array(b, dtype=np.float32) for b in blocks])


def _exposure_args(exposure, B, device):
    """(tensor or None, count, host value) for the kernels: a python number or a one-element host tensor travels by value, a one-element device tensor
    by pointer (nothing synchronises), B values per pixel.  Never differentiated."""
    if not torch.is_tensor(exposure):
        return None, 1, float(exposure)
    e = exposure.detach()
    if e.numel() == 1 and not e.is_cuda:
        return None, 1, float(e)
    if e.numel() != 1 and e.numel() != B:
        raise ValueError(f"exposure has {e.numel()} values, expected 1 or {B} (one per pixel)")
    e = e.reshape(-1).to(device=device, dtype=torch.float32).contiguous()
    return e, e.numel(), 0.0


def _pixels(t, name):
    if t.dim() < 1 or t.shape[-1] != 3:
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected (..., 3)")
    return L.require_gpu(t.detach(), torch.float32, name).reshape(-1, 3)


def _check_tables(table, grid):
    table, grid = L.require_gpu(table.detach(), torch.float32, "table"), L.require_gpu(grid, torch.float32, "grid")
    if table.dim() != 2 or table.shape[0] != 3 or not 2 <= table.shape[1] <= MAX_KNOTS or grid.shape != (table.shape[1],):
        raise ValueError(f"table {tuple(table.shape)} / grid {tuple(grid.shape)}: expected (3, n) and (n,) with 2 <= n <= {MAX_KNOTS}")
    return table, grid


class _CrfLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hdr, table, grid, exposure):
        x = _pixels(hdr, "hdr")
        tab, grid = _check_tables(table, grid)
        B, n = x.shape[0], tab.shape[1]
        e, ne, ev = _exposure_args(exposure, B, x.device)
        ldr = torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.check(L.lib().iris_crf_fwd(L.ptr(grid), L.ptr(tab), n, L.ptr(x), L.ptr(e), ne, ev, B, L.ptr(ldr), L.stream()))
        ctx.save_for_backward(x, tab, grid, e if e is not None else torch.empty(0, device=x.device))
        ctx.exposure, ctx.hdr_shape, ctx.table_shape = (e is not None, ne, ev), hdr.shape, table.shape
        return ldr.reshape(hdr.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_ldr):
        x, tab, grid, e = ctx.saved_tensors
        has_e, ne, ev = ctx.exposure
        B, n, dev = x.shape[0], tab.shape[1], x.device
        g = L.require_gpu(g_ldr, torch.float32, "g_ldr").reshape(-1, 3)
        g_hdr = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        g_table = torch.empty_like(tab) if ctx.needs_input_grad[1] else None
        ws_bytes = L.lib().iris_crf_bwd_workspace_bytes(B, n) if g_table is not None else 0
        ws = torch.empty(max(ws_bytes, 4) // 4, device=dev, dtype=torch.float32) if g_table is not None else None
        with torch.cuda.device(dev):
            L.check(L.lib().iris_crf_bwd(L.ptr(grid), L.ptr(tab), n, L.ptr(x), L.ptr(e) if has_e else None, ne, ev, B, L.ptr(g), L.ptr(g_hdr), L.ptr(g_table),
                                         L.ptr(ws), ws_bytes, L.stream()))
        return (g_hdr.reshape(ctx.hdr_shape) if g_hdr is not None else None, g_table.reshape(ctx.table_shape) if g_table is not None else None, None, None)


def crf_lookup(hdr, table, grid, exposure):
    """ldr (..., 3) = interp(grid, table[c], clip(hdr * exposure, 0, 1)) per channel c: model_crf.py:68-86 with the (3, n) table and its (n,) knots given.
    Differentiable in hdr and table; exposure (python number, one value, (B,) or (B, 1)) never gets a gradient.  A hdr that is not contiguous is copied."""
    return _CrfLookup.apply(hdr, table, grid, exposure)


def crf_inverse_table(table, grid):
    """get_inv_crf (model_crf.py:45-55) of a (3, n) table on the device, without gradient"""
    tab, grid = _check_tables(table, grid)
    inv = torch.empty_like(tab)
    with torch.cuda.device(tab.device):
        L.check(L.lib().iris_crf_inv_table(L.ptr(grid), L.ptr(tab), tab.shape[1], L.ptr(inv), L.stream()))
    return inv


def crf_lookup_inverse(ldr, inv_table, grid, exposure):
    """hdr (..., 3) = interp(grid, inv_table[c], clip(ldr, 0, 1)) / exposure: model_crf.py:88-106 with the inverse table given.  No gradient."""
    x = _pixels(ldr, "ldr")
    inv, grid = _check_tables(inv_table, grid)
    e, ne, ev = _exposure_args(exposure, x.shape[0], x.device)
    hdr = torch.empty_like(x)
    with torch.cuda.device(x.device):
        L.check(L.lib().iris_crf_lookup_inv(L.ptr(grid), L.ptr(inv), inv.shape[1], L.ptr(x), L.ptr(e), ne, ev, x.shape[0], L.ptr(hdr), L.stream()))
    return hdr.reshape(ldr.shape)


class EmorCRF(torch.nn.Module):
    """crf = f0 + weight @ basis: the EMoR mean curve plus `dim` basis curves per colour channel, sampled at n points of [0, 1]."""

    def __init__(self, dim=11, emor_path=None, _arrays=None):
        super().__init__()
        self.dim = dim
        if _arrays is None:
            path = os.path.join(os.getcwd(), "crf", "emor.txt") if emor_path is None else os.fspath(emor_path)
            if not os.path.isfile(path):
                raise FileNotFoundError(f"{path}: the EMoR basis file is missing (it is data the user brings: emor.txt of the EMoR model; pass emor_path=, "
                                        "or build the model from arrays with EmorCRF.from_arrays(f0, basis))")
            _, vectors = parse_emor_file(path)
            if len(vectors) < 2 + dim:
                raise ValueError(f"{path}: {len(vectors)} blocks, dim={dim} needs {2 + dim} (E, f0, h(1)..h({dim}))")
            f0, basis = vectors[1], vectors[2:2 + dim]
        else:
            f0, basis = _arrays
        f0 = torch.as_tensor(np.asarray(f0, dtype=np.float32)).reshape(1, -1).clone()
        basis = torch.as_tensor(np.asarray(basis, dtype=np.float32)).reshape(dim, -1).clone()
        if basis.shape[1] != f0.shape[1] or not 2 <= f0.shape[1] <= MAX_KNOTS:
            raise ValueError(f"f0 {tuple(f0.shape)} and basis {tuple(basis.shape)}: expected (1, n) and (dim, n) with 2 <= n <= {MAX_KNOTS}")
        self.register_buffer("f0", f0)
        self.register_buffer("basis", basis)
        # the knots: linspace computed on the host and moved with the module, as the reference's torch.linspace(0, 1, n).to(device); not part of the state dict
        self.register_buffer("grid", torch.linspace(0, 1, f0.shape[1]), persistent=False)
        self.weight = torch.nn.Parameter(torch.zeros(3, dim))

    @classmethod
    def from_arrays(cls, f0, basis):
        """f0: n values, basis: (dim, n) -- rows 1 and 2.. of parse_emor_file's vectors"""
        basis = np.asarray(basis.detach().cpu() if torch.is_tensor(basis) else basis, dtype=np.float32)
        f0 = np.asarray(f0.detach().cpu() if torch.is_tensor(f0) else f0, dtype=np.float32)
        if basis.ndim != 2:
            raise ValueError(f"basis has shape {basis.shape}, expected (dim, n)")
        return cls(dim=basis.shape[0], _arrays=(f0, basis))

    def get_crf(self):
        return self.f0 + self.weight @ self.basis

    def get_inv_crf(self):
        """(3, n) inverse response table of the current weights.  Runs without gradient and returns a detached tensor: the reference only calls it in
        its no-grad stages (slf_bake.py, slf_refine.py, extract_emitter_ldr.py)."""
        with torch.no_grad():
            return crf_inverse_table(self.get_crf(), self.grid)

    def initialize_weight(self, crf):
        """replaces the parameter by the least-squares fit of the three curves crf (3, n), numpy"""
        fitted = torch.from_numpy(self.cal_weight_fitting_crf(crf))
        self.weight = torch.nn.Parameter(fitted.to(device=self.weight.device, dtype=torch.float32))

    def cal_weight_fitting_crf(self, crf):
        """least-squares weights (k, dim) float32 of the curves crf (k, n), numpy: argmin_w |f0 + w @ basis - crf|, solved in float64 by an orthogonal
        factorisation (lstsq) -- the answer the reference's float32 normal equations approximate"""
        curves = np.asarray(crf, dtype=np.float64).reshape(-1, self.f0.shape[1])
        residual = curves - self.f0.detach().cpu().numpy().astype(np.float64)
        design = self.basis.detach().cpu().numpy().astype(np.float64).T           # (n, dim): one column per basis curve
        solution = np.linalg.lstsq(design, residual.T, rcond=None)[0]             # (dim, k)
        return np.ascontiguousarray(solution.T, dtype=np.float32)

    def forward(self, hdr, exposure):
        """hdr (B, 3) linear radiance -> ldr (B, 3); differentiable in hdr and, through get_crf's matmul, in weight"""
        return crf_lookup(hdr, self.get_crf(), self.grid, exposure)

    def inverse(self, ldr, exposure):
        """ldr (B, 3) -> hdr (B, 3) through the inverse table, rebuilt at every call as the reference does.  Runs without gradient and returns a
        detached tensor."""
        L.require_gpu(ldr, torch.float32, "ldr")
        return crf_lookup_inverse(ldr, self.get_inv_crf(), self.grid, exposure)

    def reg_weight(self):
        return torch.mean(self.weight ** 2)

    def reg_monotonically_increasing(self):
        crf = self.get_crf()
        return torch.sum(torch.relu(crf[:, :-1] - crf[:, 1:]))

    def reg_smoothness(self):
        crf = self.get_crf()
        return torch.mean((crf[:, :-2] + crf[:, 2:] - 2 * crf[:, 1:-1]) ** 2)
