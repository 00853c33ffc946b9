"""The camera response model's arithmetic in plain torch: the yardstick of tests/test_crf*.py and the interpolator tools/make_crf_golden.py installs
under the reference's EmorCRF (crf/model_crf.py), whose own interpolator (torch_interpolations) is a third-party package that is not available.

The interpolator contract is the project's (include/iris_hip.h).  Knots p[0..n) non-decreasing, values v[0..n), query q:
    r = first index with p[r] >= q, clamped to n - 1 (torch.bucketize);  l = max(r - 1, 0)
    dl = max(q - p[l], 0);  dr = max(p[r] - q, 0);  both zero -> both 1
    out = (v[l] * dr + v[r] * dl) / (dl + dr)
    d out / d q = (v[r] - v[l]) / (dl + dr), 0 where both were zero;  d out / d v[l] = dr / (dl + dr),  d out / d v[r] = dl / (dl + dr)
The derivatives are stated, not left to autograd's chain through the quotient, so that a float32 run has one rounding per stated operation.
Everything works in the dtype of its inputs (float32 as the model runs, float64 as the yardstick) and on any device.
"""
import torch


def segment(p, q):
    """(l, r, dl, dr, flat) of the contract; flat marks the queries whose two distances were both zero"""
    n = p.shape[0]
    r = torch.bucketize(q.contiguous(), p).clamp(max=n - 1)
    l = (r - 1).clamp(min=0)
    dl = (q - p[l]).clamp(min=0)
    dr = (p[r] - q).clamp(min=0)
    flat = (dl == 0) & (dr == 0)
    one = torch.ones_like(dl)
    return l, r, torch.where(flat, one, dl), torch.where(flat, one, dr), flat


class _Interp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, v, q):
        l, r, dl, dr, flat = segment(p, q)
        ctx.save_for_backward(v, l, r, dl, dr, flat)
        return (v[l] * dr + v[r] * dl) / (dl + dr)

    @staticmethod
    def backward(ctx, g):
        v, l, r, dl, dr, flat = ctx.saved_tensors
        den = dl + dr
        g_q = g * torch.where(flat, torch.zeros_like(den), (v[r] - v[l]) / den)
        g_v = torch.zeros_like(v).index_add_(0, l.reshape(-1), (g * (dr / den)).reshape(-1)).index_add_(0, r.reshape(-1), (g * (dl / den)).reshape(-1))
        return None, g_v, g_q


def interp(p, v, q):
    """values v over knots p at the queries q (any shape); differentiable in v and q as the contract states"""
    return _Interp.apply(p, v, q)


class RegularGridInterpolator:
    """The one-dimensional use crf/model_crf.py makes of torch_interpolations: RegularGridInterpolator([points], values)([queries])"""

    def __init__(self, points, values):
        assert len(points) == 1 and values.dim() == 1
        self.points, self.values = points[0], values

    def __call__(self, queries):
        assert len(queries) == 1
        return interp(self.points, self.values, queries[0])


def linspace(n, like):
    """torch.linspace(0, 1, n) computed in float32 on the CPU, as the model holds it, in the dtype and on the device of `like`"""
    return torch.linspace(0, 1, n).to(device=like.device, dtype=like.dtype)


def get_crf(f0, basis, weight):
    return f0 + weight @ basis


def forward(table, hdr, exposure):
    """model_crf.py:68-86: (B, 3) -> (B, 3)"""
    q = torch.clip(hdr * exposure, 0, 1)
    x = linspace(table.shape[1], table)
    return torch.stack([interp(x, table[c], q[:, c]) for c in range(3)], dim=-1)


def knots_of(crf_ch):
    """model_crf.py:22-30: the channel's table made non-decreasing from 0 to 1"""
    d = crf_ch[1:] - crf_ch[:-1]
    m = d.min()
    if m < 0:
        d = d + (-m)
    d = d / d.sum()
    return torch.cat([torch.zeros(1, dtype=d.dtype, device=d.device), torch.cumsum(d, dim=0)])


def inv_table(table):
    """model_crf.py:45-55: (3, n) -> (3, n)"""
    x = linspace(table.shape[1], table)
    return torch.stack([interp(knots_of(table[c]), x, x) for c in range(3)], dim=0)


def inverse(inv, ldr, exposure):
    """model_crf.py:88-106 with the inverse table given"""
    q = torch.clip(ldr, 0, 1)
    x = linspace(inv.shape[1], inv)
    return torch.stack([interp(x, inv[c], q[:, c]) for c in range(3)], dim=-1) / exposure


def regularisers(table, weight):
    """(reg_weight, reg_monotonically_increasing, reg_smoothness) of model_crf.py:108-122"""
    d = table[:, 1:] - table[:, :-1]
    s = table[:, :-2] + table[:, 2:] - 2 * table[:, 1:-1]
    return torch.mean(weight ** 2), torch.sum(torch.relu(-d)), torch.mean(s ** 2)


# ---- how tests/golden/crf_emor.npz was taken (tools/make_crf_golden.py), shared with the tests that replay it
def cotangent(n):
    """(n, 3) float32 cotangent of the fixture's gradients: ((3 i + c) mod 7 - 3) / 4, exact in float32, so it is not stored"""
    return ((torch.arange(n * 3) % 7).float().reshape(n, 3) - 3) / 4


def by_block(fn, x, e_pixel, block):
    """fn(rows, exposure) over the fixture's three blocks of rows with their exposures (python floats 1.0 and 1.7, then one value per pixel), concatenated"""
    exposures = (1.0, 1.7, e_pixel)
    return torch.cat([fn(x[block[k]:block[k + 1]], exposures[k]) for k in range(3)])
