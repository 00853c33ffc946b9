"""NGPBRDF (iris_amd/csrc/iris_ngp.h) in the regime the trainer runs it in: the inputs, the restated backward and the per-element envelope that
tests/test_ngp_regime_cpu.py (no GPU: vouches for all of this from the reference alone) and tests/test_ngp_regime.py (MI355X) share.

Parameter sets
  init     NGPBRDF.init_parameters(1337), restated here so that it exists without the native library (the GPU test asserts the bits are the module's):
           tables U(-1e-4, 1e-4): ~95 % of the encoded features, and about half of the non-zero hidden activations, are SUBNORMAL halves; every output is 0.5
  uniform  test_ngp_backward's +-0.3
  mixed    a checkpoint-like state: table magnitudes log-uniform over 2^-26 .. 2^-3 with random sign (values that round to zero in half, subnormals,
           normals), every 8th table float an exact TIE between two neighbouring halves; the three matrices Xavier-uniform x 4, so that outputs leave 0.5
  saturated  `mixed` with W3 x 8 (1 and 33 points, cotangents of order 1): sigmoids beyond 0.98, where half an ulp of s is percents of s (1 - s) -- the one input
           on which a sigmoid derivative taken from the unrounded s leaves the bar (mixed's own outputs stay within 0.11 .. 0.92)
  dyadic   test_ngp.py's exact network moved into the subnormal range (features 2^-15 / -2^-16, W3 in {-1,0,1} * 2^14 [* 2]): every dot product exact in f32

Backward.  reference = test_ngp_backward.f64_gradient (straight-through definition, float64, on the oracle's forward values).  Beside it:
  restated_gradient  DESIGN.md section 5f in float64 with the kernel's roundings: dz3 * loss_scale -> half, dz2 / dz1 -> half after the mask, half operands in every
                     product, / loss_scale at the end; and its mutants (MUTANTS)
  envelope           tol_i, derived (not fitted).  u = 2^-11, q = 2^-25 (half the subnormal quantum of half), f = 2^-24 (f32).  Working in scaled units (x loss_scale):
      e3 = r(|dz3|) + 4 f |dz3| + |g| ls ds                    r(x) = max(u x, q) for x > 0: one rounding to half;  4 f: the f32 products of dz3;
                                                              ds: what s can differ by where the output pre-activation is within its f32 bound of a rounding boundary
      e2 = mask2 (eh2 + r(|W3^T dz3| + eh2)),  eh2 = e3 |W3| + 16 f (|dz3| |W3|)         errors propagate as magnitudes, without cancellation
      e1 = mask1 (eh1 + r(|W2^T dz2| + eh1)),  eh1 = e2 |W2| + 64 f (A2 |W2|)            A = the propagated magnitudes: A3 = |dz3|, A2 = mask2 (A3 |W3|), ...
      an UNDECIDED (point, neuron) pair -- exact pre-activation (float64 over the half operands) within its summation bound of zero, the bound of layer 2
      including the activation uncertainty dH1 |W2| -- may carry the other mask: e = the full masked term + the above
      tol(dW3) = e3^T |H2| + (|dz3| + e3)^T dH2 + (n + 4) f A3^T |H2|       dH: the half-ulp steps H can differ by (pre-activation within its bound of a boundary)
      tol(dW2) = e2^T |H1| + (|dz2| + e2)^T dH1 + (n + 4) f A2^T |H1|       (n + 4) f: f32 summation over the points in any order
      tol(dW1) = e1^T |X|  + (n + 4) f A1^T |X|                             (X is bit-exact: no dX term)
      tol(table entry) = sum_corners w (e1 |W1| + 64 f AX) + (count + 4) f sum_corners w AX,  AX = A1 |W1|      count: the atomic adds the entry receives
      all divided by loss_scale.
Constants: E = worst |restated - reference| / tol per block class (dW1, dW2, dW3, tables) and input, measured when the tests run; E > 1 fails as a fault of the
derivation; the kernel is held to C tol, C = 4 E.

Measured (seeds as below): E 0.002 .. 0.98 over the 30 inputs x 4 classes (largest per class: dW1 0.17, dW2 0.94, dW3 0.98, tables 0.10; at 2 500 points 0.004 .. 0.11);
on an MI355X the kernel's worst |err| / (C tol) is 0.232 .. 0.276 -- the restatement's own 0.25: its element errors ARE the restated roundings.  DESIGN.md section 5f."""
import functools
import math
import sys

import numpy as np
import torch

from conftest import REPO

sys.path.insert(0, REPO)
from oracle import ngp_torch as ng     # noqa: E402
from test_ngp_backward import N_MLP, VMAX, VMIN, _blocks, _corners, _cotangents, _forward_values, _params, _positions, f64_gradient     # noqa: E402,F401

U, Q, F, TINY = 2.0 ** -11, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14
LOSS_SCALE = 128.0
SCALES = (1.0, 3e-5, 1e-6)            # cotangents: the tests as they are; a trainer batch of 8192 x 3 early on; the same batch late
SIZES = (1, 33, 2500)
CLASSES = ("dW1", "dW2", "dW3", "tables")
UNDECIDED_CAP = 1e-3


def d(t):
    return t.to(torch.float64)


def h64(t):
    """float64 -> the nearest half (ties to even, ONE rounding: numpy converts directly), as float64"""
    return torch.from_numpy(t.numpy().astype(np.float16).astype(np.float64))


def trunc_h64(t):
    """float64 -> the neighbouring half TOWARDS ZERO (a mutant's rounding)"""
    r = t.numpy().astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(t.numpy())
    return torch.from_numpy(np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float64))


def is_subnormal(t):
    a = d(t).abs()
    return (a < TINY) & (a > 0)


def flush(t):
    """subnormal halves -> 0: what an instruction that does not keep denormal inputs would read"""
    return torch.where(d(t).abs() < TINY, torch.zeros_like(t), t)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# parameter sets and inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _xavier(g, scale=1.0):
    out = []
    for rows, cols in ((64, 64), (64, 64), (16, 64)):
        out.append((torch.rand(rows * cols, generator=g) * 2 - 1) * (math.sqrt(6.0 / (rows + cols)) * scale))
    return torch.cat(out)


@functools.lru_cache(maxsize=None)
def parameters(name):
    """never modified by a test (clone before writing)"""
    n = ng.n_params()
    if name == "init":                                       # iris_amd/model/brdf.py, NGPBRDF.init_parameters(1337): the same draws in the same order
        g = torch.Generator().manual_seed(1337)
        w = _xavier(g)
        return torch.cat([w, (torch.rand(n - N_MLP, generator=g) * 2 - 1) * 1e-4])
    if name == "uniform":
        return _params(4, 0.3)
    if name == "mixed":
        g = torch.Generator().manual_seed(21)
        w = _xavier(g, 4.0)
        k = n - N_MLP
        mag = torch.exp2(torch.rand(k, generator=g, dtype=torch.float64) * 23.0 - 26.0)
        sign = torch.randint(0, 2, (k,), generator=g).to(torch.float64) * 2 - 1
        tab = mag * sign
        ties = (torch.randint(0, 2048, (k // 8,), generator=g).to(torch.float64) + 0.5) * 2.0 ** -24      # halfway between two halves below 2^-13
        tab[::8] = ties * sign[::8]
        return torch.cat([w, tab.to(torch.float32)])
    if name == "saturated":                                  # `mixed` with W3 x 8: sigmoids up to 0.99 and beyond, where half an ulp of s is percents of s (1 - s)
        p = parameters("mixed").clone()
        p[8192:N_MLP] *= 8.0
        return p
    raise KeyError(name)


def dyadic_parameters(w3_scale=1.0):
    """test_ngp.py::test_hip_forward_exact_with_dyadic_weights, in the subnormal range: features 2^-15 / -2^-16 (one constant per table feature), W1 in
    {-2..2}/8, W2 in {-1,0,1}/4, W3 in {-1,0,1} * 2^14 * w3_scale.  Layer-1 sums are multiples of 2^-19 below 2^-10, layer 2's multiples of 2^-26, layer 3's
    multiples of 2^-12 * w3_scale below 2^6: every sum exact in f32 in any order.  Returns (params, positions in the unit box)."""
    g = torch.Generator().manual_seed(7)
    params = torch.zeros(ng.n_params())
    params[:4096] = torch.randint(-2, 3, (4096,), generator=g).float() / 8
    params[4096:8192] = torch.randint(-1, 2, (4096,), generator=g).float() / 4
    params[8192:N_MLP] = torch.randint(-1, 2, (N_MLP - 8192,), generator=g).float() * (2.0 ** 14 * w3_scale)
    grid = params[N_MLP:].reshape(-1, 2)
    grid[:, 0] = 2.0 ** -15; grid[:, 1] = -2.0 ** -16
    pos = torch.rand(4096, 3, generator=g)
    return params, pos


def dyadic_forward(params, pos, accumulate=torch.float32, flushed=False, permute=False):
    """the oracle's forward on the unit box with its intermediates; `flushed`: subnormal half operands read as zero (the mutant); `permute`: another summation order"""
    op = flush if flushed else (lambda t: t)
    w = params[:N_MLP].to(torch.float16)
    W1, W2, W3 = w[:4096].reshape(64, 64), w[4096:8192].reshape(64, 64), w[8192:].reshape(16, 64)
    X = ng.encode(params, pos * 2 - 1)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(3)) if permute else torch.arange(64)
    mm = lambda a, W: op(a).to(accumulate)[:, perm] @ op(W).to(accumulate)[:, perm].T
    H1 = torch.relu(mm(X, W1)).to(torch.float16)
    H2 = torch.relu(mm(H1, W2)).to(torch.float16)
    pre = mm(H2, W3)[:, :5]
    s = torch.sigmoid(pre.to(torch.float16).float()).to(torch.float16).float()
    return dict(X=X, H1=H1, H2=H2, pre=pre, s=s)


def outputs_of(s):
    """(n, 5) half-grid sigmoids -> the network's three outputs"""
    return {"albedo": s[:, :3].contiguous(), "roughness": s[:, 3:4] * np.float32(0.98) + np.float32(0.02), "metallic": s[:, 4:5].contiguous()}


CLUSTER_CELL = (3, 4, 5)     # a level-0 cell (scale 15: p = 15 x + 0.5 in [cell, cell + 1))


def positions(kind):
    """'1' / '33' / '2500': uniform in the box (test_ngp_backward's); 'cluster': 2 500 points inside ONE level-0 cell, so that each of its 8 entries receives
    2 500 atomic adds per feature"""
    if kind == "cluster":
        u = torch.rand(2500, 3, generator=torch.Generator().manual_seed(31), dtype=torch.float64) * 0.9 + 0.05
        x = (torch.tensor(CLUSTER_CELL, dtype=torch.float64) + u - 0.5) / 15.0
        return ((x + 1) / 2 * (VMAX - VMIN) + VMIN).to(torch.float32)
    n = int(kind)
    return _positions(n, 100 + n)


def cotangents(n, c):
    return tuple(t * np.float32(c) for t in _cotangents(n, 200 + n))


def encode_positions(n=3000):
    """test_ngp.py's bit-exact encoding input: uniform in the box, the first two points at box corners (x = -1 / +1 exactly)"""
    pos = torch.rand(n, 3, generator=torch.Generator().manual_seed(11)) * (VMAX - VMIN) + VMIN
    pos[0] = torch.tensor([VMIN, VMAX, 0.25]); pos[1] = torch.tensor([VMAX, VMIN, VMIN])
    return pos


def encoder_input(pos):
    p = (pos.to(torch.float32) - np.float32(VMIN)) / np.float32(float(VMAX) - float(VMIN))
    return p * np.float32(2.0) - np.float32(1.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the forward's uncertainty: what the f32 summation order can change
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Analysis:
    pass


def analyse(params, pos):
    """the oracle's forward values, the exact pre-activations (float64 over the half operands), their f32 summation bounds, the undecided masks, the steps
    dH1 / dH2 / ds by which an f32 evaluation in another order can differ, and the touched table entries in compact form"""
    a = Analysis()
    v = a.v = _forward_values(params, pos)
    a.n = pos.shape[0]
    X, H1, H2, W1, W2, W3 = (d(v[k]) for k in ("X", "H1", "H2", "W1", "W2", "W3"))
    relu = torch.relu
    ex1 = X @ W1.T
    b1 = 64 * F * (X.abs() @ W1.abs().T)
    lo, hi = h64(relu(ex1 - b1)), h64(relu(ex1 + b1))
    assert bool(((H1 >= lo) & (H1 <= hi)).all())
    a.dH1 = hi - lo
    a.und1 = (ex1.abs() <= b1) & (b1 > 0)
    ex2 = H1 @ W2.T
    b2 = 64 * F * ((H1 + a.dH1) @ W2.abs().T) + a.dH1 @ W2.abs().T
    lo, hi = h64(relu(ex2 - b2)), h64(relu(ex2 + b2))
    assert bool(((H2 >= lo) & (H2 <= hi)).all())
    a.dH2 = hi - lo
    a.und2 = (ex2.abs() <= b2) & (b2 > 0)
    W3a = W3[:5].abs()
    ex3 = H2 @ W3[:5].T
    b3 = 64 * F * ((H2 + a.dH2) @ W3a.T) + a.dH2 @ W3a.T
    sig = lambda o: 1.0 / (1.0 + torch.exp(-o))
    lo, hi = h64(sig(h64(ex3 - b3)) * (1 - 2.0 ** -21)), h64(sig(h64(ex3 + b3)) * (1 + 2.0 ** -21))      # 2^-21: exp and the division of the f32 sigmoid
    s = d(v["s"])
    assert bool(((s >= lo) & (s <= hi)).all())
    a.ds = hi - lo
    a.exact_masks = (ex1 > 0, ex2 > 0)
    out_half = (v["H2"].float() @ v["W3"].float().T)[:, :5].to(torch.float16)
    a.s_unrounded = d(torch.sigmoid(out_half.float()))
    corners = _corners(v["x"])
    entries, inv = torch.unique(torch.cat([idx.reshape(-1) for idx, _ in corners]), return_inverse=True)
    a.entries = entries                                                      # global entry indices, sorted
    a.corners = [(inv[l * a.n * 8:(l + 1) * a.n * 8].reshape(a.n, 8), d(wgt)) for l, (_, wgt) in enumerate(corners)]
    a.count = torch.zeros(entries.numel(), dtype=torch.float64).index_add_(0, inv, torch.ones(inv.numel(), dtype=torch.float64))
    return a


def undecided_share(a):
    return max(float(a.und1.double().mean()), float(a.und2.double().mean()))


def _scatter(a, per_point, swap=False):
    """sum over the 8 corners of w * per_point[:, 2 l : 2 l + 2] into the compact table (K, 2)"""
    tab = torch.zeros(a.entries.numel(), 2, dtype=torch.float64)
    for l, (idx, wgt) in enumerate(a.corners):
        for c in range(8):
            w = wgt[:, c ^ 1] if swap and c == 3 else wgt[:, c]
            tab.index_add_(0, idx[:, c], w[:, None] * per_point[:, 2 * l:2 * l + 2])
    return tab


def compact(a, dense):
    """a dense gradient (n_params) -> (the 9216 matrix entries, the touched table entries (K, 2)), float64"""
    return d(dense[:N_MLP]), d(dense[N_MLP:].reshape(-1, 2)[a.entries])


def reference_gradient(params, pos, cot, a):
    return compact(a, f64_gradient(params, pos, cot))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the documented backward with its roundings, and its mutants
# ---------------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("flush", "loss_scale_1", "truncate", "mask_ge", "sigmoid_unrounded", "corner_swap", "no_098")


def restated_gradient(a, cot, loss_scale=LOSS_SCALE, mutant=None):
    assert mutant is None or mutant in MUTANTS
    v = a.v
    rnd = trunc_h64 if mutant == "truncate" else h64
    op = flush if mutant == "flush" else (lambda t: t)
    ls = 1.0 if mutant == "loss_scale_1" else loss_scale
    s = a.s_unrounded if mutant == "sigmoid_unrounded" else d(v["s"])
    g_r = cot[1] if mutant == "no_098" else cot[1] * np.float32(0.98)
    g = torch.cat([d(cot[0]), d(g_r), d(cot[2])], dim=1)
    mask = (lambda p: d(p >= 0)) if mutant == "mask_ge" else (lambda p: d(p > 0))
    X, H1, H2, W1, W2, W3 = (op(d(v[k])) for k in ("X", "H1", "H2", "W1", "W2", "W3"))
    dz3 = torch.zeros(a.n, 16, dtype=torch.float64)
    dz3[:, :5] = rnd(g * (s * (1 - s)) * ls)
    dz3 = op(dz3)
    dW3 = dz3.T @ H2
    dz2 = op(rnd((dz3 @ W3) * mask(v["pre2"])))
    dW2 = dz2.T @ H1
    dz1 = op(rnd((dz2 @ W2) * mask(v["pre1"])))
    dW1 = dz1.T @ X
    dX = dz1 @ W1
    return torch.cat([dW1.reshape(-1), dW2.reshape(-1), dW3.reshape(-1)]) / ls, _scatter(a, dX, swap=mutant == "corner_swap") / ls


def _r(x):
    return torch.where(x > 0, torch.clamp(U * x, min=Q), torch.zeros_like(x))


def envelope(a, cot, loss_scale=LOSS_SCALE):
    """(tol of the 9216 matrix entries, tol of the touched table entries (K, 2)); see the module docstring"""
    v, n, ls = a.v, a.n, loss_scale
    X, H1, H2, W1, W2, W3 = (d(v[k]) for k in ("X", "H1", "H2", "W1", "W2", "W3"))
    s = d(v["s"])
    g = torch.cat([d(cot[0]), d(cot[1]) * 0.98, d(cot[2])], dim=1)
    dz3 = torch.zeros(n, 16, dtype=torch.float64); e3 = torch.zeros_like(dz3)
    dz3[:, :5] = g * s * (1 - s) * ls
    A3 = dz3.abs()
    e3[:, :5] = _r(A3[:, :5] * (1 + 4 * F)) + 4 * F * A3[:, :5] + g.abs() * ls * a.ds
    m2, m1 = d(v["pre2"] > 0), d(v["pre1"] > 0)

    def layer(dz, A, e, W, m, und, k):
        t, Araw = dz @ W, A @ W.abs()
        eh = e @ W.abs() + k * F * Araw
        inside = eh + _r(t.abs() + eh)
        return t * m, torch.where(und, Araw, Araw * m), torch.where(und, t.abs() + inside, inside * m)

    dz2, A2, e2 = layer(dz3, A3, e3, W3, m2, a.und2, 16)
    dz1, A1, e1 = layer(dz2, A2, e2, W2, m1, a.und1, 64)
    AX = A1 @ W1.abs()
    eX = e1 @ W1.abs() + 64 * F * AX
    k = (n + 4) * F
    tW3 = e3.T @ H2 + (A3 + e3).T @ a.dH2 + k * (A3.T @ H2)
    tW2 = e2.T @ H1 + (dz2.abs() + e2).T @ a.dH1 + k * (A2.T @ H1)
    tW1 = e1.T @ X.abs() + k * (A1.T @ X.abs())
    tab = _scatter(a, eX) + (a.count[:, None] + 4) * F * _scatter(a, AX)
    return torch.cat([tW1.reshape(-1), tW2.reshape(-1), tW3.reshape(-1)]) / ls, tab / ls


def class_slices():
    return {"dW1": slice(0, 4096), "dW2": slice(4096, 8192), "dW3": slice(8192, N_MLP)}


def ratios(got, ref, tol):
    """{class: worst |got - ref| / tol}; an element with tol = 0 must be equal (otherwise inf)"""
    out = {}
    parts = [(k, got[0][sl], ref[0][sl], tol[0][sl]) for k, sl in class_slices().items()] + [("tables", got[1], ref[1], tol[1])]
    for k, x, r, t in parts:
        err = (d(x) - r).abs()
        q = torch.where(t > 0, err / torch.where(t > 0, t, torch.ones_like(t)), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        out[k] = float(q.max()) if q.numel() else 0.0
    return out


def block_l2(a, got, ref):
    """worst relative L2 over test_ngp_backward's blocks (dW1, dW2, dW3[0:5], the 32 level tables), on the compact representation"""
    worst = 0.0
    parts = []
    for _, sl in _blocks():
        if sl.stop <= N_MLP:
            parts.append((got[0][sl], ref[0][sl]))
        else:
            m = (a.entries >= (sl.start - N_MLP) // 2) & (a.entries < (sl.stop - N_MLP) // 2)
            parts.append((got[1][m], ref[1][m]))
    for x, r in parts:
        den = float(r.norm())
        if den > 0:
            worst = max(worst, float((d(x) - r).norm()) / den)
    return worst


CASES = [(p, str(n), c) for p in ("init", "uniform", "mixed") for c in SCALES for n in SIZES] + [("init", "cluster", 3e-5), ("saturated", "1", 1.0), ("saturated", "33", 1.0)]


@functools.lru_cache(maxsize=None)
def analysis_of(pname, kind):
    return analyse(parameters(pname), positions(kind))


@functools.lru_cache(maxsize=None)
def case(pname, kind, c):
    """(analysis, positions, cotangents, reference, restated, tol, E per class): computed once, shared, never modified; compact, so that all cases fit in memory"""
    a = analysis_of(pname, kind)
    pos = positions(kind)
    cot = cotangents(pos.shape[0], c)
    ref = reference_gradient(parameters(pname), pos, cot, a)
    res = restated_gradient(a, cot)
    tol = envelope(a, cot)
    return a, pos, cot, ref, res, tol, ratios(res, ref, tol)
