"""numpy float32 restatement of the fused Adam step (include/iris_hip.h, iris_amd/csrc/iris_optim.h): the scalars in Python double, each rounded to
float32 once; every per-element operation a separate float32 operation in the order the kernel writes it (numpy never contracts a multiply and an add)."""
import math

import numpy as np

f32 = np.float32


def adam_scalars(step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    return dict(w1=f32(1.0 - beta1), w2=f32(1.0 - beta2), beta2=f32(beta2), step_size=f32(lr / (1.0 - beta1 ** step)),
                bc2=f32(math.sqrt(1.0 - beta2 ** step)), eps=f32(eps), wd=f32(weight_decay))


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """-> (p', m', v') float32 arrays; step counts from 1; the inputs are left as they are"""
    s = adam_scalars(step, lr, beta1, beta2, eps, weight_decay)
    p, g, m, v = (np.asarray(a, dtype=f32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        if s["wd"] != 0:
            g = g + s["wd"] * p
        m = m + s["w1"] * (g - m)
        v = v * s["beta2"] + (s["w2"] * g) * g
        p = p - s["step_size"] * (m / (np.sqrt(v) / s["bc2"] + s["eps"]))
    assert p.dtype == f32 and m.dtype == f32 and v.dtype == f32
    return p, m, v


def problem(n, seed, n_steps):
    """(p0, [g_1 .. g_n_steps]): parameters at 1e-4 and 0.3 (alternating blocks), gradients of magnitude 1e-12 .. 1 with random signs, half of them
    exactly zero"""
    rng = np.random.default_rng(seed)
    scale = np.where(np.arange(n) % 2 == 0, 1e-4, 0.3)
    p0 = (rng.uniform(-1, 1, n) * scale).astype(f32)
    grads = []
    for _ in range(n_steps):
        g = 10.0 ** rng.uniform(-12, 0, n) * rng.choice([-1.0, 1.0], n)
        g[rng.permutation(n)[:n // 2]] = 0.0
        grads.append(g.astype(f32))
    return p0, grads


def run(p0, grads, lrs, weight_decay=0.0, **kw):
    """the restatement over len(grads) steps from zero state, step k at learning rate lrs[k] -> (p, m, v)"""
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for k, (g, lr) in enumerate(zip(grads, lrs)):
        p, m, v = adam_step(p, g, m, v, k + 1, lr, weight_decay=weight_decay, **kw)
    return p, m, v
