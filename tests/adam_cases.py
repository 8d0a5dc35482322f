"""Shared by tests/test_adam.py and tests/test_gpu_adam.py: the inputs of the 30-step trajectories and a
plain numpy restatement of the update rule of include/nr_raster.h (nothing shared with the package)."""
import numpy as np

N, STEPS = 5000, 30
LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-8


def gradients(rs, shape, zero_share, lo=-4., hi=2.):
    """Magnitudes over 10^[lo, hi], random signs, and a share of exact zeros."""
    g = 10. ** rs.uniform(lo, hi, shape) * rs.choice([-1., 1.], shape)
    g[rs.uniform(size=shape) < zero_share] = 0.
    return g


def inputs(seed=0):
    """p0 [N] of order 1 and grads [STEPS, N] with magnitudes over 10^[-4, 2] and 30 % exact zeros (float64)."""
    rs = np.random.RandomState(seed)
    return rs.uniform(-1, 1, N), gradients(rs, (STEPS, N), 0.3)


def np_factors(t, lr, scale, beta1, beta2):
    """(step_size, inv_sqrt_bc2) of step t in double."""
    return lr * scale / (1 - beta1 ** t), 1 / np.sqrt(1 - beta2 ** t)


def np_rule(p, m, v, g, step_size, inv_sqrt_bc2, beta1, beta2, eps, skip):
    """One step of the rule in the dtype of p (float64, or float32 with every operation rounded to
    float32, in the order the header gives); step_size and inv_sqrt_bc2 are taken as given.  Returns
    the new (p, m, v)."""
    ft = p.dtype.type
    c1, c2, eps, ss, isb = ft(1 - beta1), ft(1 - beta2), ft(eps), ft(step_size), ft(inv_sqrt_bc2)
    with np.errstate(all="ignore"):
        m2 = m + c1 * (g - m)
        v2 = v + c2 * (g * g - v)
        v2 = np.where(v2 < 0, ft(0), v2)
        p2 = p - ss * (m2 / (np.sqrt(v2) * isb + eps))
    if skip:
        zero = g == 0
        p2, m2, v2 = np.where(zero, p, p2), np.where(zero, m, m2), np.where(zero, v, v2)
    assert p2.dtype == m2.dtype == v2.dtype == p.dtype
    return p2, m2, v2


def np_trajectory(p0, grads, lr=LR, scale=1., beta1=BETA1, beta2=BETA2, eps=EPS, skip=False):
    """The float64 trajectory: p after every step [STEPS, N], and the final m and v."""
    p, m, v = np.asarray(p0, np.float64), np.zeros(len(p0)), np.zeros(len(p0))
    out = []
    for t, g in enumerate(np.asarray(grads, np.float64), 1):
        ss, isb = np_factors(t, lr, scale, beta1, beta2)
        p, m, v = np_rule(p, m, v, g, ss, isb, beta1, beta2, eps, skip)
        out.append(p)
    return np.stack(out), m, v
