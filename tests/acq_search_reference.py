"""Float64 torch restatements of the three kernels of csrc/acq_search.hip (mobocmf_jes_group_forward,
mobocmf_ascent_adam_step, mobocmf_select_topk) as include/mobocmf_hip.h states them: what tests/test_hip_acq_search.py compares
the GPU against and tests/test_acq_search_cpu.py pins to torch.autograd, torch.optim.Adam and torch.topk."""
import math

import torch


def model_v(moments, noise, T, S):
    """(v (n, T), mbar (n, T)) of every model from raw moments (n, 2, T S): TinyPredictGroup.acquisition_moments."""
    n = moments.shape[0]
    mu = moments[:, 0].reshape(n, T, S)
    var = moments[:, 1].reshape(n, T, S) + noise.reshape(n, 1, 1)
    if S == 1:
        return var[:, :, 0], mu[:, :, 0]
    mbar = mu.sum(2) / S
    return (var + mu * mu).sum(2) / S - mbar * mbar, mbar


def jes_group_forward(moments, noise, T, S, want_seeds=True):
    """(acq (T,), seeds like moments or None, log terms (T,): sum_p |log v_u| + |log v_c|, the scale of acq's rounding)."""
    n = moments.shape[0]
    v, mbar = model_v(moments, noise, T, S)
    lu, lc = torch.log(v[0::2]), torch.log(v[1::2])
    diff = lu - lc
    acq = torch.zeros(T, dtype=moments.dtype)
    for p in range(n // 2):      # summed in pair order
        acq = acq + 0.5 * torch.clamp(diff[p], min=0.0)
    scale = (lu.abs() + lc.abs()).sum(0)
    if not want_seeds:
        return acq, None, scale
    passes = diff >= 0.0
    gv = torch.zeros_like(v)
    gv[0::2] = torch.where(passes, 0.5 / v[0::2], torch.zeros_like(diff))
    gv[1::2] = torch.where(passes, -0.5 / v[1::2], torch.zeros_like(diff))
    mu = moments[:, 0].reshape(n, T, S)
    seeds = torch.zeros_like(moments)
    seeds[:, 0] = (gv[:, :, None] * (2.0 * (mu - mbar[:, :, None]) / S)).reshape(n, T * S)
    seeds[:, 1] = (gv[:, :, None] * (1.0 / S)).expand(n, T, S).reshape(n, T * S)
    return acq, seeds, scale


def track_best(acq, x, best_v, best_x):
    """The tracking of mobocmf_jes_group_forward: strict, a NaN never wins.  Returns new (best_v, best_x)."""
    better = acq > best_v
    return torch.where(better, acq, best_v), torch.where(better[:, None], x, best_x)


def ascent_adam_step(x, gx, lo, hi, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """One step (``step``: 1-based): returns new (x, m, v).  g = -(gx[0] + gx[1] + ...), torch.optim.Adam's update, the clamp."""
    s = gx[0].clone()
    for k in range(1, gx.shape[0]):
        s = s + gx[k]
    g = -s
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    x = x - (lr / bc1) * m / (v.sqrt() / bc2s + eps)
    return torch.minimum(torch.maximum(x, lo), hi), m, v


def select_topk(vals, k, x=None):
    """(values, indices, rows or None): descending, ties to the lower index, NaN after every number."""
    v = vals.tolist()
    order = sorted(range(len(v)), key=lambda i: (v[i] != v[i], 0.0 if v[i] != v[i] else -v[i], i))[:k]
    idx = torch.tensor(order, dtype=torch.int64)
    return vals[idx], idx, None if x is None else x[idx]
