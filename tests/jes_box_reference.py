"""Float64 torch restatement of mobocmf_jes_mc_box_forward (csrc/acq_search.hip) as include/mobocmf_hip.h states it: JES per
black-box, term_p[t] = (1/K) sum_k 0.5 max(log v_u,p - log v_c,pk, 0), in its two modes (all boxes; the box each test point
names).  What tests/test_hip_jes_box.py compares the GPU against and tests/test_jes_box_cpu.py pins to torch.autograd and to
the coupled restatement (tests/jes_mc_reference.py)."""
import math

import torch

from tests.acq_search_reference import model_v


def box_terms(moments, noise, K, T, S):
    """(terms (n_boxes, T), gv (n, T): d term_p / d v of the models of box p, scale (n_boxes, T): |log v_u| + (1/K) sum_k
    |log v_c,k|, v, mbar).  The k-sum in the order of k, then the rounded product with 1/K."""
    n, stride = moments.shape[0], 1 + K
    n_boxes = n // stride
    assert K >= 1 and n == n_boxes * stride
    v, mbar = model_v(moments, noise, T, S)
    lv = torch.log(v)
    inv_k = 1.0 / K
    terms, scale, gv = [], [], torch.zeros_like(v)
    for p in range(n_boxes):
        u = p * stride
        box, cnt, labs = None, torch.zeros(T, dtype=moments.dtype), torch.zeros(T, dtype=moments.dtype)
        for k in range(1, K + 1):
            diff = lv[u] - lv[u + k]
            term = 0.5 * torch.clamp(diff, min=0.0)
            box = term if box is None else box + term
            passes = diff >= 0.0
            cnt = cnt + passes.to(moments.dtype)
            gv[u + k] = torch.where(passes, -0.5 / (K * v[u + k]), torch.zeros_like(diff))
            labs = labs + lv[u + k].abs()
        terms.append(inv_k * box)
        gv[u] = torch.where(cnt > 0, cnt * (0.5 / (K * v[u])), torch.zeros_like(cnt))
        scale.append(lv[u].abs() + inv_k * labs)
    return torch.stack(terms), gv, torch.stack(scale), v, mbar


def jes_mc_box_all(moments, noise, K, T, S):
    """The all-box mode: (acq (n_boxes, T), scale (n_boxes, T))."""
    terms, _, scale, _, _ = box_terms(moments, noise, K, T, S)
    return terms, scale


def jes_mc_box_selected(moments, noise, K, T, S, box_of_point, want_seeds=True):
    """The selected-box mode: (acq (T,), seeds like moments or None, scale (T,)).  A word outside [0, n_boxes): NaN, zero seeds
    (scale 0 there)."""
    n, stride = moments.shape[0], 1 + K
    n_boxes = n // stride
    terms, gv, scale, _, mbar = box_terms(moments, noise, K, T, S)
    b = box_of_point.to(torch.int64)
    ok = (b >= 0) & (b < n_boxes)
    bc = torch.where(ok, b, torch.zeros_like(b))
    t = torch.arange(T)
    acq = torch.where(ok, terms[bc, t], torch.full((T,), math.nan, dtype=moments.dtype))
    sc = torch.where(ok, scale[bc, t], torch.zeros(T, dtype=moments.dtype))
    if not want_seeds:
        return acq, None, sc
    own = (torch.arange(n)[:, None] // stride == b[None, :]) & ok[None, :]      # (n, T): model m belongs to the box of t
    own3 = own[:, :, None].expand(n, T, S).reshape(n, T * S)
    mu = moments[:, 0].reshape(n, T, S)
    zero = torch.zeros(n, T * S, dtype=moments.dtype)
    seeds = torch.zeros_like(moments)
    seeds[:, 0] = torch.where(own3, (gv[:, :, None] * (2.0 * (mu - mbar[:, :, None]) / S)).reshape(n, T * S), zero)
    seeds[:, 1] = torch.where(own3, (gv[:, :, None] * (1.0 / S)).expand(n, T, S).reshape(n, T * S), zero)
    return acq, seeds, sc


def jes_box_value(moments, noise, K, T, S, box_of_point):
    """term_b[t], b = box_of_point[t] (all in range), as one differentiable expression of ``moments``."""
    v, _ = model_v(moments, noise, T, S)
    lv = torch.log(v)
    t = torch.arange(T)
    rows = []
    for p in range(moments.shape[0] // (1 + K)):
        u = p * (1 + K)
        rows.append((1.0 / K) * sum(0.5 * torch.clamp(lv[u] - lv[u + k], min=0.0) for k in range(1, K + 1)))
    return torch.stack(rows)[box_of_point.to(torch.int64), t]


def box_patterns(n_boxes, T):
    """The two assignments of test points to boxes the tests use: interleaved, and in blocks (the engine's layout)."""
    t = torch.arange(T, dtype=torch.int32)
    return {"interleaved": t % n_boxes, "blocks": t // int(math.ceil(T / n_boxes))}
