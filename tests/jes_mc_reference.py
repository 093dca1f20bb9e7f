"""Float64 torch restatement of mobocmf_jes_mc_group_forward (csrc/acq_search.hip) as include/mobocmf_hip.h states it: JES
averaged over K sampled Pareto sets, black-box p owning the models p (1 + K) (unconditioned) and p (1 + K) + 1 + k (conditioned
on sample k).  What tests/test_hip_jes_mc.py compares the GPU against and tests/test_jes_mc_cpu.py pins to torch.autograd and to
the single-sample restatement (tests/acq_search_reference.py)."""
import torch

from tests.acq_search_reference import model_v


def passing(moments, noise, K, T, S):
    """(n_boxes, K, T) bool: where log v_u,p - log v_c,pk >= 0 (the clamp passes the gradient)."""
    v, _ = model_v(moments, noise, T, S)
    lv = torch.log(v)
    return torch.stack([lv[0::1 + K] - lv[k::1 + K] >= 0.0 for k in range(1, K + 1)], 1)


def jes_mc_group_forward(moments, noise, K, T, S, want_seeds=True):
    """(acq (T,), seeds like moments or None, scale (T,): sum_p |log v_u| + (1/K) sum_k |log v_c,k|, the size of what acq's
    roundings are relative to).  The k-sum in the order of k, times 1/K, then the sum over p in the order of p."""
    n, stride = moments.shape[0], 1 + K
    n_boxes = n // stride
    assert K >= 1 and n == n_boxes * stride
    v, mbar = model_v(moments, noise, T, S)
    lv = torch.log(v)
    inv_k = 1.0 / K
    acq = torch.zeros(T, dtype=moments.dtype)
    scale = torch.zeros(T, dtype=moments.dtype)
    gv = torch.zeros_like(v)
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
        acq = acq + inv_k * box
        gv[u] = torch.where(cnt > 0, cnt * (0.5 / (K * v[u])), torch.zeros_like(cnt))
        scale = scale + lv[u].abs() + inv_k * labs
    if not want_seeds:
        return acq, None, scale
    mu = moments[:, 0].reshape(n, T, S)
    seeds = torch.zeros_like(moments)
    seeds[:, 0] = (gv[:, :, None] * (2.0 * (mu - mbar[:, :, None]) / S)).reshape(n, T * S)
    seeds[:, 1] = (gv[:, :, None] * (1.0 / S)).expand(n, T, S).reshape(n, T * S)
    return acq, seeds, scale


def jes_mc_value(moments, noise, K, T, S):
    """The same value as one differentiable expression of ``moments`` (what torch.autograd differentiates)."""
    v, _ = model_v(moments, noise, T, S)
    lv = torch.log(v)
    acq = 0.0
    for p in range(moments.shape[0] // (1 + K)):
        u = p * (1 + K)
        box = sum(0.5 * torch.clamp(lv[u] - lv[u + k], min=0.0) for k in range(1, K + 1))
        acq = acq + (1.0 / K) * box
    return acq


def mc_inputs(n_boxes, K, T, S, seed, flip):
    """Inputs in the manner of tests/test_hip_acq_search.py ``_jes_inputs``: means ~ N(0, 1), variances ~ U(0.05, 2), noise ~
    U(1e-3, 0.1); the model of black-box p conditioned on sample k is rescaled at test point t so that v_c is about 2 v_u where
    (p + b k + t + flip) is even (clamped: zero seeds) and about v_u / 2 elsewhere, b = bit 1 of (t + flip).  Where b = 1 the
    parity alternates with k (0 < #passing < K for K >= 2); where b = 0 it does not depend on k, so all K samples pass or none
    does, alternating with t: a parity of (p + k + t + flip) alone would make every test point a mixed one.  flip = 0 .. 3 visits
    every case also at T = 1."""
    g = torch.Generator().manual_seed(seed)
    stride = 1 + K
    n = n_boxes * stride
    mom = torch.empty(n, 2, T * S, dtype=torch.float64)
    mom[:, 0] = torch.randn(n, T * S, dtype=torch.float64, generator=g)
    mom[:, 1] = 0.05 + 1.95 * torch.rand(n, T * S, dtype=torch.float64, generator=g)
    noise = 1e-3 + 0.099 * torch.rand(n, dtype=torch.float64, generator=g)
    v, _ = model_v(mom, noise, T, S)
    two, half = torch.tensor(2.0, dtype=torch.float64), torch.tensor(0.5, dtype=torch.float64)
    for p in range(n_boxes):
        vu = v[p * stride]
        for k in range(K):
            i = p * stride + 1 + k
            vc, tc = v[i], noise[i]
            t = torch.arange(T)
            b = ((t + flip) >> 1) & 1
            r = torch.where((p + b * k + t + flip) % 2 == 0, two, half)
            c2 = torch.maximum(r * vu - tc, 0.01 * vu) / (vc - tc)       # v_c -> c2 (v_c - tau_c) + tau_c
            c2 = c2[:, None].expand(T, S).reshape(T * S)
            mom[i, 0] *= c2.sqrt()
            mom[i, 1] *= c2
    return mom, noise
