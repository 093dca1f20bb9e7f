"""CPU restatement (float64 torch) of the natural-gradient update of q(u) = N(m, L_S L_S^T) that mobocmf_natgrad_step
performs ("Natural gradients"), the gamma schedule in exact arithmetic, and the closed-form optimum of the conjugate
one-layer problem the tests pin both against."""
from decimal import Decimal, getcontext

import torch


def gamma_at(t, gamma, gamma_init, warmup_steps):
    """gamma_t = min(gamma, gamma_init rho^t), rho = (gamma / gamma_init)^(1 / warmup_steps), to 40 digits (the float64 power
    rho ** t carries t roundings of rho: not a reference at 1e-14)."""
    if warmup_steps <= 0 or t >= warmup_steps:
        return float(gamma)
    getcontext().prec = 40
    g, g0 = Decimal(repr(float(gamma))), Decimal(repr(float(gamma_init)))
    val = g0 * ((g / g0).ln() * Decimal(t) / Decimal(warmup_steps)).exp()
    return float(min(g, val))


def psi_of(L_S, g_LS):
    """Psi = sym(Phi(L_S^T g_LS)): G_S = dloss/dS = L_S^-T Psi L_S^-1 (Phi: lower triangle, halved diagonal)."""
    L = torch.tril(L_S)
    P = torch.tril(L.T @ torch.tril(g_LS))
    Phi = P - 0.5 * torch.diag(torch.diagonal(P))
    return 0.5 * (Phi + Phi.T)


def natgrad_update(m, L_S, g_m, g_LS, gamma, scale=1.0):
    """One step: returns (m_new, L_new, B, ok).  L_new is lower triangular with the diagonal signs of L_S; when B = I + 2 gamma
    scale Psi is not positive definite ok is False and (m, tril(L_S)) come back unchanged."""
    M = m.numel()
    L = torch.tril(L_S)
    B = torch.eye(M, dtype=m.dtype) + 2.0 * gamma * scale * psi_of(L_S, g_LS)
    J = torch.flip(torch.eye(M, dtype=m.dtype), [0])
    C, info = torch.linalg.cholesky_ex(J @ B @ J)
    if int(info) != 0:
        return m.clone(), L, B, False
    Cinv = torch.linalg.solve_triangular(C, torch.eye(M, dtype=m.dtype), upper=False)
    T = J @ Cinv.T @ J                      # lower triangular, T T^T = B^-1
    L_new = torch.tril(L @ T)
    m_new = m - gamma * scale * (L_new @ (L_new.T @ g_m))
    return m_new, L_new, B, True


def conjugate_optimum(Kmm, Kmn, y, noise):
    """S* = (K^-1 + K^-1 K_mn K_nm K^-1 / noise)^-1,  m* = S* K^-1 K_mn y / noise  (Titsias' optimal q(u), unwhitened)."""
    Ki = torch.linalg.inv(Kmm)
    A = Ki @ Kmn
    Lam = Ki + A @ A.T / noise
    S = torch.linalg.inv(Lam)
    S = 0.5 * (S + S.T)
    return S @ (A @ y) / noise, S, Lam


def conjugate_neg_elbo(m, L_S, Kmm, Kmn, knn, y, noise):
    """-ELBO of the one-layer sparse GP with Gaussian noise (unwhitened q(u), zero prior mean), differentiable in m, L_S."""
    L = torch.tril(L_S)
    S = L @ L.T
    Ki = torch.linalg.inv(Kmm)
    A = Ki @ Kmn
    mu = A.T @ m
    var = knn - (Kmn * A).sum(0) + (A * (S @ A)).sum(0)
    ll = (-0.5 * torch.log(2 * torch.pi * noise) - 0.5 * ((y - mu) ** 2 + var) / noise).sum()
    M = m.numel()
    kl = 0.5 * ((Ki * S).sum() + m @ Ki @ m - M + torch.logdet(Kmm) - 2.0 * torch.log(torch.abs(torch.diagonal(L))).sum())
    return -(ll - kl)


def conjugate_problem(M=12, N=40, d=2, seed=0):
    """A small conjugate problem: squared-exponential K, random inputs; returns (Kmm + 1e-6 I, Kmn, knn, y, noise)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, d, dtype=torch.float64, generator=g)
    z = torch.rand(M, d, dtype=torch.float64, generator=g)
    y = torch.sin(3.0 * x.sum(1)) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    k = lambda a, b: 1.3 * torch.exp(-0.5 * torch.cdist(a, b) ** 2 / 0.4 ** 2)
    return k(z, z) + 1e-6 * torch.eye(M, dtype=torch.float64), k(z, x), torch.full((N,), 1.3, dtype=torch.float64), y, \
        torch.tensor(0.05, dtype=torch.float64)
