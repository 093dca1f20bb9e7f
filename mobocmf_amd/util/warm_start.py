"""Warm-start refits (``MFDGP(..., previously_trained_model=prev, warm_start="posterior")``): q(u) of a fitted model carried
over to a model with more inducing inputs, exactly.

With new inducing inputs Z* next to the old ones Z, q_new(u, u*) = q_old(u) p(u* | u) leaves the layer's predictive distribution
at every input and its KL term unchanged -- for the unwhitened parameterisation, with the jitter (p is the prior the layer itself
uses, N(0, k + jitter I)), and through the deep chain Z~_l = [Z_x, m_{l-1}], because the extended mean of layer l - 1 at the new
rows is what layer l gets as the f column of its new inducing inputs.

Everything here is float64 host algebra on plain tensors, O(M^2 n) once per refit, next to the constructor's other set-up
algebra (``gp.gram_cpu_init``); nothing here needs the native library.
"""
import torch

from ..gp import gram_cpu as gram
from ..layers.mfdgp_hidden_layer import NotPSDError

# The carried-over likelihood noise is clipped to [lo + NOISE_MARGIN_LOW w, hi - NOISE_MARGIN_HIGH w], w = hi - lo the width of
# the NEW model's interval.  Its lower bound is the same in every model, so the lower margin only keeps the inverse transform
# finite for a noise that sits on the bound (raw >= -27.6).  The upper bound is 0.1 std(y) of the new data: a previous noise
# above it is clipped to a point where the sigmoid still has a slope of 1e-3 of its width, so that training can move it.
NOISE_MARGIN_LOW, NOISE_MARGIN_HIGH = 1e-12, 1e-3


def extend_qu(hyp, kind, Z_old, Z_new, m, L_S, jitter):
    """q(u) = N(m, L_S L_S^T) at the M inducing inputs ``Z_old`` extended by the n inputs ``Z_new``:

        K~  = k(Z, Z) + jitter I
        A   = K~^-1 k(Z, Z*)                                   (M x n)
        C   = k(Z*, Z*) + jitter I - k(Z*, Z) A                (n x n, symmetrised)
        m'  = [m; A^T m]        L_S' = [[tril(L_S), 0], [A^T tril(L_S), chol(C)]]

    Returns (m' (M + n,), L_S' (M + n, M + n), A), float64; the old rows of m and L_S are copied bitwise (L_S as stored, its
    upper triangle included).  n = 0 is a pure copy.  Raises NotPSDError when K~ or C is not positive definite."""
    Z_old, Z_new = Z_old.detach().double().cpu(), Z_new.detach().double().cpu()
    m, L_S = m.detach().double().cpu().reshape(-1), L_S.detach().double().cpu()
    M, n = Z_old.shape[0], Z_new.shape[0]
    if m.shape[0] != M or tuple(L_S.shape) != (M, M) or (n and Z_new.shape[1] != Z_old.shape[1]):
        raise ValueError("extend_qu: q(u) has %d means and a %s factor for %d inducing inputs of %d columns (new ones: %d)"
                         % (m.shape[0], tuple(L_S.shape), M, Z_old.shape[1], Z_new.shape[1] if n else Z_old.shape[1]))
    if n == 0:
        return m.clone(), L_S.clone(), torch.zeros(M, 0, dtype=torch.float64)
    K = gram(hyp, kind, Z_old, Z_old) + jitter * torch.eye(M, dtype=torch.float64)
    Lk, info = torch.linalg.cholesky_ex(K)
    if int(info) != 0:
        raise NotPSDError("warm start: the previous layer's K_mm + %.1e I is not positive definite (pivot %d)"
                          % (jitter, int(info)))
    Kzs = gram(hyp, kind, Z_old, Z_new)
    A = torch.cholesky_solve(Kzs, Lk)
    C = gram(hyp, kind, Z_new, Z_new) + jitter * torch.eye(n, dtype=torch.float64) - Kzs.T @ A
    C = 0.5 * (C + C.T)
    Lc, info = torch.linalg.cholesky_ex(C)
    if int(info) != 0:
        raise NotPSDError("warm start: the prior covariance of the %d new inducing values given the old ones is not positive "
                          "definite (pivot %d, jitter %.1e)" % (n, int(info), jitter))
    m_new = torch.cat([m, A.T @ m])
    L_new = torch.zeros(M + n, M + n, dtype=torch.float64)
    L_new[:M, :M] = L_S
    L_new[M:, :M] = A.T @ torch.tril(L_S)
    L_new[M:, M:] = Lc
    return m_new, L_new, A


def check_inducing_rule(Zx_old, Zx_new, selection="first"):
    """The inducing-input rule of ``warm_start="posterior"``: the new model's Z_x begins with the previous model's, row for row
    and bitwise in float64; every row after that is new.  Anything else is a ValueError naming the first differing row."""
    Zx_old, Zx_new = Zx_old.detach().double().cpu(), Zx_new.detach().double().cpu()
    how = " (inducing_selection='greedy_variance' picked them: this selection does not extend the previous one)" \
        if selection == "greedy_variance" else ""
    if Zx_new.shape[1] != Zx_old.shape[1]:
        raise ValueError("warm_start='posterior': the previous model has %d input dimensions, the new one %d"
                         % (Zx_old.shape[1], Zx_new.shape[1]))
    if Zx_new.shape[0] < Zx_old.shape[0]:
        raise ValueError("warm_start='posterior': the new model has %d inducing inputs, fewer than the previous model's %d%s"
                         % (Zx_new.shape[0], Zx_old.shape[0], how))
    differs = (Zx_new[:Zx_old.shape[0]] != Zx_old).any(1)
    if bool(differs.any()):
        raise ValueError("warm_start='posterior': the new inducing inputs must begin with the previous model's, row for row; "
                         "row %d differs%s" % (int(torch.nonzero(differs)[0]), how))


def clip_noise(noise, lower_bound, upper_bound):
    """``noise`` strictly inside (lower_bound, upper_bound), the margins above."""
    w = upper_bound - lower_bound
    return min(max(float(noise), lower_bound + NOISE_MARGIN_LOW * w), upper_bound - NOISE_MARGIN_HIGH * w)
