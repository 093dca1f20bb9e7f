"""Float64 torch-CPU restatement of csrc/frozen_predict.hip: the column algebra of the layer's eval branch from a CHAIN state
(L^-1, U, a -- formed here with torch), layer by layer as the kernel runs it, and the kernel's own backward formulas.

    layer 0 at x_t:                 k = k(Z, x_t);  A = L^-1 k;  C = U^T A;  mean = a^T A;  var = max(k_nn - |A|^2 + |C|^2, 1e-10)
    layer l >= 1 at column (t, s):  f = mean_{l-1} + sqrt(var_{l-1}) samples_l[s]  (layer 0's column t serves the S replicas)

``hyp`` is the packed vector of the C-ABI: kind 0 [alpha, ls (d)], kind 1 [a1, af, nu, a2, lsf, ls1 (d), ls2 (d)].
"""
import torch

MIN_VARIANCE = 1e-10


def kernel(hyp, kind, Z, X):
    """k(Z, X): (M, n).  Rows of kind 1 are [x, f]."""
    def rbf(a, b, ls):
        a, b = a / ls, b / ls
        return torch.exp(-0.5 * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    if kind == 0:
        return hyp[0] * rbf(Z, X, hyp[1:])
    d = Z.shape[1] - 1
    a1, af, nu, a2, lsf = hyp[0], hyp[1], hyp[2], hyp[3], hyp[4]
    ls1, ls2 = hyp[5:5 + d], hyp[5 + d:5 + 2 * d]
    zx, zf, xx, xf = Z[:, :d], Z[:, d], X[:, :d], X[:, d]
    ef = torch.exp(-0.5 * ((zf[:, None] - xf[None, :]) / lsf) ** 2)
    return a1 * rbf(zx, xx, ls1) * (nu * zf[:, None] * xf[None, :] + af * ef) + a2 * rbf(zx, xx, ls2)


def kernel_diag(hyp, kind, X):
    if kind == 0:
        return hyp[0] * torch.ones(X.shape[0], dtype=X.dtype)
    f = X[:, -1]
    return hyp[0] * (hyp[2] * f * f + hyp[1]) + hyp[3]


def chain_state(hyp, kind, Z, m, L_S, jitter):
    """What the layer's CHAIN half leaves: L^-1, U = L^-1 L_S, a = L^-1 m of K_mm + jitter I = L L^T."""
    M = Z.shape[0]
    L = torch.linalg.cholesky(kernel(hyp, kind, Z, Z) + jitter * torch.eye(M, dtype=Z.dtype))
    Linv = torch.linalg.solve_triangular(L, torch.eye(M, dtype=Z.dtype), upper=False)
    return dict(kind=kind, hyp=hyp, Z=Z, Linv=Linv, U=Linv @ torch.tril(L_S), a=Linv @ m)


def layer_columns(ch, X):
    """(mean, var, saved) of one layer at the rows X (n, d or d + 1)."""
    K = kernel(ch["hyp"], ch["kind"], ch["Z"], X)
    A = ch["Linv"] @ K
    C = ch["U"].T @ A
    raw = (kernel_diag(ch["hyp"], ch["kind"], X) - (A * A).sum(0)) + (C * C).sum(0)
    return ch["a"] @ A, raw.clamp_min(MIN_VARIANCE), dict(A=A, C=C, raw=raw)


def predict(chains, samples, X, S):
    """Top-layer (mean, var), T S columns (T for one layer), column t S + s; and per layer (rows, mean, var, saved)."""
    T = X.shape[0]
    mean, var, saved = layer_columns(chains[0], X)
    per_layer = [(X, mean, var, saved)]
    for l in range(1, len(chains)):
        if l == 1:
            mean, var = mean.repeat_interleave(S), var.repeat_interleave(S)
        f = mean + torch.sqrt(var) * samples[l].reshape(-1).repeat(T)
        rows = torch.cat([X.repeat_interleave(S, 0), f[:, None]], 1)
        mean, var, saved = layer_columns(chains[l], rows)
        per_layer.append((rows, mean, var, saved))
    return mean, var, per_layer


def input_gradient(chains, samples, X, S, g_mean, g_var):
    """d / dX of <g_mean, top mean> + <g_var, top var> by autograd."""
    Xa = X.detach().clone().requires_grad_(True)
    mean, var, _ = predict(chains, samples, Xa, S)
    ((mean * g_mean).sum() + (var * g_var).sum()).backward()
    return Xa.grad


def input_gradient_by_the_kernels_formulas(chains, samples, X, S, g_mean, g_var):
    """The same, the way the kernel forms it: gv = g_var [raw > 1e-10]; dA = 2 U (C gv) + a g_mean - 2 A gv; dK = L^-T dA; the
    Gram backward w.r.t. the rows (autograd on k alone, and d k_nn / d f); the propagation backward g_mean_{l-1} = sum_s g_f,
    g_var_{l-1} = sum_s g_f eps / (2 sqrt(var_{l-1})); gx = the sum over the layers and the S columns of a base row."""
    T, d = X.shape
    with torch.no_grad():
        _, _, per_layer = predict(chains, samples, X, S)
    gx = torch.zeros_like(X)
    gm, gv = g_mean, g_var
    for l in range(len(chains) - 1, -1, -1):
        ch = chains[l]
        rows, _, var, sv = per_layer[l]
        gvr = torch.where(sv["raw"] > MIN_VARIANCE, gv, torch.zeros_like(gv))
        dA = 2.0 * ch["U"] @ (sv["C"] * gvr) + ch["a"][:, None] * gm[None, :] - 2.0 * sv["A"] * gvr
        dK = ch["Linv"].T @ dA
        R = rows.detach().clone().requires_grad_(True)
        ((kernel(ch["hyp"], ch["kind"], ch["Z"], R) * dK).sum() + (kernel_diag(ch["hyp"], ch["kind"], R) * gvr).sum()).backward()
        g_rows = R.grad
        gx = gx + (g_rows[:, :d].reshape(T, -1, d).sum(1) if l else g_rows)
        if l:
            g_f = g_rows[:, d]
            eps = samples[l].reshape(-1).repeat(T)
            var_prev = per_layer[l - 1][2]
            if l == 1:
                gm = g_f.reshape(T, S).sum(1)
                gv = (g_f * eps).reshape(T, S).sum(1) * 0.5 / torch.sqrt(var_prev)
            else:
                gm, gv = g_f, g_f * eps * 0.5 / torch.sqrt(var_prev)
    return gx
