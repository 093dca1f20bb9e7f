"""Reference of the exact-GP device fit (mobocmf_exact_fit_*, util/exact_fit.py): a numpy restatement, in longdouble, of the
sums of include/mobocmf_hip.h, of the chain rule to the raw parameters and of the update rule.  CPU only; the GPU tests
(test_hip_exact_fit.py) and the CPU proofs (test_exact_fit_cpu.py) share it.

With alpha and K^-1 GIVEN, G = (alpha alpha^T - K^-1) / 2 and value k of the 83 (os_s, ls_s[32], os_n, ls_n[32], tau, sig[8],
ntab[8]):
    S_k = sum_ij G_ij dK_ij / dvalue_k,      R_k = sum_ij (|alpha_i alpha_j| + |K^-1_ij|) / 2 |dK_ij / dvalue_k|
Gate of the gradient launch:  |got - S_k| <= (n^2 + C_T) u R_k.  n^2 bounds the error of summing n^2 terms in ANY order; C_T is
the allowance for the rounding of one term (G_ij: a product, a difference, a halving; dK_ij / dvalue: 2 d + 6 operations and an
exponential whose argument's error is amplified by |arg|; the closing factors os / ls^3), MEASURED as GRAM_C and
EXACT_PREDICT_RATIO_MEASURED were: EXACT_FIT_TERM_RATIO_MEASURED is the worst |term_f64 - term| / (u (|alpha_i alpha_j| +
|K^-1_ij|) / 2 |dK_ij / dvalue|) of the float64 restatement of a single term against the longdouble one over CASES
(test_exact_fit_cpu.py measures and pins it), and C_T = 4 x that: the device divides by the lengthscales where the restatement
does, but fuses and orders otherwise, each worth a few u |arg|; the margin covers inputs not sampled.
The device's own worst ratio over CASES, |got - S_k| / (u R_k) against the bound's n^2 + C_T (printed by
test_hip_exact_fit.py on the MI355X): see EXACT_FIT_DEVICE_RATIO_MEASURED below.
"""
import copy

import numpy as np
import torch

from tests.kernel_reference import U, ld, _ratio      # noqa: F401  (re-exported for the tests)

# (class, n, d, nf): one row; below one tile; the only small nf at which the rho^2 loop of ntab is live; across the 128 padding;
# the level limit (the loop runs k = 3 .. 6); both size limits
CASES = (("MFGP", 1, 1, 2), ("MFGP", 14, 2, 2), ("MFGP_lin", 40, 1, 5), ("MFGP_lin", 130, 3, 3), ("MFGP_lin", 257, 8, 8),
         ("MFGP", 512, 32, 2))
EXACT_FIT_TERM_RATIO_MEASURED = 54.0      # worst single-term ratio of the float64 restatement over CASES: 53.2 at (MFGP_lin, 40, 1, 5)
EXACT_FIT_CT = 4.0 * EXACT_FIT_TERM_RATIO_MEASURED
# worst |got - S_k| / (u R_k) of the device over CASES, per case in the order above (MI355X); the bound is n^2 + C_T
EXACT_FIT_DEVICE_RATIO_MEASURED = (0.31, 0.49, 0.40, 0.99, 0.96, 2.35)

D_MAX, L_MAX, SUMS = 32, 8, 83
S_OS_S, S_LS_S, S_OS_N, S_LS_N, S_TAU, S_SIG, S_NTAB = 0, 1, 33, 34, 66, 67, 75
SLOTS = ("noise", "os_s", "ls_s", "os_n", "ls_n", "rho")


def _data(n, d, nf, seed):
    """tests/test_hip_baselines.py's data: inputs uniform in [0, 1]^d, the levels cycling over the rows."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    fid = (np.arange(n) % nf).astype(float)
    y = np.sin(3 * x.sum(1)) + 0.3 * fid * np.cos(2 * x[:, 0]) + 0.05 * rng.standard_normal(n)
    return torch.as_tensor(np.concatenate([x, fid[:, None]], 1)), torch.as_tensor(y)[:, None]


_models = {}


def make_model(cls_name, n, d, nf):
    """A CPU model of a case with off-default hyper-parameters (every factor of the kernels takes part); a fresh deep copy of a
    cached original at every call."""
    key = (cls_name, n, d, nf)
    if key not in _models:
        from mobocmf_amd.models.mfgp import MFGP, MFGP_lin
        cls = MFGP if cls_name == "MFGP" else MFGP_lin
        X, Y = _data(n, d, nf, seed=n + d)
        m = cls(X, Y, nf)
        with torch.no_grad():
            cm = m.covar_module
            ls = cm.cov_funct_signal.base_kernel.lengthscale.reshape(-1)
            if not bool(torch.isfinite(ls).all()) or float(ls.min()) <= 0.0:      # (n = 1: no pair of rows, no median distance)
                ls = torch.ones_like(ls)
            ramp = torch.linspace(0.8, 1.3, d, dtype=torch.float64)      # a different lengthscale per coordinate
            cm.cov_funct_signal.base_kernel.lengthscale = ls * ramp
            cm.cov_funct_noise.base_kernel.lengthscale = 0.7 * ls * ramp.flip(0)
            cm.cov_funct_signal.outputscale = 0.8
            cm.cov_funct_noise.outputscale = 0.35
            m.likelihood.noise = 0.02
            if cls is MFGP_lin:
                cm.rho.copy_(torch.linspace(0.6, 1.4, nf - 1))
        _models[key] = m
    return copy.deepcopy(_models[key])


def slots_of(model):
    """[(raw parameter or None, constraint or None)] in the order of SLOTS."""
    cm, lk = model.covar_module, model.likelihood
    ks, kn = cm.cov_funct_signal, cm.cov_funct_noise
    return [(lk.raw_noise, lk.raw_noise_constraint), (ks.raw_outputscale, ks.raw_outputscale_constraint),
            (ks.base_kernel.raw_lengthscale, ks.base_kernel.raw_lengthscale_constraint),
            (kn.raw_outputscale, kn.raw_outputscale_constraint),
            (kn.base_kernel.raw_lengthscale, kn.base_kernel.raw_lengthscale_constraint),
            (getattr(cm, "rho", None), None)]


def param_names(model):
    """{slot: the parameter's name in named_parameters()}."""
    by_id = {id(p): k for k, p in model.named_parameters()}
    return {s: by_id[id(p)] for s, (p, _) in zip(SLOTS, slots_of(model)) if p is not None}


def case_of(model):
    """The numbers of a live model (any device) as float64 numpy: x (n x d), lev, y, per slot the raw values and the constraint
    (kind 'id' / 'softplus' / 'sigmoid', lo, hi)."""
    from mobocmf_amd import gp
    d = model.input_dim
    xt = model.x_train.detach().cpu()
    c = dict(n=xt.shape[0], d=d, nl=model.num_fidelities, lin=hasattr(model.covar_module, "rho"),
             x=xt[:, :d].numpy().copy(), lev=xt[:, d].round().to(torch.int64).numpy().copy(),
             y=model.y_train.detach().cpu().reshape(-1).numpy().copy(), raw={}, con={})
    for s, (p, k) in zip(SLOTS, slots_of(model)):
        if p is None:
            continue
        c["raw"][s] = p.detach().cpu().double().reshape(-1).numpy().copy()
        if k is None:
            c["con"][s] = ("id", 0.0, 0.0)
        elif type(k) is gp.Interval:
            c["con"][s] = ("sigmoid", k.lower_bound, k.upper_bound)
        else:
            c["con"][s] = ("softplus", getattr(k, "lower_bound", 0.0), 0.0)
    return c


def _transform(con, raw, dtype):
    kind, lo, hi = con
    r = np.asarray(raw, dtype)
    if kind == "softplus":
        return dtype(lo) + np.where(r > 20, r, np.log1p(np.exp(np.minimum(r, dtype(20)))))
    if kind == "sigmoid":
        return dtype(lo) + (dtype(hi) - dtype(lo)) / (1 + np.exp(-r))
    return r


def _slope(con, raw, dtype):
    kind, lo, hi = con
    r = np.asarray(raw, dtype)
    if kind == "softplus":
        z = np.exp(np.minimum(r, dtype(20)))
        return np.where(r > 20, dtype(1), z / (z + 1))
    if kind == "sigmoid":
        s = 1 / (1 + np.exp(-r))
        return (dtype(hi) - dtype(lo)) * s * (1 - s)
    return np.ones_like(r)


def values(c, dtype=np.longdouble):
    """The constrained values and the level tables: tau, os_s, ls_s, os_n, ls_n, rho, sig (nl), ntab (nl)."""
    v = {s: _transform(c["con"][s], c["raw"][s], dtype) for s in c["raw"]}
    nl = c["nl"]
    out = dict(tau=v["noise"][0], os_s=v["os_s"][0], ls_s=v["ls_s"], os_n=v["os_n"][0], ls_n=v["ls_n"])
    if c["lin"]:
        rho = v["rho"]
        sig = np.concatenate([np.ones(1, dtype), np.cumprod(rho)])
        ntab = np.zeros(nl, dtype)
        for t in range(nl):
            ntab[t] = dtype(1 if t >= 1 else 0) + sum((rho[k - 2] ** 2 for k in range(3, nl - 1) if t + 1 >= k), dtype(0))
        out.update(rho=rho, sig=sig, ntab=ntab)
    else:
        out.update(rho=np.zeros(0, dtype), sig=np.ones(nl, dtype), ntab=np.arange(nl).astype(dtype))
    return out


def _exps(c, v, dtype):
    diff = np.asarray(c["x"], dtype)[:, None, :] - np.asarray(c["x"], dtype)[None, :, :]
    half = dtype(0.5)
    Es = np.exp(-half * ((diff / v["ls_s"]) ** 2).sum(-1))
    En = np.exp(-half * ((diff / v["ls_n"]) ** 2).sum(-1))
    return diff, Es, En


def covariance(c, dtype=np.longdouble):
    """K with tau on the diagonal."""
    v = values(c, dtype)
    _, Es, En = _exps(c, v, dtype)
    lev = c["lev"]
    sg = v["sig"][lev]
    return sg[:, None] * sg[None, :] * v["os_s"] * Es + v["ntab"][np.minimum(lev[:, None], lev[None, :])] * v["os_n"] * En + \
        v["tau"] * np.eye(c["n"], dtype=dtype)


def terms(c, alpha, Kinv, dtype=np.longdouble):
    """Yields (k, T, W) per value k of the 83 that exists (coordinates < d, levels < nl): the n x n terms G_ij dK_ij / dvalue_k
    and the weights (|alpha_i alpha_j| + |K^-1_ij|) / 2 |dK_ij / dvalue_k|."""
    n, d, nl, lev = c["n"], c["d"], c["nl"], c["lev"]
    v = values(c, dtype)
    diff, Es, En = _exps(c, v, dtype)
    a, Ki = np.asarray(alpha, dtype)[:n], np.asarray(Kinv, dtype)[:n, :n]
    half = dtype(0.5)
    G = half * (a[:, None] * a[None, :] - Ki)
    Gabs = half * (np.abs(a[:, None] * a[None, :]) + np.abs(Ki))
    sg = v["sig"][lev]
    ss = sg[:, None] * sg[None, :]
    mn = np.minimum(lev[:, None], lev[None, :])
    nt = v["ntab"][mn]
    def dK():
        yield S_OS_S, ss * Es
        yield S_OS_N, nt * En
        yield S_TAU, np.eye(n, dtype=dtype)
        for k in range(d):
            yield S_LS_S + k, ss * v["os_s"] * Es * diff[:, :, k] ** 2 / v["ls_s"][k] ** 3
            yield S_LS_N + k, nt * v["os_n"] * En * diff[:, :, k] ** 2 / v["ls_n"][k] ** 3
        for l in range(nl):
            yield S_SIG + l, 2 * (lev == l).astype(dtype)[:, None] * sg[None, :] * v["os_s"] * Es
            yield S_NTAB + l, (mn == l).astype(dtype) * v["os_n"] * En

    for k, m in dK():      # (one value at a time: 83 longdouble matrices of n = 512 are not kept together)
        yield k, G * m, Gabs * np.abs(m)


def sums_ref(c, alpha, Kinv, dtype=np.longdouble):
    """(S, R): the 83 sums and their componentwise scales on the alpha and K^-1 GIVEN (entries that do not exist: 0)."""
    S, R = np.zeros(SUMS, dtype), np.zeros(SUMS, dtype)
    for k, T, W in terms(c, alpha, Kinv, dtype):
        S[k], R[k] = T.sum(), W.sum()
    return S, R


def term_ratio(c, alpha, Kinv):
    """Worst |term_f64 - term| / (u weight) over every term of every sum (what C_T is measured from)."""
    return max(_ratio(np.abs(ld(T64) - T), W)
               for (k, T, W), (_, T64, _w) in zip(terms(c, alpha, Kinv), terms(c, alpha, Kinv, np.float64)))


def chain(c, S, dtype=np.longdouble):
    """d(-mll) / d raw per slot from the sums S = d mll / d value: through sig and ntab to rho (prefix and running products),
    through the constraints' slopes, the sign flipped."""
    v, nl = values(c, dtype), c["nl"]
    S = np.asarray(S, dtype)
    dv = {"noise": S[S_TAU:S_TAU + 1], "os_s": S[S_OS_S:S_OS_S + 1], "ls_s": S[S_LS_S:S_LS_S + c["d"]],
          "os_n": S[S_OS_N:S_OS_N + 1], "ls_n": S[S_LS_N:S_LS_N + c["d"]]}
    if c["lin"]:
        rho = v["rho"]
        g = np.zeros(nl - 1, dtype)
        for q in range(nl - 1):
            run = np.prod(rho[:q]) if q else dtype(1)
            for l in range(q + 1, nl):
                g[q] += S[S_SIG + l] * run
                if l < nl - 1:
                    run = run * rho[l]
            k = q + 2
            if 3 <= k <= nl - 2:
                g[q] += 2 * rho[q] * S[S_NTAB + k - 1:S_NTAB + nl].sum()
        dv["rho"] = g
    return {s: -dv[s] * _slope(c["con"][s], c["raw"][s], dtype) for s in dv}


def given_from_float64(c):
    """(alpha, K^-1) of the case as float64, from the float64 covariance, refined by one Newton step in longdouble (tests of
    the restatement itself; the GPU tests take the DEVICE's alpha and K^-1)."""
    K = covariance(c)
    X = ld(np.linalg.inv(np.asarray(K, np.float64)))
    X = X @ (2 * np.eye(c["n"], dtype=np.longdouble) - K @ X)
    return X @ ld(c["y"]), X


def mll_ref(c):
    K = np.asarray(covariance(c), np.float64)
    L = np.linalg.cholesky(K)
    a = np.linalg.solve(L, c["y"])
    return float(-0.5 * a @ a - np.log(np.diag(L)).sum() - 0.5 * c["n"] * np.log(2 * np.pi))


# ---- the update rule: fit()'s bookkeeping and torch-default Adam on given losses and gradients
class UpdateModel:
    """State of one model's optimiser: raw (flat), the best copy, Adam's moments, the counters -- advanced by ``step(loss,
    info, grad)`` and closed by ``finish(loss, info)`` exactly as mobocmf_exact_fit_update states them."""

    def __init__(self, raw, lr, betas=(0.9, 0.999), eps=1e-8, dtype=np.longdouble):
        self.raw = np.asarray(raw, dtype).copy()
        self.best = np.zeros_like(self.raw)
        self.m, self.v = np.zeros_like(self.raw), np.zeros_like(self.raw)
        self.lr, self.b1, self.b2, self.eps, self.dtype = dtype(lr), dtype(betas[0]), dtype(betas[1]), dtype(eps), dtype
        self.it, self.stopped_at, self.best_it, self.best_loss, self.restored, self.losses = 0, None, None, None, False, []

    def step(self, loss, info, grad):
        if self.stopped_at is not None:
            return
        if not np.isfinite(loss) or info != 0:
            self.stopped_at = self.it
            return
        self.losses.append(float(loss))
        if self.best_it is None or loss < self.best_loss:
            self.best_loss, self.best_it, self.best = loss, self.it, self.raw.copy()
        g, t = np.asarray(grad, self.dtype), self.it + 1
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        bc1, bc2s = 1 - self.b1 ** t, np.sqrt(1 - self.b2 ** t)
        self.raw = self.raw - (self.lr / bc1) * self.m / (np.sqrt(self.v) / bc2s + self.eps)
        self.it += 1

    def finish(self, loss, info):
        if self.best_it is not None and (not np.isfinite(loss) or info != 0 or loss > self.best_loss):
            self.raw, self.restored = self.best.copy(), True


def host_loop(model, num_iters, lr):
    """fit()'s loop restated on the torch statement of the likelihood (``marginal_log_likelihood(hip=False)``), recording what
    it sees: dict(losses, best, best_iteration, stopped_at, restored, final).  The model is fitted in place."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    best, state = None, None
    seen = dict(losses=[], best=None, best_iteration=None, stopped_at=None, restored=False, final=None)
    for it in range(num_iters):
        opt.zero_grad()
        loss = -model.marginal_log_likelihood(hip=False)
        if not bool(torch.isfinite(loss)):
            seen["stopped_at"] = it
            break
        seen["losses"].append(float(loss))
        if best is None or float(loss) < best:
            best, state = float(loss), {k: v.detach().clone() for k, v in model.state_dict().items()}
            seen["best"], seen["best_iteration"] = best, it
        loss.backward()
        opt.step()
    if state is not None:
        final = -model.marginal_log_likelihood(hip=False)
        seen["final"] = float(final)
        if not bool(torch.isfinite(final)) or float(final) > best:
            model.load_state_dict(state)
            seen["restored"] = True
    for p in model.parameters():
        p.grad = None
    return seen
