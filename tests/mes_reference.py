"""References of the MES baseline's device path: the MES value and its seeds (mobocmf_mes_group_forward) and the frozen exact-GP
predict group (mobocmf_exact_predict).  CPU only; the GPU tests (test_hip_mes_kernel.py, test_hip_exact_predict.py,
test_hip_mes_search.py) and the CPU proofs (test_mes_reference_cpu.py) share it.

MES.  ``mes_torch`` is the float64 restatement on GIVEN moments (torch, differentiable: the host statement of
``_MES_MFGP.forward`` without a model in it); ``mes_mp`` the same value with ANALYTIC derivatives in mpmath at 50 digits --
tests/golden/make_mes_golden.py records it in tests/golden/mes_kernel_cases.npz, which is what the GPU test reads.

Gate of the MES kernel:  |got - ref| <= C u kappa_max (1 + |ref|),  kappa = 1 / (1 - cdf) per objective and point, kappa_max the
largest among the objectives at that point whose cdf clamp does not bind (1 where there is none).  The float64 formula loses
digits in 1 - Phi(z); C is measured: MES_C = 4 x MES_RATIO_MEASURED, the larger of the float64 host restatement's worst ratio on
the golden cases (value 10.21, d/dmean 70.41, d/dvar 93.93; test_mes_reference_cpu.py) and the device's on the
MI355X (value 10.21, d/dmean 69.86, d/dvar 93.28; printed by test_hip_mes_kernel.py), rounded up.

Exact-GP predict.  ``exact_predict_ref`` restates the algebra of include/mobocmf_hip.h in longdouble on the L^-1 and a GIVEN,
with the componentwise scales R of the bounds
    moments   (2 n + 4 + C_k) u R,          R_mean = |a|^T |L^-1| |k|,  R_var = kss + (|L^-1| |k|)^2         (predict_check's form)
    gradient  (3 n + 12 + 2 C_k) u R_grad,  R_grad = sum_r (|L^-1|^T (|g_m| |a| + 2 |g_v| |L^-1| |k|))_r |dk_r / dx_j|
|k| and |dk| being the sums of the absolute signal and noise terms.  Gradient count: w carries n + C_k (an n-term product on top
of k's own rounding), c = g_m a - 2 g_v w three more, e = L^-T c another n; dk_r/dx_j carries C_k and six operations (the
difference, two squared reciprocal lengthscales, two products, one sum, the product with the difference), e_r dk_r one, the sum
over r another n: 3 n + 12 + 2 C_k with two to spare.
C_k, the allowance for the rounding of k itself (per term 2 d + 4 operations and an exponential whose argument's error is
amplified by |arg|), is MEASURED as GRAM_C was: the worst |k_f64 - k| / (u |k|) of the float64 restatement of k against the
longdouble one over the cases of the GPU test is EXACT_PREDICT_RATIO_MEASURED, and C_k = 4 x that: the device precomputes
reciprocal lengthscales, fuses, and orders the sum otherwise, each worth a few u |arg|; the margin covers inputs not sampled.
"""
import math

import numpy as np
import torch

from tests.kernel_reference import U, exact_gp, factor_case, ld, matmul_hp, _ratio      # noqa: F401  (re-exported for the tests)

E = float(np.finfo(np.float32).eps)      # the host's CLAMP_LB

# ------------------------------------------------------------------------------------------------------------------ MES
MES_SHAPES = ((1, 0, 1), (2, 1, 5), (1, 2, 67), (3, 2, 200))      # (n_obj, n_con, T)
MES_RATIO_MEASURED = {"acq": 10.3, "dmean": 71.0, "dvar": 94.0}
MES_C = {k: 4.0 * v for k, v in MES_RATIO_MEASURED.items()}
MES_KINK = 5.2      # Phi(z) = 1 - E near z = 5.17: no case is within 1 of it


def mes_case(n_obj, n_con, T, seed=0):
    """Inputs of one shape: var ~ U(0.05, 2), noise ~ U(1e-3, 0.1), best ~ N(0, 1); z ~ U(-4, 3) at three points in four and
    z ~ U(6, 8) (the cdf clamp binds) at every fourth (t % 4 == 3), the mean placed accordingly.  float64 numpy."""
    n = n_obj + n_con
    rng = np.random.default_rng(1000 * n_obj + 100 * n_con + T + seed)
    var = rng.uniform(0.05, 2.0, (n, T))
    noise = rng.uniform(1e-3, 0.1, n)
    best = rng.standard_normal(n)
    z = np.where((np.arange(T) % 4 == 3)[None, :], rng.uniform(6.0, 8.0, (n, T)), rng.uniform(-4.0, 3.0, (n, T)))
    mean = best[:, None] - z * np.sqrt(var)
    moments = np.ascontiguousarray(np.stack([mean, var], 1))
    return dict(n_obj=n_obj, n_con=n_con, T=T, moments=moments, noise=noise, best=best)


def _ncdf(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))


def mes_torch(moments, noise, best, n_obj, n_con):
    """acq (T,) from ``moments`` (n, 2, T), ``noise`` (n,), ``best`` (n,), torch float64, differentiable: the expressions of
    ``_MES_MFGP.forward`` and ``MESMOC_MFGP.coupled_acq`` operation for operation, on given moments."""
    T = moments.shape[2]
    acq = torch.zeros(T, dtype=moments.dtype, device=moments.device)
    feas = torch.ones(T, dtype=moments.dtype, device=moments.device)
    for m in range(n_obj + n_con):
        mean, var = moments[m, 0], moments[m, 1]
        stdv = var.sqrt()
        z = (best[m] - mean) / stdv
        if m >= n_obj:
            feas = feas * (1.0 - _ncdf(z))
            continue
        cdf = _ncdf(z).clamp_max(1 - E)
        pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        ratio = pdf / (1.0 - cdf)
        var_trunc = var * (1 + (z - ratio) * ratio).clamp_min(E) + noise[m]
        acq = acq + torch.clamp(0.5 * torch.log(var + noise[m]) - 0.5 * torch.log(var_trunc), min=0.0)
    return acq * feas


def mes_f64(c):
    """(acq (T,), seeds (n, 2, T)) of a case as float64 numpy: ``mes_torch`` and torch.autograd through it."""
    mom = torch.tensor(c["moments"], dtype=torch.float64, requires_grad=True)
    acq = mes_torch(mom, torch.tensor(c["noise"]), torch.tensor(c["best"]), c["n_obj"], c["n_con"])
    (g,) = torch.autograd.grad(acq.sum(), mom)
    return acq.detach().numpy(), g.numpy()


def mes_mp(c, dps=50):
    """The same at ``dps`` digits with analytic derivatives: (acq (T,), seeds (n, 2, T), kappa (n_obj, T), clamped (n_obj, T)
    bool: the cdf clamp binds, term (n_obj, T)) as float64 numpy (rounded once).  The three clamps pass where they do not
    bind; under a binding cdf clamp the cdf is a constant while phi still varies."""
    import mpmath as mp
    mp.mp.dps = dps
    n_obj, n_con, T = c["n_obj"], c["n_con"], c["T"]
    n = n_obj + n_con
    Em, half, one = mp.mpf(E), mp.mpf("0.5"), mp.mpf(1)
    acq, seeds = np.zeros(T), np.zeros((n, 2, T))
    kappa, clamped, term = np.ones((n_obj, T)), np.zeros((n_obj, T), bool), np.zeros((n_obj, T))
    for t in range(T):
        val, gm, gv = [], [], []
        for m in range(n):
            mean, var = mp.mpf(float(c["moments"][m, 0, t])), mp.mpf(float(c["moments"][m, 1, t]))
            tau, b = mp.mpf(float(c["noise"][m])), mp.mpf(float(c["best"][m]))
            s = mp.sqrt(var)
            z = (b - mean) / s
            Phi, pdf = mp.ncdf(z), mp.npdf(z)
            dz_dm, dz_dv = -one / s, -half * z / var
            if m >= n_obj:
                val.append(one - Phi)
                gm.append(-pdf * dz_dm)
                gv.append(-pdf * dz_dv)
                continue
            bind = Phi > one - Em
            cdf = one - Em if bind else Phi
            r = pdf / (one - cdf)
            u = one + (z - r) * r
            floor = u < Em
            g = Em if floor else u
            vt = var * g + tau
            diff = half * mp.log(var + tau) - half * mp.log(vt)
            kappa[m, t], clamped[m, t], term[m, t] = float(one / (one - cdf)), bool(bind), float(diff)
            if diff < 0:
                val.append(mp.mpf(0)); gm.append(mp.mpf(0)); gv.append(mp.mpf(0))
                continue
            dr_dz = -z * r + (mp.mpf(0) if bind else r * r)
            du_dz = mp.mpf(0) if floor else r + (z - 2 * r) * dr_dz
            dl = half / vt * var * du_dz
            val.append(diff)
            gm.append(-dl * dz_dm)
            gv.append(half / (var + tau) - half / vt * g - dl * dz_dv)
        total = mp.fsum(val[:n_obj])
        feas = mp.fprod(val[n_obj:]) if n_con else one
        acq[t] = float(total * feas)
        for m in range(n):
            scale = feas if m < n_obj else total * mp.fprod([val[k] for k in range(n_obj, n) if k != m])
            seeds[m, 0, t], seeds[m, 1, t] = float(scale * gm[m]), float(scale * gv[m])
    return acq, seeds, kappa, clamped, term


def mes_kappa_max(kappa, clamped):
    """(T,): the largest kappa among the objectives whose cdf clamp does not bind at that point, 1 where there is none."""
    return np.where(clamped, 1.0, kappa).max(0)


def mes_ratios(acq, seeds, ref_acq, ref_seeds, kmax):
    """Worst |got - ref| / (u kappa_max (1 + |ref|)) of the value, d/dmean and d/dvar (a NaN counts as infinite)."""
    def worst(got, ref):
        q = np.abs(np.asarray(got, np.float64) - ref) / (U * kmax * (1.0 + np.abs(ref)))
        return float(np.max(np.where(np.isnan(q), np.inf, q)))
    return {"acq": worst(acq, ref_acq), "dmean": worst(seeds[:, 0], ref_seeds[:, 0]), "dvar": worst(seeds[:, 1], ref_seeds[:, 1])}


def mes_gate(acq, seeds, ref_acq, ref_seeds, kmax):
    """(ok, ratios) under MES_C."""
    r = mes_ratios(acq, seeds, ref_acq, ref_seeds, kmax)
    return all(r[k] <= MES_C[k] for k in r), r


_golden = None


def mes_golden():
    """tests/golden/mes_kernel_cases.npz as {shape: dict(case inputs, acq, seeds, kappa, clamped, term)} (read once)."""
    global _golden
    if _golden is None:
        import os
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mes_kernel_cases.npz"))
        _golden = {}
        for shape in MES_SHAPES:
            p = "o%d_c%d_T%d_" % shape
            g = {k: z[p + k] for k in ("moments", "noise", "best", "acq", "seeds", "kappa", "clamped", "term")}
            g.update(n_obj=shape[0], n_con=shape[1], T=shape[2])
            _golden[shape] = g
    return _golden


# ------------------------------------------------------------------------------------------------------ exact-GP predict
EXACT_PREDICT_RATIO_MEASURED = 8.0
EXACT_PREDICT_CK = 4.0 * EXACT_PREDICT_RATIO_MEASURED
EXACT_PREDICT_CASES = ((1, 1, 1), (15, 2, 5), (17, 3, 16), (65, 2, 17), (130, 8, 33), (512, 2, 5))      # (n, d, T)
EXACT_PREDICT_KINDS = {"mf": 2, "lin": 3}      # kernel class -> fidelity levels


def kernel_tables(kind, n_levels):
    """(sig, ntab) per level as the kernel classes' own hip_factors / hip_noise_table give them: MFKernel -- sig all ones, ntab
    the min level itself; MFKernel_lin with rho = (0.7, -0.5, ...) -- sig the cumulative products (mixed sign)."""
    from mobocmf_amd.models.mfgp import MFKernel, MFKernel_lin
    rows = torch.zeros(n_levels, 2, dtype=torch.float64)
    rows[:, 1] = torch.arange(n_levels, dtype=torch.float64)
    if kind == "mf":
        cm = MFKernel(2, torch.tensor(1.0, dtype=torch.float64))
    else:
        cm = MFKernel_lin(2, torch.tensor(1.0, dtype=torch.float64), n_levels)
        with torch.no_grad():
            cm.rho.copy_(torch.tensor([0.7, -0.5, 1.2, 0.9, -1.1, 0.8, 0.6][:n_levels - 1], dtype=cm.rho.dtype))
    _, sig = cm.hip_factors(rows)
    sig = torch.ones(n_levels, dtype=torch.float64) if sig is None else sig
    return sig.double().numpy().copy(), cm.hip_noise_table(n_levels, "cpu").double().numpy().copy()


_predict_cache = {}


def exact_predict_case(n, d, T, kind, level, seed=0):
    """One model of a predict test, float64 numpy, read-only and cached: training inputs and test points uniform in [0, 1]^d,
    levels uniform over the kernel's levels (each present where n allows), lengthscales in [0.5, 1.5] (signal) and [0.4, 1.2]
    (noise) so that |arg| stays below 16 at d = 8, seeds of mixed sign with every third exactly zero.  The training
    covariance -- K, y = factor_case("rbf", n): the workload's conditioning -- is independent of these (the kernel's contract
    is on the L^-1 and a GIVEN)."""
    key = (n, d, T, kind, level, seed)
    if key not in _predict_cache:
        nl = EXACT_PREDICT_KINDS[kind]
        rng = np.random.default_rng(100003 * n + 1009 * d + 31 * T + 7 * nl + level + seed)
        lev = rng.integers(0, nl, n).astype(np.int32)
        lev[:min(n, nl)] = np.arange(min(n, nl))
        sig, ntab = kernel_tables(kind, nl)
        hyp_s = np.concatenate([[1.3], rng.uniform(0.5, 1.5, d)])
        hyp_n = np.concatenate([[0.2], rng.uniform(0.4, 1.2, d)])
        sign = (-1.0) ** np.arange(T)
        gm, gv = sign * np.abs(rng.standard_normal(T)), sign * np.abs(rng.standard_normal(T))
        gm[::3] = 0.0
        gv[1::3] = 0.0
        if T > 2:
            gm[2], gv[2] = 0.0, 0.0      # a point whose seeds are both zero
        c = dict(n=n, d=d, T=T, kind=kind, n_levels=nl, level=level, xtr=rng.random((n, d)), lev=lev, sig=sig, ntab=ntab,
                 hyp_s=hyp_s, hyp_n=hyp_n, x=rng.random((T, d)), gm=gm, gv=gv,
                 kss=float(sig[level] * sig[level] * hyp_s[0] + ntab[level] * hyp_n[0]))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _predict_cache[key] = c
    return _predict_cache[key]


def kernel_terms(c, dtype=np.longdouble):
    """(S, N, diff): signal and noise term of k (n x T) and x_tj - X_rj (n x T x d), the header's expressions in ``dtype``."""
    f = lambda a: np.asarray(a, dtype)
    diff = f(c["x"])[None, :, :] - f(c["xtr"])[:, None, :]
    lev, level = c["lev"], c["level"]
    half = dtype(0.5)
    qs = ((diff / f(c["hyp_s"][1:])) ** 2).sum(-1)
    qn = ((diff / f(c["hyp_n"][1:])) ** 2).sum(-1)
    S = (f(c["sig"])[level] * f(c["sig"])[lev] * f(c["hyp_s"][0]))[:, None] * np.exp(-half * qs)
    N = (f(c["ntab"])[np.minimum(level, lev)] * f(c["hyp_n"][0]))[:, None] * np.exp(-half * qn)
    return S, N, diff


def exact_predict_ref(c, Linv, a):
    """The algebra of mobocmf_exact_predict in longdouble on the ``Linv`` (n x n, lower triangle used) and ``a`` GIVEN.
    Returns dict(mean, var, grad (T x d), Rm, Rv, Rg): references and the componentwise scales of the bounds (module docstring)."""
    n = c["n"]
    Li = np.tril(np.asarray(Linv, np.float64)[:n, :n])
    av = ld(np.asarray(a, np.float64)[:n])
    S, N, diff = kernel_terms(c)
    k, kabs = S + N, np.abs(S) + np.abs(N)
    W = matmul_hp(Li, k)
    mean, var = av @ W, ld(c["kss"]) - (W * W).sum(0)
    G = matmul_hp(np.abs(Li), kabs)
    Rm, Rv = np.abs(av) @ G, abs(ld(c["kss"])) + (G * G).sum(0)
    gm, gv = ld(c["gm"]), ld(c["gv"])
    e = matmul_hp(Li.T, gm[None, :] * av[:, None] - 2 * gv[None, :] * W)
    eabs = matmul_hp(np.abs(Li).T, np.abs(gm)[None, :] * np.abs(av)[:, None] + 2 * np.abs(gv)[None, :] * G)
    is2, in2 = 1 / ld(c["hyp_s"][1:]) ** 2, 1 / ld(c["hyp_n"][1:]) ** 2
    dk = -diff * (S[:, :, None] * is2 + N[:, :, None] * in2)
    dkabs = np.abs(diff) * (np.abs(S)[:, :, None] * is2 + np.abs(N)[:, :, None] * in2)
    return dict(mean=mean, var=var, grad=(e[:, :, None] * dk).sum(0), Rm=Rm, Rv=Rv, Rg=(eabs[:, :, None] * dkabs).sum(0))


def moments_units(n):
    return 2 * n + 4 + EXACT_PREDICT_CK


def grad_units(n):
    return 3 * n + 12 + 2 * EXACT_PREDICT_CK


def exact_predict_check(c, ref, mean, var, grad=None):
    """(ok, ratios in u R) of device results against ``ref`` = exact_predict_ref(...) under the bounds of the module docstring."""
    n = c["n"]
    em, ev = np.abs(ld(mean) - ref["mean"]), np.abs(ld(var) - ref["var"])
    r = {"mean": _ratio(em, ref["Rm"]), "var": _ratio(ev, ref["Rv"])}
    ok = r["mean"] <= moments_units(n) and r["var"] <= moments_units(n)
    if grad is not None:
        r["grad"] = _ratio(np.abs(ld(grad) - ref["grad"]), ref["Rg"])
        ok = ok and r["grad"] <= grad_units(n)
    return bool(ok), r


def kernel_ratio(c):
    """Worst |k_f64 - k| / (u |k|) of the float64 restatement of k against the longdouble one (what C_k is measured from)."""
    S, N, _ = kernel_terms(c)
    S64, N64, _ = kernel_terms(c, np.float64)
    return _ratio(np.abs(ld(S64 + N64) - (S + N)), np.abs(S) + np.abs(N))


# ------------------------------------------------------------------------------------------------------ the public surface
def model_case(model, level, x, gm=None, gv=None):
    """The exact_predict_case form of a live ``MFGP`` / ``MFGP_lin`` (CPU, float64) at ``level`` and test points ``x`` (T x d)."""
    cm, d, nl = model.covar_module, model.input_dim, model.num_fidelities
    rows = torch.zeros(nl, d + 1, dtype=torch.float64)
    rows[:, d] = torch.arange(nl, dtype=torch.float64)
    with torch.no_grad():
        lev, _ = cm.hip_factors(model.x_train)
        _, sig = cm.hip_factors(rows)
        sig = torch.ones(nl, dtype=torch.float64) if sig is None else sig
        ntab = cm.hip_noise_table(nl, "cpu")
        hyp = [torch.cat([k.outputscale.reshape(1), k.base_kernel.lengthscale.reshape(-1)]).double().numpy()
               for k in (cm.cov_funct_signal, cm.cov_funct_noise)]
    sig, ntab = sig.double().numpy(), ntab.double().numpy()
    T = x.shape[0]
    return dict(n=model.x_train.shape[0], d=d, T=T, n_levels=nl, level=level, xtr=model.x_train[:, :d].numpy(), lev=lev.numpy(),
                sig=sig, ntab=ntab, hyp_s=hyp[0], hyp_n=hyp[1], x=np.asarray(x, np.float64),
                gm=np.zeros(T) if gm is None else gm, gv=np.zeros(T) if gv is None else gv,
                kss=float(sig[level] * sig[level] * hyp[0][0] + ntab[level] * hyp[1][0]))


def mes_models(n, d=2, n_fid=2, seed=0, device="cpu", classes=None):
    """{name: unfitted-but-initialised exact GP} on n rows each, the levels cycling over the rows: objectives o0 (MFGP), o1
    (MFGP_lin), constraint c0 (MFGP), the default lengthscale and noise 0.1 (cond(K) in the hundreds)."""
    from mobocmf_amd.models.mfgp import MFGP, MFGP_lin
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, (name, cls) in enumerate((classes or {"o0": MFGP, "o1": MFGP_lin, "c0": MFGP}).items()):
        x = torch.rand(n, d, generator=g, dtype=torch.float64)
        fid = (torch.arange(n) % n_fid).double()[:, None]
        y = torch.sin(3.0 * x.sum(1) + k) + 0.3 * fid[:, 0] + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
        out[name] = cls(torch.cat([x, fid], 1), y, n_fid).to(device)
    return out


def mes_problem(n, d=2, n_fid=2, seed=0, device="cpu", search="host", models=None):
    """A ``MESMOC_MFGP`` over ``mes_models``: two objectives and one constraint registered at every fidelity (cost 1 + f), the
    unit box."""
    from mobocmf_amd.acquisition_functions.MESMOC_MFGP import MESMOC_MFGP
    models = mes_models(n, d, n_fid, seed, device) if models is None else models
    objectives = {k: m for k, m in models.items() if k.startswith("o")}
    constraints = {k: m for k, m in models.items() if k.startswith("c")}
    bounds = torch.tensor([[0.0] * d, [1.0] * d], dtype=torch.float64, device=device)
    acq = MESMOC_MFGP(objectives, constraints, d, n_fid, {"o0": 0.3, "o1": -0.2}, {"c0": 0.1}, standard_bounds=bounds, search=search)
    for f in range(n_fid):
        for name in objectives:
            acq.add_blackbox(f, name, cost_evaluation=1.0 + f)
        for name in constraints:
            acq.add_blackbox(f, name, is_constraint=True)
    return acq
