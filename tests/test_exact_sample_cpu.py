"""The exact-GP function sample on the CPU: the host engine of mobocmf_amd/util/exact_sample.py against the longdouble
restatement tests/exact_sample_reference.py, the identities that tie block order, folding, scales and packing to the algebra, the
distribution of the draws, and ``sample_pareto_front`` on CPU models."""
import numpy as np
import pytest
import torch

from tests import exact_sample_reference as S
from tests import mes_reference as M

U = S.U
needs_ld = pytest.mark.skipif(not S.HAVE_LONGDOUBLE, reason="numpy longdouble is float64 on this platform")


def _split(c):
    """(model operands, draws) of a reference case as float64 CPU tensors, in the form the engines take."""
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt)
    ops = dict(x=t(c["x"]), lev=t(c["lev"], torch.int32), y=t(c["y"]), sig=t(c["sig"]), ntab=t(c["ntab"]),
               sqd=t(S.tables(c["ntab"])), scal=t(c["scal"]))
    rnd = {k: t(c[k]) for k in ("W_sig", "b_sig", "W_noi", "b_noi", "theta0", "e")}
    return ops, rnd


def _restate(c, levels=()):
    return S.restate(c["x"], c["lev"], c["y"], c["sig"], c["ntab"], c["scal"], c["W_sig"], c["b_sig"], c["W_noi"], c["b_noi"],
                     c["theta0"], c["e"], levels=levels)


def solve_bounds(c, R):
    """First-order bounds on ||w^ - w||_2 and ||theta^ - theta||_2 of a float64 evaluation of the algebra, from its operation
    counts.  With m = (1 + n_levels) F terms per entry of Phi^T Phi and of Phi^T theta0, A_max the largest cosine argument sum and
    kappa = cond_2(G):
      * G^: each entry m products of cosines carrying (d + 1) A u + 4 u each  ->  relative perturbation (2 (d + 1) A_max + m + 16) u
        on |Phi|^T |Phi|, which kappa carries to w;
      * the Cholesky solve is backward stable with a constant of at most 3 n + 8 (Higham, Accuracy and Stability, Thm 10.4);
      * r^: (m + 2) u (|y| + |Phi|^T |theta0| + |e|), which ||G^-1||_2 carries to w;
      * theta^ = theta0 + Phi w^: ||Phi||_2 times the bound on w, and (n + 2) u (|theta0| + |Phi| |w|) for the product itself.
    Nothing here comes from a measured error."""
    ld = S.ld
    n, m = R["G"].shape[0], R["Phi"].shape[0]
    G64 = np.asarray(R["G"], np.float64)
    sv = np.linalg.svd(G64, compute_uv=False)
    kappa, ginv = sv[0] / sv[-1], 1.0 / sv[-1]
    amax = float(max(R["A_sig"].max(), R["A_noi"].max()))
    cst = 3 * n + 8 + 2 * (R["d"] + 1) * amax + m + 16
    absPhi = np.abs(R["Phi"])
    rabs = np.abs(R["y"]) + absPhi.T @ np.abs(R["theta0"]) + np.abs(R["e"])
    nrm = lambda v: float(np.sqrt((ld(v) ** 2).sum()))
    bw = U * (cst * kappa * nrm(R["w"]) + (m + 2) * ginv * nrm(rabs))
    phi2 = float(np.linalg.svd(np.asarray(R["Phi"], np.float64), compute_uv=False)[0])
    bt = phi2 * bw + (n + 2) * U * nrm(np.abs(R["theta0"]) + absPhi @ np.abs(R["w"]))
    return bw, bt, kappa


# ------------------------------------------------------------------------------------------- 1. host engine / restatement
@needs_ld
@pytest.mark.parametrize("shape", [(40, 2, 3, 64, "min"), (17, 9, 5, 33, "lin"), (1, 1, 1, 1, "min")], ids=str)
def test_host_engine_matches_the_longdouble_restatement(shape):
    from mobocmf_amd.util.exact_sample import host_draw
    n, d, nl, F, kern = shape
    c = S.case(n, d, nl, F, kern)
    R = _restate(c, levels=range(nl))
    ops, rnd = _split(c)
    got = host_draw(ops, rnd, range(nl))
    bw, bt, kappa = solve_bounds(c, R)
    ew = float(np.sqrt(((S.ld(got.w.numpy()) - R["w"]) ** 2).sum()))
    et = float(np.sqrt(((S.ld(got.theta.numpy()) - R["theta"]) ** 2).sum()))
    print("host engine %s: cond %.2e  |dw| %.3e (bound %.3e)  |dtheta| %.3e (bound %.3e)" % (shape, kappa, ew, bw, et, bt))
    assert ew <= bw and et <= bt
    for f in range(nl):      # the folded operands are the restatement's, to the same bound times the fold's scales
        th = got.samples[f].layers[0]["theta"].numpy()
        scale = float(max(np.abs(c["sig"]).max() * R["c_sig"], R["c_noi"] * np.abs(R["sqd"]).sum()))
        assert float(np.abs(S.ld(th) - R["folded"][f]).max()) <= scale * bt + 8 * U * float(np.abs(R["folded"][f]).max())


@needs_ld
def test_the_two_statements_of_G_agree():
    c = S.case(40, 2, 3, 64, "lin")
    R = _restate(c)
    assert float(np.abs(R["G"] - R["G_phi"]).max()) <= 1e-15 * float(np.abs(R["G"]).max())


# ------------------------------------------------------------------------------------------- 2. the interpolation identity
def _identity_residuals(draw, ops):
    """max over the rows of |g_{l_i}(x_i) + e_i + noise w_i - y_i|, the samples evaluated through RFFChainSample.__call__."""
    x, lev, y = ops["x"].cpu().numpy(), ops["lev"].cpu().numpy(), ops["y"].cpu().numpy()
    w, e, noise = draw.w.cpu().numpy(), draw.e.cpu().numpy(), float(draw.noise)
    res = np.zeros(x.shape[0])
    for f, smp in draw.samples.items():
        rows = lev == f
        if rows.any():
            res[rows] = smp(x[rows]) + e[rows] + noise * w[rows] - y[rows]
    return np.abs(res)


def identity_bound(R):
    """The identity is the solved system G w = r read row by row, so its residual is the solve's BACKWARD error (independent of
    cond(G)): (3 n + 8) u ||G||_2 ||w||_2 for the Cholesky solve (Higham Thm 10.4), plus the evaluation of both sides in
    float64 -- m = (1 + n_levels) F terms on each, twice: (2 m + 2 (d + 1) A_max + 16) u (|y| + |Phi|^T |theta| + |e| + noise |w|)."""
    n, m = R["G"].shape[0], R["Phi"].shape[0]
    g2 = float(np.linalg.svd(np.asarray(R["G"], np.float64), compute_uv=False)[0])
    amax = float(max(R["A_sig"].max(), R["A_noi"].max()))
    mag = np.abs(R["y"]) + np.abs(R["Phi"]).T @ np.abs(R["theta"]) + np.abs(R["e"]) + R["noise"] * np.abs(R["w"])
    return float(U * ((3 * n + 8) * g2 * np.sqrt((R["w"] ** 2).sum()) + (2 * m + 2 * (R["d"] + 1) * amax + 16) * mag.max()))


@needs_ld
@pytest.mark.parametrize("kern", ["min", "lin"])
def test_interpolation_identity_through_the_returned_samples(kern):
    from mobocmf_amd.layers.rff import RFFChainSample
    from mobocmf_amd.util.exact_sample import host_draw
    c = S.case(40, 2, 3, 64, kern, noise=1e-2)
    ops, rnd = _split(c)
    draw = host_draw(ops, rnd, range(3))
    res, bound = _identity_residuals(draw, ops), identity_bound(_restate(c))
    print("interpolation identity (%s): residual %.3e (bound %.3e)" % (kern, res.max(), bound))
    assert res.max() <= bound
    for smp in draw.samples.values():      # F' = 2F, alpha = s0^2 F' / 2, and the pack round trip is bitwise
        L = smp.layers[0]
        assert L["F"] == 128 and L["alpha"] == L["scales"][0] ** 2 * L["F"] / 2
        buf = smp.pack()
        back = RFFChainSample.unpack(buf)
        assert torch.equal(back.pack().view(torch.int64), buf.view(torch.int64))
        xt = torch.as_tensor(c["x"])
        assert torch.equal(back._torch(xt), smp._torch(xt))
        assert torch.equal(smp.negated()._torch(xt), -smp._torch(xt))


# ------------------------------------------------------------------------------------------- 3. MFGP_lin, the rho^2 terms live
@needs_ld
def test_mfgp_lin_tables_reproduce_the_kernel_and_the_feature_expansion():
    from mobocmf_amd.models.mfgp import MFGP_lin
    from mobocmf_amd.util.exact_sample import draw_operands, model_operands
    g = torch.Generator().manual_seed(3)
    n, d, nf = 30, 2, 5
    x = torch.rand(n, d, generator=g, dtype=torch.float64)
    fid = (torch.arange(n) % nf).double()[:, None]
    model = MFGP_lin(torch.cat([x, fid], 1), torch.randn(n, generator=g, dtype=torch.float64), nf)
    with torch.no_grad():
        model.covar_module.rho.copy_(torch.tensor([0.7, -0.5, 0.9, 0.6], dtype=torch.float64))
    ops = model_operands(model)
    assert float(ops["ntab"][2] - ops["ntab"][1]) == pytest.approx(0.25)      # rho[1]^2 enters at min level 2
    # the tables restate MFKernel_lin.forward
    from mobocmf_amd.models.mfgp import _rbf
    cm = model.covar_module
    with torch.no_grad():
        Ks = cm.cov_funct_signal.outputscale * _rbf(x, x, cm.cov_funct_signal.base_kernel.lengthscale)
        Kn = cm.cov_funct_noise.outputscale * _rbf(x, x, cm.cov_funct_noise.base_kernel.lengthscale)
        lev = ops["lev"].long()
        K_tab = ops["sig"][lev][:, None] * ops["sig"][lev][None, :] * Ks + ops["ntab"][torch.minimum(lev[:, None], lev[None, :])] * Kn
        K_fwd = cm(model.x_train, model.x_train)
    assert float((K_tab - K_fwd).abs().max()) <= 16 * U * float(K_fwd.abs().max())
    assert torch.allclose(ops["sqd"] ** 2, ops["ntab"] - torch.cat([torch.zeros(1, dtype=torch.float64), ops["ntab"][:-1]]), atol=1e-15)
    # for fixed features, Phi^T Phi from the tables is the feature expansion
    rnd = draw_operands(model, 48, torch.Generator().manual_seed(4), ops)
    num = lambda t: t.detach().numpy()
    R = S.restate(num(ops["x"]), num(ops["lev"]), num(ops["y"]), num(ops["sig"]), num(ops["ntab"]), num(ops["scal"]),
                  num(rnd["W_sig"]), num(rnd["b_sig"]), num(rnd["W_noi"]), num(rnd["b_noi"]), num(rnd["theta0"]), num(rnd["e"]))
    assert float(np.abs(R["G"] - R["G_phi"]).max()) <= 1e-15 * float(np.abs(R["G"]).max())


# ------------------------------------------------------------------------------------------- 4. the distribution, exactly
def test_draws_have_the_weight_space_posterior_moments():
    """Features fixed, 2000 (theta0, e) pairs: mean and variance of g_f(x*) at three points within five standard errors of
    phi*^T A^-1 Phi y and noise phi*^T A^-1 phi*, A = Phi Phi^T + noise I (standard errors of a Gaussian sample: sqrt(var / N) and
    var sqrt(2 / (N - 1)))."""
    from mobocmf_amd.util.exact_sample import host_draw
    n, d, nl, F, N, top = 12, 2, 3, 32, 2000, 2
    c = S.case(n, d, nl, F, "lin", seed=5, noise=0.05)
    ops, rnd = _split(c)
    g = torch.Generator().manual_seed(11)
    xs = torch.rand(3, d, generator=g, dtype=torch.float64)
    noise = float(c["scal"][2])
    theta0 = torch.randn(N, (1 + nl) * F, generator=g, dtype=torch.float64)
    e = np.sqrt(noise) * torch.randn(N, n, generator=g, dtype=torch.float64)
    vals = torch.zeros(N, 3, dtype=torch.float64)
    for k in range(N):
        vals[k] = host_draw(ops, dict(rnd, theta0=theta0[k], e=e[k]), [top]).samples[top]._torch(xs)
    # the weight-space posterior in float64 numpy
    sqd = S.tables(c["ntab"])
    cs, cn = np.sqrt(2 * c["scal"][0] / F), np.sqrt(2 * c["scal"][1] / F)

    def phi(x, lev):
        Cs, Cn = np.cos(c["W_sig"] @ x.T + c["b_sig"][:, None]), np.cos(c["W_noi"] @ x.T + c["b_noi"][:, None])
        return np.concatenate([c["sig"][lev] * cs * Cs] + [sqd[l] * cn * Cn * (lev >= l) for l in range(nl)], 0)

    Phi, ps = phi(c["x"], c["lev"].astype(np.int64)), phi(xs.numpy(), np.full(3, top))
    A = Phi @ Phi.T + noise * np.eye(Phi.shape[0])
    mean = ps.T @ np.linalg.solve(A, Phi @ c["y"])
    var = noise * np.einsum("fi,fi->i", ps, np.linalg.solve(A, ps))
    m_hat, v_hat = vals.mean(0).numpy(), vals.var(0, unbiased=True).numpy()
    print("distribution: mean off by %s standard errors, variance by %s" %
          (np.round(np.abs(m_hat - mean) / np.sqrt(var / N), 2), np.round(np.abs(v_hat - var) / (var * np.sqrt(2.0 / (N - 1))), 2)))
    assert np.all(np.abs(m_hat - mean) <= 5 * np.sqrt(var / N))
    assert np.all(np.abs(v_hat - var) <= 5 * var * np.sqrt(2.0 / (N - 1)))


# ------------------------------------------------------------------------------------------- 5. sample_pareto_front, host
def test_sample_pareto_front_on_cpu_models():
    from mobocmf_amd.util.mes_front import sample_pareto_front
    models = M.mes_models(12, 2, 2, seed=2)
    objs = {k: m for k, m in models.items() if k.startswith("o")}
    cons = {k: m for k, m in models.items() if k.startswith("c")}
    inputs = models["o0"].x_train[:, :2].numpy()
    out = sample_pareto_front(objs, cons, {"c0": -0.5}, inputs, 2, nFeatures=24, generator=torch.Generator().manual_seed(0),
                              rng=np.random.default_rng(0), engine="host", grid_size=40)
    front, pset = out.pareto_front.numpy(), out.pareto_set.numpy()
    assert set(out.engines.values()) == {"host"} and set(out.engines) == {"o0", "o1", "c0"}
    assert out.tries >= 1 and not out.fallback and front.shape[0] >= 1 and front.shape[1] == 2
    for j, k in enumerate(objs):
        assert out.best_objective_values[k] == -front[:, j].min()
        assert np.allclose(-out.samples_objs[k](pset), front[:, j], rtol=0, atol=1e-12)      # MOOP saw the negated samples
    assert np.all(out.samples_cons["c0"](pset) >= -0.5 - 1e-6)                               # (SLSQP's constraint tolerance)
    # an unreachable threshold: every try fails, then the least infeasible rows serve
    out = sample_pareto_front(objs, cons, {"c0": 1e6}, inputs, 2, nFeatures=24, generator=torch.Generator().manual_seed(0),
                              rng=np.random.default_rng(0), engine="host", grid_size=40, max_tries=3)
    assert out.tries == 3 and out.fallback and out.pareto_front.shape[0] >= 1
    assert all(np.isfinite(v) for v in out.best_objective_values.values())


# ------------------------------------------------------------------------------------------- 6. errors
def test_errors():
    from mobocmf_amd.util.exact_sample import draw_chain_samples
    model = M.mes_models(8, 2, 2)["o0"]
    with pytest.raises(ValueError, match="engine"):
        model.sample_chain_from_posterior(1, nFeatures=8, engine="gpu")
    with pytest.raises(ValueError, match="fidelity"):
        model.sample_chain_from_posterior(2, nFeatures=8, engine="host")
    with pytest.raises(ValueError, match="fidelity"):
        model.sample_chain_from_posterior(-1, nFeatures=8, engine="host")
    with pytest.raises(RuntimeError, match="the model is not on the GPU"):
        model.sample_chain_from_posterior(1, nFeatures=8, engine="device")
    with pytest.raises(ValueError, match="engine"):
        draw_chain_samples([model], 1, engine="cuda")
    res = draw_chain_samples([model], 1, nFeatures=8, engine="device")      # the batched form falls back per model and says so
    assert res.engines == {0: "host"}
    smp = model.sample_chain_from_posterior(1, nFeatures=8, generator=torch.Generator().manual_seed(0), engine="host")
    again = model.sample_chain_from_posterior(1, nFeatures=8, generator=torch.Generator().manual_seed(0), engine="host")
    assert torch.equal(smp.pack(), again.pack()) and len(smp.layers) == 1 and smp.layers[0]["kind"] == 0 and smp.F == 16
