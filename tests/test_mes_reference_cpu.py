"""CPU proofs of tests/mes_reference.py: the float64 restatements against the package's own host statements, the golden file
against mpmath, and the host restatement under the gate the MI355X test applies (the case list is a condition: the float64
formula alone must pass on it)."""
import types

import numpy as np
import pytest
import torch

from mobocmf_amd.acquisition_functions.MESMOC_MFGP import MESMOC_MFGP
from tests import kernel_reference as KR
from tests import mes_reference as M


class _Stub:
    """A model whose predict returns given moments (T,), whatever X."""

    def __init__(self, mom, noise):
        self.mom = mom
        self.likelihood = types.SimpleNamespace(noise=noise.reshape(1))

    def predict(self, X, fidelity):
        return types.SimpleNamespace(mean=self.mom[0], variance=self.mom[1])


@pytest.mark.parametrize("shape", M.MES_SHAPES)
def test_mes_restatement_equals_the_host_forward(shape):
    """mes_torch on given moments == MESMOC_MFGP.coupled_acq (the sum of _MES_MFGP.forward times the feasibilities) on stub
    models returning those moments, and autograd through both, to 1e-14 relative."""
    c = M.mes_case(*shape)
    n_obj, n_con, T = shape
    mom = torch.tensor(c["moments"], requires_grad=True)
    noise, best = torch.tensor(c["noise"]), torch.tensor(c["best"])
    stubs = [_Stub(mom[m], noise[m]) for m in range(n_obj + n_con)]
    objectives = {"o%d" % p: stubs[p] for p in range(n_obj)}
    constraints = {"c%d" % q: stubs[n_obj + q] for q in range(n_con)}
    acq = MESMOC_MFGP(objectives, constraints, 2, 1, {k: best[p] for p, k in enumerate(objectives)},
                      {k: best[n_obj + q] for q, k in enumerate(constraints)})
    for k in objectives:
        acq.add_blackbox(0, k)
    for k in constraints:
        acq.add_blackbox(0, k, is_constraint=True)
    host = acq.coupled_acq(torch.zeros(T, 2, dtype=torch.float64), 0)
    (gh,) = torch.autograd.grad(host.sum(), mom)
    mom2 = torch.tensor(c["moments"], requires_grad=True)
    mine = M.mes_torch(mom2, noise, best, n_obj, n_con)
    (gm,) = torch.autograd.grad(mine.sum(), mom2)
    a, b = M.mes_f64(c)
    assert np.array_equal(a, mine.detach().numpy()) and np.array_equal(b, gm.numpy())
    for got, ref in ((mine.detach(), host.detach()), (gm, gh)):
        assert float((got - ref).abs().max()) <= 1e-14 * float(ref.abs().max() + 1e-300)


def test_mes_golden_file_is_what_mpmath_gives():
    pytest.importorskip("mpmath")
    G = M.mes_golden()
    for shape in M.MES_SHAPES:
        c, g = M.mes_case(*shape), G[shape]
        for k in ("moments", "noise", "best"):
            assert np.array_equal(c[k], g[k]), (shape, k)
        for k, v in zip(("acq", "seeds", "kappa", "clamped", "term"), M.mes_mp(c)):
            assert np.array_equal(v, g[k]), (shape, k)


def test_mes_cases_are_the_stated_ones_and_the_host_restatement_passes_the_gate():
    """Both regimes occur (cdf clamp free / binding), nothing lies within 1 of the kink, every unclamped term is > 0 in the
    reference -- and at the clamped points (z in 6..8, cdf frozen at 1 - E) the reference's term is < 0 BEFORE its outer
    clamp, so the value there is exactly 0 with zero seeds: the third clamp binds there and nowhere else.  The float64 host
    restatement passes the gate with C = 4 x MES_RATIO_MEASURED, and the recorded constants cover its own worst ratios."""
    worst, kinds = {}, set()
    for shape, g in M.mes_golden().items():
        mean, var = g["moments"][:, 0], g["moments"][:, 1]
        z = (g["best"][:, None] - mean) / np.sqrt(var)
        assert float(np.abs(z - M.MES_KINK).min()) >= 0.8      # (the kink itself is at 5.17)
        assert 0.05 <= var.min() and var.max() <= 2.0 and 1e-3 <= g["noise"].min() and g["noise"].max() <= 0.1
        cl = g["clamped"]
        assert np.array_equal(cl, z[:shape[0]] > 5.2)
        kinds |= set(np.unique(cl).tolist())
        assert (g["term"][~cl] > 0).all() and (g["term"][cl] < 0).all()
        assert (g["acq"][cl.all(0)] == 0).all() and (g["seeds"][:, :, cl.all(0)] == 0).all()
        acq, seeds = M.mes_f64(g)
        ok, r = M.mes_gate(acq, seeds, g["acq"], g["seeds"], M.mes_kappa_max(g["kappa"], cl))
        print(shape, r)
        assert ok, (shape, r)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert kinds == {False, True}
    print("host worst ratios", worst)
    for k, v in worst.items():
        assert v <= M.MES_RATIO_MEASURED[k], (k, v)
        assert M.MES_C[k] == 4.0 * M.MES_RATIO_MEASURED[k]


@pytest.mark.parametrize("cls", ["MFGP", "MFGP_lin"])
def test_predict_restatement_equals_the_posterior(cls):
    """exact_predict_ref on L^-1 and a of the model's own training covariance == _ExactMFGP.posterior (mean, variance) at every
    level to 1e-9 of kss (n cond u with two digits to spare: cond(K) < 1e4 asserted), and its gradient == autograd through the
    posterior to 1e-9 of the gradient's own scale R_grad."""
    from mobocmf_amd.models import mfgp
    n, d, T, nf = 40, 3, 7, 3 if cls == "MFGP_lin" else 2
    model = M.mes_models(n, d, nf, seed=3, classes={"m": getattr(mfgp, cls)})["m"]
    with torch.no_grad():
        noise = float(model.likelihood.noise)      # (0.1 as the constructor sets it, through the constraint's transform)
        assert abs(noise - 0.1) < 1e-7
        K = (model.covar_module(model.x_train, model.x_train) + noise * torch.eye(n, dtype=torch.float64)).numpy()
    assert np.linalg.cond(K) < 1e4
    L = np.linalg.cholesky(K)
    Linv = np.asarray(KR.tri_inverse_hp(L), np.float64)
    a = np.asarray(KR.matmul_hp(Linv, model.y_train.numpy()), np.float64)[:, 0]
    rng = np.random.default_rng(5)
    x, gm, gv = rng.random((T, d)), rng.standard_normal(T), rng.standard_normal(T)
    for level in range(nf):
        c = M.model_case(model, level, x, gm, gv)
        ref = M.exact_predict_ref(c, Linv, a)
        xt = torch.tensor(x, requires_grad=True)
        model.eval()
        post = model.posterior(torch.cat([xt, level * torch.ones(T, 1, dtype=torch.float64)], 1))
        model.train()
        mean, var = post.mean, post.variance
        (g,) = torch.autograd.grad((torch.tensor(gm) * mean).sum() + (torch.tensor(gv) * var).sum(), xt)
        tol = 1e-9 * c["kss"]
        assert float(np.abs(mean.detach().numpy() - ref["mean"]).max()) <= tol
        assert float(np.abs(var.detach().numpy() - ref["var"]).max()) <= tol
        assert bool(np.all(np.abs(g.numpy() - ref["grad"]) <= 1e-9 * ref["Rg"]))
        assert float(np.abs(ref["grad"]).max()) > 1e-3


def test_exact_predict_constant_is_the_measured_one():
    """Worst |k_f64 - k| / (u |k|) over the cases of the GPU test; the recorded EXACT_PREDICT_RATIO_MEASURED must cover it and
    not be stale (within a factor of two), and C_k is four times it."""
    worst = 0.0
    for n, d, T in M.EXACT_PREDICT_CASES:
        for kind, nl in M.EXACT_PREDICT_KINDS.items():
            for level in range(nl):
                worst = max(worst, M.kernel_ratio(M.exact_predict_case(n, d, T, kind, level)))
    print("k ratio worst", worst)
    assert worst <= M.EXACT_PREDICT_RATIO_MEASURED <= 2.0 * worst
    assert M.EXACT_PREDICT_CK == 4.0 * M.EXACT_PREDICT_RATIO_MEASURED


def test_predict_cases_have_mixed_seeds_and_every_level():
    for n, d, T in M.EXACT_PREDICT_CASES:
        c = M.exact_predict_case(n, d, T, "lin", 1)
        assert set(c["lev"].tolist()) == set(range(min(n, 3)))
        if T >= 5:
            assert (c["gm"] == 0).any() and (c["gm"] > 0).any() and (c["gm"] < 0).any() and (c["gv"] > 0).any() and (c["gv"] < 0).any()
            assert c["gm"][2] == 0 and c["gv"][2] == 0
    assert (M.kernel_tables("lin", 3)[0] < 0).any() and np.array_equal(M.kernel_tables("mf", 2)[1], [0.0, 1.0])
