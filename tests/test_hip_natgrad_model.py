"""Natural gradients for q(u) through the model and the captured steps (variational_optimizer="natgrad"): the conjugate known
answer, the trajectory against the oracle's gradients with the restatement of tests/natgrad_reference.py applied to (m, L_S)
and torch.optim.Adam to the other leaves, and the mini-batch and conditioned steps."""
import copy

import pytest
import torch

from mobocmf_amd.util import synthetic
from oracle import mfdgp_oracle as O
from tests import natgrad_reference as R
from tests.helpers import to_t
from tests.test_hip_model import _model_param_for, _raw_from_model, build_model, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
GTOL = 1e-6      # the project's gradient tolerance for M < 128; the update is linear in those gradients


def _vd(model, l=0):
    return getattr(model, "hidden_layer_%d" % l).variational_strategy._variational_distribution


def _m_S(model, l=0):
    vd = _vd(model, l)
    L = torch.tril(vd.chol_variational_covar.detach().cpu())
    return vd.variational_mean.detach().cpu().clone(), L @ L.T


# ------------------------------------------------------------------ 6. known answer through the model
@pytest.fixture(scope="module")
def conjugate():
    """One fidelity (one layer, kind 0), N = 64, 24 inducing points, d = 2; the closed form on the CPU from the model's own
    K_mm + 1e-6 I, K_mn and noise; the restatement's own error against it fixes the tolerance."""
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.models import MFDGP
    g = torch.Generator().manual_seed(11)
    N, M, d = 64, 24, 2
    x = torch.rand(N, d, dtype=torch.float64, generator=g)
    y = (torch.sin(4.0 * x[:, :1]) + x[:, 1:] ** 2 + 0.05 * torch.randn(N, 1, dtype=torch.float64, generator=g))
    fid = torch.zeros(N, 1, dtype=torch.float64)
    torch.manual_seed(3)
    model = MFDGP(x, y, fid, num_fidelities=1, num_inducing=M)
    model.double()
    with torch.no_grad():      # a start away from the prior in both parameters, one negative diagonal entry
        vd = _vd(model)
        vd.chol_variational_covar.copy_(0.3 * torch.eye(M) + 0.05 * torch.tril(torch.randn(M, M, generator=g)))
        vd.chol_variational_covar[3, 3] *= -1.0
    layer = model.hidden_layer_0
    cm = layer.covar_module
    hyp = {"ls": cm.base_kernel.lengthscale.detach().double().reshape(-1), "alpha": cm.outputscale.detach().double().reshape(())}
    Z = layer.variational_strategy.Zx.detach().double().cpu()
    noise = model.hidden_layer_likelihood_0.noise.detach().double().reshape(())
    Kmm = O.gram(hyp, Z, Z) + 1e-6 * torch.eye(M, dtype=torch.float64)
    Kmn, knn = O.gram(hyp, Z, x), O.gram_diag(hyp, x)
    m_opt, S_opt, Lam_opt = R.conjugate_optimum(Kmm, Kmn, y[:, 0], noise)
    m0 = _vd(model).variational_mean.detach().double().clone()
    L0 = _vd(model).chol_variational_covar.detach().double().clone()

    def grads(m, L):
        m, L = m.clone().requires_grad_(True), L.clone().requires_grad_(True)
        R.conjugate_neg_elbo(m, L, Kmm, Kmn, knn, y[:, 0], noise).backward()
        return m.grad, L.grad

    m1, L1, _, ok = R.natgrad_update(m0, L0, *grads(m0, L0), 1.0)
    assert ok
    err = max(rel(L1 @ L1.T, S_opt), rel(m1, m_opt))
    tol = max(100.0 * err, GTOL)
    print("conjugate problem: the restatement's own error %.3e -> tolerance %.3e" % (err, tol))

    def make_step(gamma, use_graph):
        from mobocmf_amd.util.graphed_step import GraphedELBOStep
        mdl = copy.deepcopy(model).to(DEV)
        step = GraphedELBOStep(mdl, VariationalELBOMF(mdl, N, 1), x.to(DEV), y.to(DEV), fid.to(DEV), lr=0.0, use_graph=use_graph,
                               variational_optimizer="natgrad", natgrad_gamma=gamma, natgrad_gamma_init=gamma,
                               natgrad_warmup_steps=0)
        return mdl, step

    S0 = torch.tril(L0) @ torch.tril(L0).T
    return dict(make_step=make_step, m_opt=m_opt, S_opt=S_opt, Lam_opt=Lam_opt, tol=tol, m0=m0, S0=S0)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
def test_one_step_of_length_one_is_the_conjugate_optimum(conjugate, use_graph):
    c = conjugate
    model, step = c["make_step"](1.0, use_graph)
    step.step()
    step.check()
    m1, S1 = _m_S(model)
    errs = (rel(S1, c["S_opt"]), rel(m1, c["m_opt"]))
    print("after one step: rel err S %.3e m %.3e (tolerance %.3e)" % (errs + (c["tol"],)))
    assert max(errs) < c["tol"]
    step.step()
    step.check()
    m2, S2 = _m_S(model)
    assert rel(S2, S1) < c["tol"] and rel(m2, m1) < c["tol"]
    assert step.skipped_steps() == [0] and int(step.optimizer.natgrad_steps[0]) == 2
    step.close()


def test_natural_parameters_contract_geometrically(conjugate):
    """gamma = 0.5: S_t^-1 = Lambda* + 0.5^t (Lambda_0 - Lambda*) and S_t^-1 m_t likewise, t = 1..5."""
    c = conjugate
    model, step = c["make_step"](0.5, True)
    Lam0, th0 = torch.linalg.inv(c["S0"]), torch.linalg.solve(c["S0"], c["m0"])
    th_opt = c["Lam_opt"] @ c["m_opt"]
    for t in range(1, 6):
        step.step()
        step.check()
        m, S = _m_S(model)
        want_Lam = c["Lam_opt"] + 0.5 ** t * (Lam0 - c["Lam_opt"])
        want_th = th_opt + 0.5 ** t * (th0 - th_opt)
        errs = (rel(torch.linalg.inv(S), want_Lam), rel(torch.linalg.solve(S, m), want_th))
        print("t %d: rel err Lambda %.3e theta %.3e" % ((t,) + errs))
        assert max(errs) < c["tol"], t
    step.close()


# ------------------------------------------------------------------ 7. trajectory against the oracle
CFGS = [dict(d=2, L=2, M=8, N=12, S=3, seed=0), dict(d=3, L=3, M=10, N=16, S=2, seed=0), dict(d=3, L=3, M=10, N=16, S=2, seed=7)]


def _step_for(model, prob, cfg, use_graph, **kw):
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util.graphed_step import GraphedELBOStep
    x, y, fid = to_t(prob["x"]).to(DEV), to_t(prob["y"])[:, None].to(DEV), to_t(prob["fid"])[:, None].to(DEV)
    eps = [None] + [to_t(e).to(DEV) for e in prob["eps"][1:]]
    return GraphedELBOStep(model, VariationalELBOMF(model, cfg["N"], cfg["L"]), x, y, fid, lr=1e-2, use_graph=use_graph,
                           fixed_eps=eps, **kw)


NG = dict(variational_optimizer="natgrad", natgrad_gamma=0.1, natgrad_warmup_steps=0)


def _params(model):
    return [p.detach().cpu().clone() for p in model.parameters()]


@pytest.mark.parametrize("cfg", CFGS, ids=["small2d", "3layer", "3layer_seed7"])
def test_trajectory_matches_oracle_gradients_with_the_restatement(cfg):
    """Five steps, gamma = 0.1, no warm-up, Adam lr = 1e-2 on the rest: every step's -ELBO and every parameter at the end within
    100 gtol of the oracle's loss and autograd gradients + the restatement on (m, L_S) + torch.optim.Adam on the other leaves;
    the captured replay equals the eager run to the same tolerance.  The lower layers of these problems are far from conjugate
    (likelihood noise 1e-6 above them): in the three-layer problems I + 2 gamma Psi of a lower layer is clearly indefinite at some
    steps (smallest eigenvalue -34 / -964 at the first step of layer 0; -0.2 / -0.4 in layer 1 at steps 3 and 4 with seed 7), so
    the trajectory also exercises the skip rule: the restatement leaves such a layer alone, and the per-layer skip counts
    must agree."""
    prob = synthetic.make_problem(**cfg)
    S, L, N = cfg["S"], cfg["L"], cfg["N"]
    model = build_model(prob, S_train=S)
    model_g = copy.deepcopy(model)
    raw = _raw_from_model(model, L)
    x, y, fid = to_t(prob["x"]), to_t(prob["y"]), to_t(prob["fid"])
    eps = [None] + [to_t(e) for e in prob["eps"][1:]]
    variational = [lay[k] for lay in raw["layers"] for k in ("m", "L_S")]
    others = [p for p in O.flatten_raw(raw) if not any(p is v for v in variational)]
    opt_o = torch.optim.Adam(others, lr=1e-2)
    step_e, step_g = _step_for(model, prob, cfg, False, **NG), _step_for(model_g, prob, cfg, True, **NG)
    skipped_ref = [0] * L
    for k in range(5):
        for p in O.flatten_raw(raw):
            p.grad = None
        e_o, _ = O.elbo(O.state_from_raw(raw), x, y, fid, eps=eps, S=S)
        (-e_o).backward()
        with torch.no_grad():
            for li, lay in enumerate(raw["layers"]):
                m_new, L_new, _, ok = R.natgrad_update(lay["m"], lay["L_S"], lay["m"].grad, lay["L_S"].grad, 0.1)
                skipped_ref[li] += 0 if ok else 1      # (not ok: m and L_S come back unchanged)
                lay["L_S"].copy_(L_new + torch.triu(lay["L_S"], 1))
                lay["m"].copy_(m_new)
        opt_o.step()
        step_e.step()
        step_g.step()
        step_e.check()
        step_g.check()
        print("step %d: -ELBO oracle %.12g eager %.12g captured %.12g" % (k, -float(e_o.detach()), float(step_e.loss), float(step_g.loss)))
        assert rel(step_e.loss, -e_o) < 100 * GTOL and rel(step_g.loss, step_e.loss) < 100 * GTOL, k
        for l in range(L):      # every parameter after every step, and the skip counts so far
            for key, t in raw["layers"][l].items():
                p, pg = _model_param_for(model, l, key), _model_param_for(model_g, l, key)
                assert rel(p.reshape(t.shape), t.detach()) < 100 * GTOL, (k, l, key)
                assert rel(pg.reshape(t.shape), p.reshape(t.shape)) < 100 * GTOL, (k, l, key)
            for mdl in (model, model_g):
                noise = getattr(mdl, "hidden_layer_likelihood_%d" % l).raw_noise.reshape(())
                assert rel(noise, raw["raw_noise"][l].detach()) < 100 * GTOL, (k, l)
        assert step_e.skipped_steps() == skipped_ref and step_g.skipped_steps() == skipped_ref, k
    print("skipped per layer:", skipped_ref)
    step_e.close()
    step_g.close()


def test_frozen_covariance_and_the_adam_keyword_are_todays_adam_step_bitwise():
    """With fix_variational_hypers(True) no layer has both gradients: the 'natgrad' step IS today's Adam step, bitwise; and
    variational_optimizer='adam' is the default, bitwise."""
    cfg = CFGS[0]
    prob = synthetic.make_problem(**cfg)
    base = build_model(prob, S_train=cfg["S"])
    out = {}
    for name, fix, kw in (("default", False, {}), ("adam", False, dict(variational_optimizer="adam")),
                          ("default_fixed", True, {}), ("natgrad_fixed", True, NG)):
        model = copy.deepcopy(base)
        model.fix_variational_hypers(fix)
        step = _step_for(model, prob, cfg, True, **kw)
        for _ in range(3):
            step.step()
        step.check()
        out[name] = _params(model)
        step.close()
    for a, b in (("default", "adam"), ("default_fixed", "natgrad_fixed")):
        assert all(torch.equal(p, q) for p, q in zip(out[a], out[b])), (a, b)
    assert not all(torch.equal(p, q) for p, q in zip(out["default"], out["default_fixed"]))


# ------------------------------------------------------------------ 8. mini-batch and conditioned steps
@pytest.mark.parametrize("B", [16, 20], ids=["even_batches", "ragged_last_batch"])
def test_minibatch_step_with_natural_gradients(B):
    """N = 48: three steps (B = 16: one batch shape; B = 20: the full and the ragged shape).  Finite loss, nothing skipped, the
    captured run equals the eager one, and a rollback restores gamma's counter."""
    from mobocmf_amd import functional as F
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util.graphed_step import GraphedMiniBatchStep
    cfg = dict(d=2, L=2, M=8, N=48, S=3, seed=0)
    prob = synthetic.make_problem(**cfg)
    x, y, fid = to_t(prob["x"]).to(DEV), to_t(prob["y"])[:, None].to(DEV), to_t(prob["fid"])[:, None].to(DEV)
    eps = [None] + [to_t(e[:B * cfg["S"]].copy()).to(DEV) for e in prob["eps"][1:]]
    res = {}
    for use_graph in (False, True):
        model = synthetic.model_from_problem(prob, num_samples_for_training=cfg["S"], device=DEV)
        step = GraphedMiniBatchStep(model, VariationalELBOMF(model, 48, 2), x, y, fid, B, lr=1e-2, use_graph=use_graph,
                                    fixed_eps=eps, sampler_state=F.minibatch_state(77, DEV), variational_optimizer="natgrad",
                                    natgrad_gamma=0.1, natgrad_gamma_init=1e-3, natgrad_warmup_steps=10)
        losses = []
        for k in range(3):
            if k == 2:
                step.snapshot()
                before = _params(model)
            step.step()
            step.check()
            losses.append(float(step.loss))
        assert all(l == l and abs(l) < float("inf") for l in losses)
        assert step.skipped_steps() == [0, 0] and int(step.optimizer.natgrad_steps[0]) == 3
        res[use_graph] = (losses, _params(model))
        if use_graph:
            step.restore_and_go_eager()
            assert int(step.optimizer.natgrad_steps[0]) == 2 and all(torch.equal(p, q) for p, q in zip(_params(model), before))
            step.step()      # the same batch again, eagerly, with the same gamma_t: the third step once more
            step.check()
            assert int(step.optimizer.natgrad_steps[0]) == 3
            assert all(rel(p, q) < 100 * GTOL for p, q in zip(_params(model), res[True][1]))
        step.close()
    assert all(abs(a - b) <= 100 * GTOL * abs(a) for a, b in zip(*[res[g][0] for g in (False, True)]))
    assert all(rel(p, q) < 100 * GTOL for p, q in zip(res[True][1], res[False][1]))


def test_conditioned_step_with_natural_gradients():
    """Two black-boxes (an objective and a constraint), M = N = 12, an injected Pareto set, the layer path: three iterations,
    captured against eager; the four layers are one call of the update."""
    from mobocmf_amd.util.graphed_step import GraphedConditionedStep
    from tests.test_hip_conditioned import _fitter
    g = torch.Generator().manual_seed(2)
    ps, pf = torch.rand(5, 2, dtype=torch.float64, generator=g), torch.randn(5, 1, dtype=torch.float64, generator=g) * 0.3
    xt = torch.rand(10, 2, dtype=torch.float64, generator=g).to(DEV)
    res = {}
    for use_graph in (False, True):
        fitter, _ = _fitter(1, 1, 12, 12)
        fitter.set_pareto_solution(ps, pf)
        for _, _, h in fitter._handlers():
            h.mfdgp.fix_variational_hypers_cond(True)
        torch.manual_seed(0)            # layer-1 eps of both runs: drawn from the device generator
        step = GraphedConditionedStep(fitter, lr=5e-3, use_graph=use_graph, fixed_x_tilde=xt, variational_optimizer="natgrad",
                                      natgrad_gamma=0.05, natgrad_gamma_init=1e-3, natgrad_warmup_steps=10)
        models = [h.mfdgp for _, _, h in fitter._handlers()]
        losses = []
        for k in range(3):
            if k == 2:
                step.snapshot()
            step.step()
            step.check()
            losses.append(float(step.loss))
        assert all(l == l and abs(l) < float("inf") for l in losses)
        assert step.skipped_steps() == [0] * 4 and int(step.optimizer.natgrad_steps[0]) == 3
        res[use_graph] = (losses, [p for m in models for p in _params(m)])
        if use_graph:
            step.restore_and_go_eager()
            assert int(step.optimizer.natgrad_steps[0]) == 2
        step.close()
    assert all(abs(a - b) <= 100 * GTOL * abs(a) for a, b in zip(*[res[g][0] for g in (False, True)]))
    assert all(rel(p, q) < 100 * GTOL for p, q in zip(res[True][1], res[False][1]))


# ------------------------------------------------------------------ 9. through the fitter
def test_fitter_trains_with_natural_gradients_on_the_layer_path(monkeypatch):
    """BlackBoxMFDGPFitter(variational_optimizer="natgrad") on surrogates small enough for the one-launch steps: both training
    phases and the conditioned fit take the layer path's captured steps with the fitter's gamma settings, no one-launch step is
    built, L_S stays put while it is frozen (first phase: Adam alone) and (m, L_S) move afterwards."""
    import numpy as np
    from mobocmf_amd.util import coop_step, graphed_step, tiny_step
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    rng = np.random.default_rng(0)
    N = 24
    x = torch.tensor(rng.random((N, 2)))
    fid = torch.tensor((np.arange(N) % 4 == 0).astype(np.float64))[:, None]
    fitter = BlackBoxMFDGPFitter(2, N, num_epochs_1=2, num_epochs_2=3, device=DEV, num_inducing=12, variational_optimizer="natgrad",
                                 natgrad_gamma=0.05, natgrad_gamma_init=1e-3, natgrad_warmup_steps=10)
    fitter.verbose = False
    for k in range(2):
        y = torch.sin(3.0 * x[:, :1] + k) + 0.3 * (k + 1) * x[:, 1:] * fid
        fitter.initialize_mfdgp(x, y, fid, "f%d" % k, is_constraint=(k == 1))
    built = []
    for cls in (graphed_step.GraphedELBOStep, graphed_step.GraphedConditionedStep):
        def init(self, *a, _orig=cls.__init__, _name=cls.__name__, **kw):
            built.append((_name, {k: v for k, v in kw.items() if k.startswith(("variational", "natgrad"))}))
            _orig(self, *a, **kw)
        monkeypatch.setattr(cls, "__init__", init)
    for cls in (tiny_step.TinyELBOStep, coop_step.CoopELBOStep, tiny_step.TinyConditionedStep, coop_step.CoopConditionedStep):
        def refuse(self, *a, _name=cls.__name__, **kw):
            raise AssertionError("%s built although variational_optimizer='natgrad'" % _name)
        monkeypatch.setattr(cls, "__init__", refuse)
    models = [h.mfdgp for _, _, h in fitter._handlers()]
    state = lambda: [(_vd(m, l).variational_mean.detach().clone(), _vd(m, l).chol_variational_covar.detach().clone())
                     for m in models for l in range(2)]
    s0 = state()
    fitter._train_mfdgp_graphed(True, fitter.num_epochs_1, fitter.lr_1)
    s1 = state()
    assert all(torch.equal(a[1], b[1]) and not torch.equal(a[0], b[0]) for a, b in zip(s0, s1))      # L_S frozen, m by Adam
    fitter._train_mfdgp_graphed(False, fitter.num_epochs_2, fitter.lr_2)
    s2 = state()
    assert all(not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) for a, b in zip(s1, s2))
    want = dict(variational_optimizer="natgrad", natgrad_gamma=0.05, natgrad_gamma_init=1e-3, natgrad_warmup_steps=10)
    assert built == [("GraphedELBOStep", want)] * 4
    g = torch.Generator().manual_seed(2)
    fitter.models_uncond_trained = True
    fitter.set_pareto_solution(torch.rand(5, 2, dtype=torch.float64, generator=g),
                               torch.randn(5, 1, dtype=torch.float64, generator=g) * 0.3)
    fitter.train_conditioned_mfdgps(num_iters=3)
    s3 = state()
    assert built[4:] == [("GraphedConditionedStep", want)]
    assert all(not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) for a, b in zip(s2, s3))
    assert all(bool(torch.isfinite(t).all()) for pair in s3 for t in pair)
