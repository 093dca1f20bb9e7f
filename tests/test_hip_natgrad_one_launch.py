"""Natural gradients for q(u) through the one-launch steps (TinyELBOStep / CoopELBOStep and their conditioned forms with
variational_optimizer="natgrad": the step's launch with the trainable bits of (m, L_S) cleared, then ONE launch of
mobocmf_natgrad_small_step for all layers): the conjugate known answer, the trajectory against the layer path's natural-gradient
step, the frozen case, the conditioned iteration, the fitter's opt-in and the hand-over of the gamma schedule."""
import copy

import pytest
import torch

from mobocmf_amd.util import synthetic
from oracle import mfdgp_oracle as O
from tests import natgrad_reference as R
from tests.helpers import to_t
from tests.test_hip_model import build_model, rel
from tests.test_hip_natgrad_model import CFGS, GTOL, NG, _m_S, _params, _step_for, _vd

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = ["small2d", "3layer", "3layer_seed7"]


def _classes():
    from mobocmf_amd.util.coop_step import CoopConditionedStep, CoopELBOStep
    from mobocmf_amd.util.tiny_step import TinyConditionedStep, TinyELBOStep
    return {"tiny": (TinyELBOStep, TinyConditionedStep), "coop": (CoopELBOStep, CoopConditionedStep)}


# ------------------------------------------------------------------ known answer
def conjugate_setup(M, N, seed=11):
    """One fidelity (one layer, kind 0), d = 2, Gaussian likelihood, as the fixture of test_hip_natgrad_model.py: a model on the
    CPU whose q(u) starts away from the prior with one negative diagonal entry, and the closed-form optimum from the model's own
    K_mm + 1e-6 I, K_mn and noise.  Returns (model, x, y, fid, m_opt, S_opt, the restatement's own relative error)."""
    from mobocmf_amd.models import MFDGP
    g = torch.Generator().manual_seed(seed)
    d = 2
    x = torch.rand(N, d, dtype=torch.float64, generator=g)
    y = (torch.sin(4.0 * x[:, :1]) + x[:, 1:] ** 2 + 0.05 * torch.randn(N, 1, dtype=torch.float64, generator=g))
    fid = torch.zeros(N, 1, dtype=torch.float64)
    torch.manual_seed(3)
    model = MFDGP(x, y, fid, num_fidelities=1, num_inducing=M)
    model.double()
    with torch.no_grad():
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
    m_opt, S_opt, _ = R.conjugate_optimum(Kmm, Kmn, y[:, 0], noise)
    m0, L0 = vd.variational_mean.detach().double().clone(), vd.chol_variational_covar.detach().double().clone()
    m0g, L0g = m0.clone().requires_grad_(True), L0.clone().requires_grad_(True)
    R.conjugate_neg_elbo(m0g, L0g, Kmm, Kmn, knn, y[:, 0], noise).backward()
    m1, L1, _, ok = R.natgrad_update(m0, L0, m0g.grad, L0g.grad, 1.0)
    assert ok
    return model, x, y, fid, m_opt, S_opt, max(rel(L1 @ L1.T, S_opt), rel(m1, m_opt))


@pytest.mark.parametrize("kind,M,N", [("tiny", 12, 40), ("coop", 12, 40), ("coop", 40, 64)], ids=["tiny_M12", "coop_M12", "coop_M40"])
def test_one_step_of_length_one_is_the_conjugate_optimum(kind, M, N):
    """Fixed hyper-parameters (lr = 0), gamma = 1, no warm-up: ONE step() lands on the closed-form optimum within 1e-6, the
    tolerance of test_hip_natgrad_model.py; a second step stays there."""
    model, x, y, fid, m_opt, S_opt, own = conjugate_setup(M, N)
    model = copy.deepcopy(model).to(DEV)
    step = _classes()[kind][0]([model], [N], [x.to(DEV)], [y.to(DEV)], [fid.to(DEV)], lr=0.0, force=True,
                               variational_optimizer="natgrad", natgrad_gamma=1.0, natgrad_gamma_init=1.0, natgrad_warmup_steps=0)
    step.step()
    step.check()
    m1, S1 = _m_S(model)
    errs = (rel(S1, S_opt), rel(m1, m_opt))
    print("%s M %d: rel err S %.3e m %.3e (the restatement's own error %.3e)" % ((kind, M) + errs + (own,)))
    assert max(errs) < GTOL
    step.step()
    step.check()
    m2, S2 = _m_S(model)
    assert rel(S2, S1) < GTOL and rel(m2, m1) < GTOL
    assert step.skipped_steps() == [0] and step.natgrad_steps.tolist() == [2]
    step.close()


# ------------------------------------------------------------------ trajectory against the layer path
def _one_launch_step(kind, model, prob, cfg, **kw):
    x, y, fid = to_t(prob["x"]).to(DEV), to_t(prob["y"])[:, None].to(DEV), to_t(prob["fid"])[:, None].to(DEV)
    eps = [None] + [to_t(e).to(DEV) for e in prob["eps"][1:]]
    return _classes()[kind][0]([model], [cfg["N"]], [x], [y], [fid], lr=1e-2, fixed_eps=[eps], force=True, **kw)


@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_trajectory_matches_the_layer_path(cfg):
    """Five steps, gamma = 0.1, no warm-up, Adam lr = 1e-2 on the rest, the same fixed eps: TinyELBOStep and CoopELBOStep with
    "natgrad" against the eager GraphedELBOStep with "natgrad" (itself pinned to the oracle's gradients and the restatement):
    every step's loss and every parameter after every step within 100 gtol, and the same per-layer skip counts -- these
    problems do skip lower-layer steps (I + 2 gamma Psi indefinite), by design."""
    prob = synthetic.make_problem(**cfg)
    base = build_model(prob, S_train=cfg["S"])
    models = {k: copy.deepcopy(base) for k in ("layer", "tiny", "coop")}
    ref = _step_for(models["layer"], prob, cfg, False, **NG)
    steps = {k: _one_launch_step(k, models[k], prob, cfg, **NG) for k in ("tiny", "coop")}
    for k in range(5):
        ref.step()
        ref.check()
        want = _params(models["layer"])
        skipped = ref.skipped_steps()
        for kind, step in steps.items():
            step.step()
            step.check()
            print("step %d %s: -ELBO %.12g (layer path %.12g), skipped %s" % (k, kind, float(step.loss[0]), float(ref.loss),
                                                                              step.skipped_steps()))
            assert rel(step.loss[0], ref.loss) < 100 * GTOL, (k, kind)
            for j, (p, q) in enumerate(zip(_params(models[kind]), want)):
                assert rel(p, q) < 100 * GTOL, (k, kind, j, rel(p, q))
            assert step.skipped_steps() == skipped, (k, kind)
            assert step.skipped == skipped      # (what check() left for run_verified)
    print("skipped per layer:", skipped)
    ref.close()
    for step in steps.values():
        step.close()


@pytest.mark.parametrize("kind", ["tiny", "coop"])
def test_frozen_covariance_is_todays_step_bitwise(kind):
    """fix_variational_hypers(True): no layer has both gradients, so three "natgrad" steps ARE three default steps, bitwise."""
    cfg = CFGS[0]
    prob = synthetic.make_problem(**cfg)
    base = build_model(prob, S_train=cfg["S"])
    out = {}
    for name, kw in (("default", {}), ("natgrad", NG)):
        model = copy.deepcopy(base)
        model.fix_variational_hypers(True)
        step = _one_launch_step(kind, model, prob, cfg, **kw)
        for _ in range(3):
            step.step()
        step.check()
        out[name] = _params(model) + [step.losses.cpu().clone()]
        assert step.skipped_steps() == [0] * cfg["L"]
        step.close()
    assert all(torch.equal(p, q) for p, q in zip(out["default"], out["natgrad"]))


# ------------------------------------------------------------------ the conditioned iteration
def _conditioned_case():
    from tests.test_hip_conditioned import _fitter
    g = torch.Generator().manual_seed(2)
    ps, pf = torch.rand(5, 2, dtype=torch.float64, generator=g), torch.randn(5, 1, dtype=torch.float64, generator=g) * 0.3
    xt = torch.rand(10, 2, dtype=torch.float64, generator=g).to(DEV)
    fitter, _ = _fitter(1, 1, 12, 12)
    fitter.set_pareto_solution(ps, pf)
    ge = torch.Generator().manual_seed(5)
    eps_all = {}
    for tag, i, h in fitter._handlers():
        h.mfdgp.fix_variational_hypers_cond(True)
        eps_all[(tag, i)] = [None, torch.randn(12 + 5 + 10, dtype=torch.float64, generator=ge).to(DEV)]      # rows [batch | Pareto | x~]
    return fitter, xt, eps_all


CNG = dict(variational_optimizer="natgrad", natgrad_gamma=0.05, natgrad_gamma_init=1e-3, natgrad_warmup_steps=10)


@pytest.fixture(scope="module")
def conditioned_layer_path():
    """Three iterations of GraphedConditionedStep with "natgrad" on the case above, the loss evaluated with the fixed eps and the
    unshuffled batch: per iteration (loss, parameters).  Computed once."""
    from mobocmf_amd.util.graphed_step import GraphedConditionedStep
    fitter, xt, eps_all = _conditioned_case()
    batches = {(tag, i): h.train_dataset.tensors for tag, i, h in fitter._handlers()}
    plain = fitter.conditioned_loss
    fitter.conditioned_loss = lambda x_tilde: plain(x_tilde, eps=eps_all, batches=batches)
    step = GraphedConditionedStep(fitter, lr=5e-3, use_graph=False, fixed_x_tilde=xt, **CNG)
    hist = []
    for _ in range(3):
        step.step()
        step.check()
        hist.append((float(step.loss), [p for _, _, h in fitter._handlers() for p in _params(h.mfdgp)]))
    assert step.skipped_steps() == [0] * 4
    step.close()
    return hist


@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "uncaptured"])
@pytest.mark.parametrize("kind", ["tiny", "coop"])
def test_conditioned_iteration_matches_the_layer_path(conditioned_layer_path, kind, use_graph):
    """One objective and one constraint, M = N = 12, an injected Pareto set of 5, a fixed x~, three iterations: losses and
    parameters within 100 gtol of the layer path's natural-gradient iteration, nothing skipped; a snapshot before the third
    iteration + restore brings the parameters back bitwise and the gamma counters back to 2."""
    fitter, xt, eps_all = _conditioned_case()
    step = _classes()[kind][1](fitter, lr=5e-3, fixed_x_tilde=xt, fixed_eps=eps_all, **CNG)
    step.use_graph = use_graph
    models = [h.mfdgp for _, _, h in fitter._handlers()]
    for k, (loss_ref, params_ref) in enumerate(conditioned_layer_path):
        if k == 2:
            step.snapshot()
            step.stream.synchronize()
            before = [p for m in models for p in _params(m)]
        step.step()
        step.check()
        print("iteration %d %s: loss %.12g (layer path %.12g)" % (k, kind, float(step.loss), loss_ref))
        assert abs(float(step.loss) - loss_ref) <= 100 * GTOL * abs(loss_ref), k
        for j, (p, q) in enumerate(zip([p for m in models for p in _params(m)], params_ref)):
            assert rel(p, q) < 100 * GTOL, (k, j, rel(p, q))
    assert step.skipped_steps() == [0] * 4 and step.natgrad_steps.tolist() == [3] * 4
    step.restore()
    step.stream.synchronize()
    assert step.natgrad_steps.tolist() == [2] * 4
    assert all(torch.equal(p, q) for p, q in zip([p for m in models for p in _params(m)], before))
    step.close()


def test_captured_conditioned_iteration_above_64_kb_of_lds():
    """M = N = 100: the natural-gradient launch needs more dynamic LDS than a kernel gets by default (two packed triangles of 28
    tiles, 123 KB), and the captured iteration is the first to issue it.  Two replays equal two uncaptured iterations."""
    from tests.test_hip_conditioned import _fitter
    g = torch.Generator().manual_seed(2)
    ps, pf = torch.rand(5, 2, dtype=torch.float64, generator=g), torch.randn(5, 1, dtype=torch.float64, generator=g) * 0.3
    xt = torch.rand(10, 2, dtype=torch.float64, generator=g).to(DEV)
    res = {}
    for use_graph in (True, False):
        fitter, _ = _fitter(1, 1, 100, 100)
        fitter.set_pareto_solution(ps, pf)
        ge = torch.Generator().manual_seed(5)
        eps_all = {}
        for tag, i, h in fitter._handlers():
            h.mfdgp.fix_variational_hypers_cond(True)
            eps_all[(tag, i)] = [None, torch.randn(100 + 5 + 10, dtype=torch.float64, generator=ge).to(DEV)]
        step = _classes()["coop"][1](fitter, lr=5e-3, fixed_x_tilde=xt, fixed_eps=eps_all, **CNG)
        step.use_graph = use_graph
        before = [p for _, _, h in fitter._handlers() for p in _params(h.mfdgp)]
        losses = []
        for _ in range(2):
            step.step()
            step.check()
            losses.append(float(step.loss))
        assert step.natgrad_steps.tolist() == [2] * 4
        res[use_graph] = (losses, [p for _, _, h in fitter._handlers() for p in _params(h.mfdgp)], step.skipped_steps())
        assert sum(not torch.equal(p, q) for p, q in zip(res[use_graph][1], before)) >= 8      # (m, L_S) of the four layers moved
        step.close()
    print("losses captured %s uncaptured %s, skipped %s" % (res[True][0], res[False][0], res[True][2]))
    assert all(abs(a - b) <= 100 * GTOL * abs(b) for a, b in zip(res[True][0], res[False][0]))
    assert all(rel(p, q) < 100 * GTOL for p, q in zip(res[True][1], res[False][1])) and res[True][2] == res[False][2]


# ------------------------------------------------------------------ through the fitter
def test_fitter_takes_the_one_launch_steps_on_request(monkeypatch):
    """The setting of test_fitter_trains_with_natural_gradients_on_the_layer_path with natgrad_one_launch=True: both phases and the
    conditioned fit build one-launch step objects with the fitter's gamma settings, no GraphedELBOStep is built, L_S is bitwise
    fixed in phase 1 (frozen: Adam alone), (m, L_S) move afterwards, everything stays finite."""
    import numpy as np
    from mobocmf_amd.util import coop_step, graphed_step, tiny_step
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    rng = np.random.default_rng(0)
    N = 24
    x = torch.tensor(rng.random((N, 2)))
    fid = torch.tensor((np.arange(N) % 4 == 0).astype(np.float64))[:, None]
    fitter = BlackBoxMFDGPFitter(2, N, num_epochs_1=2, num_epochs_2=3, device=DEV, num_inducing=12, variational_optimizer="natgrad",
                                 natgrad_gamma=0.05, natgrad_gamma_init=1e-3, natgrad_warmup_steps=10, natgrad_one_launch=True)
    fitter.verbose = False
    for k in range(2):
        y = torch.sin(3.0 * x[:, :1] + k) + 0.3 * (k + 1) * x[:, 1:] * fid
        fitter.initialize_mfdgp(x, y, fid, "f%d" % k, is_constraint=(k == 1))
    built = []
    one_launch = (tiny_step.TinyELBOStep, coop_step.CoopELBOStep, tiny_step.TinyConditionedStep, coop_step.CoopConditionedStep)
    for cls in one_launch:
        def init(self, *a, _orig=cls.__init__, _cls=cls, **kw):
            if type(self) is _cls:      # (the conditioned classes call the plain class's constructor themselves)
                built.append((_cls.__name__, {k: v for k, v in kw.items() if k.startswith(("variational", "natgrad"))}))
            _orig(self, *a, **kw)
        monkeypatch.setattr(cls, "__init__", init)
    for cls in (graphed_step.GraphedELBOStep, graphed_step.GraphedConditionedStep):
        def refuse(self, *a, _name=cls.__name__, **kw):
            raise AssertionError("%s built although natgrad_one_launch=True" % _name)
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
    assert built == [("TinyELBOStep", want)] * 2
    g = torch.Generator().manual_seed(2)
    fitter.models_uncond_trained = True
    fitter.set_pareto_solution(torch.rand(5, 2, dtype=torch.float64, generator=g),
                               torch.randn(5, 1, dtype=torch.float64, generator=g) * 0.3)
    fitter.train_conditioned_mfdgps(num_iters=3)
    s3 = state()
    assert built[2:] == [("TinyConditionedStep", want)]
    assert all(not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) for a, b in zip(s2, s3))
    assert all(bool(torch.isfinite(t).all()) for pair in s3 for t in pair)


def test_export_adam_state_hands_the_gamma_schedule_over():
    """After three steps a FusedNatGradAdam that takes over (the layer path after a failed Cholesky) continues at t = 3."""
    from mobocmf_amd import functional as F
    cfg = CFGS[0]
    prob = synthetic.make_problem(**cfg)
    model = build_model(prob, S_train=cfg["S"])
    step = _one_launch_step("tiny", model, prob, cfg, **NG)
    for _ in range(3):
        step.step()
    step.check()
    opt = F.FusedNatGradAdam(model, lr=1e-2, gamma=0.1, warmup_steps=0)
    assert opt.natgrad_steps.tolist() == [0] * len(opt.groups)
    step.export_adam_state(0, opt)
    assert opt.natgrad_steps.tolist() == [3] * len(opt.groups) and int(opt.steps_done) == 3
    step.close()
