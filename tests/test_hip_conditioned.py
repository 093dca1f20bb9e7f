"""the conditioned-training loss (ELBO on the data + ELBO data term on the Pareto pseudo-observations
+ theta factors + omega factors, blackbox_mfdgp_fitter.py:227-343) on the HIP path vs the oracle."""
import numpy as np
import pytest
import torch

from mobocmf_amd.util import synthetic
from oracle import mfdgp_oracle as O
from tests.helpers import oracle_state, to_t

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _fitter(n_obj=2, n_con=1, N=12, M=8, d=2):
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter, MFDGPHandler
    from torch.utils.data import TensorDataset
    fitter = BlackBoxMFDGPFitter(2, N, device=DEV)
    fitter.verbose = False
    probs = []
    for o in range(n_obj + n_con):
        prob = synthetic.make_problem(d=d, L=2, M=M, N=N, S=1, output=o, seed=o)
        prob["noise"] = [np.array(1e-2), np.array(2e-2)]          # benign noise: well-scaled losses
        probs.append(prob)
        model = synthetic.model_from_problem(prob, num_samples_for_training=1, device=DEV)
        h = MFDGPHandler.__new__(MFDGPHandler)
        h.mfdgp, h.num_data, h.num_fidelities, h.batch_size = model, N, 2, N
        h.elbo = VariationalELBOMF(model, N, 2)
        t = lambda a: to_t(a).to(DEV)
        h.train_dataset = TensorDataset(t(prob["x"]), t(prob["y"])[:, None], t(prob["fid"])[:, None])
        h.iter_train_loader = None
        (fitter.mfdgp_handlers_objs if o < n_obj else fitter.mfdgp_handlers_cons)["bb%d" % o] = h
    fitter.num_obj, fitter.num_con = n_obj, n_con
    fitter.thresholds_cons = torch.tensor([0.1] * n_con, dtype=torch.float64)
    return fitter, probs


def test_conditioned_loss_and_gradients_match_oracle():
    n_obj, n_con, N, P, T, d = 2, 1, 12, 5, 10, 2
    fitter, probs = _fitter(n_obj, n_con, N)
    g = torch.Generator().manual_seed(0)
    pareto_set = torch.rand(P, d, dtype=torch.float64, generator=g)
    pareto_front = torch.randn(P, n_obj, dtype=torch.float64, generator=g) * 0.5
    x_tilde = torch.rand(T, d, dtype=torch.float64, generator=g)
    fitter.set_pareto_solution(pareto_set, pareto_front)
    eps_all = {}
    objs, cons = [], []
    for idx, (tag, i, h) in enumerate(fitter._handlers()):
        e = torch.randn(N + P + T, dtype=torch.float64, generator=g)
        eps_all[(tag, i)] = [None, e.to(DEV)]
        st = oracle_state(probs[idx], requires_grad=True)
        rec = {"state": st, "x": to_t(probs[idx]["x"]), "y": to_t(probs[idx]["y"]), "fid": to_t(probs[idx]["fid"]),
               "eps_batch": [None, e[:N]], "eps_pareto": [None, e[N:N + P]], "eps_tilde": [None, e[N + P:]]}
        (objs if tag == "OBJ" else cons).append(rec)
    loss_o = O.conditioned_loss(objs, cons, pareto_set, pareto_front, x_tilde, fitter.thresholds_cons, fitter.eps)
    loss_o.backward()
    loss = fitter.conditioned_loss(x_tilde.to(DEV), eps=eps_all)
    loss.backward()
    assert abs(float(loss) - float(loss_o)) / abs(float(loss_o)) < 1e-8
    for rec, (tag, i, h) in zip(objs + cons, fitter._handlers()):
        for l in range(2):
            vd = getattr(h.mfdgp, f"hidden_layer_{l}").variational_strategy._variational_distribution
            ref = rec["state"]["layers"][l]["m"].grad
            err = float((vd.variational_mean.grad.cpu() - ref).abs().max() / ref.abs().max())
            assert err < 1e-6, (tag, i, l, err)
            refL = torch.tril(rec["state"]["layers"][l]["L_S"].grad)
            errL = float((vd.chol_variational_covar.grad.cpu() - refL).abs().max() / refL.abs().max())
            assert errL < 1e-6, (tag, i, l, errL)


def test_conditioned_training_runs_and_reduces_the_loss():
    fitter, _ = _fitter(2, 1, 12)
    g = torch.Generator().manual_seed(1)
    fitter.set_pareto_solution(torch.rand(5, 2, dtype=torch.float64, generator=g),
                               torch.randn(5, 2, dtype=torch.float64, generator=g) * 0.3)
    xt = torch.rand(10, 2, dtype=torch.float64, generator=g).to(DEV)
    torch.manual_seed(0)
    l0 = float(fitter.conditioned_loss(xt))
    fitter.lr_2 = 5e-3
    fitter.train_conditioned_mfdgps(num_iters=60)
    torch.manual_seed(0)
    l1 = float(fitter.conditioned_loss(xt))
    assert np.isfinite(l1) and l1 < l0
    # kernel hyper-parameters stay frozen in conditioned training (fix_variational_hypers_cond)
    for _, _, h in fitter._handlers():
        assert not any(p.requires_grad for p in h.mfdgp.hidden_layer_1.covar_module.parameters())
    fc = fitter.copy_uncond()
    assert fc.pareto_set is not fitter.pareto_set


def _conditioned_fitter_with_a_failing_verdict(monkeypatch, cls):
    """A fitter ready for conditioned training whose second verdict through ``cls.check`` fails -- on the host: the exception is
    injected, nothing is faulted on the device -- and the GraphedConditionedStep objects that training constructs."""
    from mobocmf_amd.layers.mfdgp_hidden_layer import NotPSDError
    from mobocmf_amd.util import blackbox_mfdgp_fitter as BF
    from mobocmf_amd.util import graphed_step
    monkeypatch.setattr(BF, "ITER_PRINT", 4)
    fitter, _ = _fitter(2, 1, 12)
    g = torch.Generator().manual_seed(1)
    fitter.set_pareto_solution(torch.rand(5, 2, dtype=torch.float64, generator=g),
                               torch.randn(5, 2, dtype=torch.float64, generator=g) * 0.3)
    fitter.lr_2 = 5e-3
    calls = {"n": 0}
    real_check = cls.check

    def failing_check(self):
        calls["n"] += 1
        if calls["n"] == 2:      # the verdict at iteration 4 (iteration 0 passed)
            raise NotPSDError("injected")
        return real_check(self)

    monkeypatch.setattr(cls, "check", failing_check)
    made = []
    real_init = graphed_step.GraphedConditionedStep.__init__
    monkeypatch.setattr(graphed_step.GraphedConditionedStep, "__init__",
                        lambda self, *a, **k: (real_init(self, *a, **k), made.append(self))[0])
    return fitter, made


def test_captured_conditioned_training_redoes_the_iterations_after_a_failed_verdict(monkeypatch):
    import warnings
    from mobocmf_amd.util.graphed_step import GraphedConditionedStep
    fitter, made = _conditioned_fitter_with_a_failing_verdict(monkeypatch, GraphedConditionedStep)
    fitter.use_tiny_step = False                               # the captured iteration from the start
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        fitter.train_conditioned_mfdgps(num_iters=10)
    assert any("conditioned training: injected -- rolling back 4 iterations and redoing them eagerly" in str(m.message) for m in w)
    step, = made
    assert step.use_graph and int(step.optimizer.steps_done) == 10
    for _, _, h in fitter._handlers():
        assert all(bool(torch.isfinite(p).all()) for p in h.mfdgp.parameters())
        assert h.iter_train_loader is None


def test_one_launch_conditioned_training_hands_over_to_the_layer_path_after_a_failed_verdict(monkeypatch):
    import warnings
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    from mobocmf_amd.util.tiny_step import TinyELBOStep
    fitter, made = _conditioned_fitter_with_a_failing_verdict(monkeypatch, TinyELBOStep)
    handed = []
    real_tiny = BlackBoxMFDGPFitter._train_conditioned_tiny
    monkeypatch.setattr(BlackBoxMFDGPFitter, "_train_conditioned_tiny",
                        lambda self, n: (handed.append(real_tiny(self, n)), handed[-1])[1])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        fitter.train_conditioned_mfdgps(num_iters=10)
    assert any("conditioned training: injected -- rolling back 4 iterations; the layer path continues" in str(m.message) for m in w)
    (done, tiny), = handed
    assert done == 1 < 10 and tiny is not None                # iteration 0 stands
    step, = made                                              # the layer path took over ...
    assert int(step.optimizer.steps_done) == 10               # ... with the step count (1 + 9 of its own) and the moments
    assert sum(float(st["exp_avg_sq"].abs().sum()) for st in step.optimizer.state.values() if "exp_avg_sq" in st) > 0
    for _, _, h in fitter._handlers():
        assert all(bool(torch.isfinite(p).all()) for p in h.mfdgp.parameters())


def test_graphed_conditioned_step_equals_eager():
    """HIP-graph replay of the joint conditioned iteration == the eager iteration (same x~ every step)."""
    from mobocmf_amd.util.graphed_step import GraphedConditionedStep
    g = torch.Generator().manual_seed(2)
    ps, pf = torch.rand(5, 2, dtype=torch.float64, generator=g), torch.randn(5, 2, dtype=torch.float64, generator=g) * 0.3
    xt = torch.rand(10, 2, dtype=torch.float64, generator=g).to(DEV)
    traj = []
    for use_graph in (False, True):
        fitter, _ = _fitter(2, 1, 12)
        fitter.set_pareto_solution(ps, pf)
        for _, _, h in fitter._handlers():
            h.mfdgp.fix_variational_hypers_cond(True)
        torch.manual_seed(0)            # layer-1 eps of both runs: drawn from the device generator
        step = GraphedConditionedStep(fitter, lr=5e-3, use_graph=use_graph, fixed_x_tilde=xt)
        ls = []
        for _ in range(6):
            step.step()
            step.stream.synchronize()
            ls.append(float(step.loss))
        step.check()
        traj.append(ls)
    # eps is drawn inside the layers' propagation launches from (seed, call counter): the seeds of both runs come from the
    # same torch.manual_seed state and the captured step's warm-up draws are rolled back, so the replayed trajectory IS the
    # eager one
    assert all(np.isfinite(v) for v in traj[0] + traj[1])
    assert traj[0][-1] < traj[0][0] and traj[1][-1] < traj[1][0]
    for a, b in zip(*traj):
        assert abs(a - b) < 1e-9 * abs(a), (traj[0], traj[1])


def test_jesmoc_next_point_flow():
    """The reference's acquisition flow (JESMOC_MFDGP.__init__ :57-98, add_blackbox :101-116, coupled_acq :125-135,
    get_nextpoint_coupled :151-184) on the mirrored classes; the coupled value equals the sum of the per-black-box
    oracle JES values, and the optimiser returns a point inside the bounds that is at least as good as a random one."""
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP
    fitter, probs = _fitter(2, 1, 12)
    g = torch.Generator().manual_seed(3)
    fitter.set_pareto_solution(torch.rand(5, 2, dtype=torch.float64, generator=g),
                               torch.randn(5, 2, dtype=torch.float64, generator=g) * 0.3)
    fitter.lr_2, fitter.num_epochs_2 = 5e-3, 40
    acq = JESMOC_MFDGP(fitter, num_fidelities=2,
                       standard_bounds=torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device=DEV))
    for f in range(2):
        acq.add_blackbox(f, "bb0", cost_evaluation=1.0 if f == 0 else 10.0)
        acq.add_blackbox(f, "bb1", cost_evaluation=1.0 if f == 0 else 10.0)
        acq.add_blackbox(f, "bb2", cost_evaluation=1.0 if f == 0 else 10.0, is_constraint=True)
    X = torch.rand(7, 2, dtype=torch.float64, generator=g).to(DEV)
    total = acq.coupled_acq(X, fidelity=1)
    parts = [acq.decoupled_acq(X, 1, n, is_constraint=(n == "bb2")) for n in ("bb0", "bb1", "bb2")]
    assert torch.allclose(total, sum(parts))
    assert (total >= 0).all()
    # oracle value of one black-box
    from tests.test_hip_model import _raw_from_model
    mu, mc = acq.objectives[1]["bb0"].mfdgp_uncond, acq.objectives[1]["bb0"].mfdgp_cond
    su = O.state_from_raw(_raw_from_model(mu, 2))
    sc = O.state_from_raw(_raw_from_model(mc, 2))
    su["samples"] = [None, mu.hidden_layer_1.samples.detach().cpu().double().reshape(-1)]
    sc["samples"] = [None, mc.hidden_layer_1.samples.detach().cpu().double().reshape(-1)]
    with torch.no_grad():
        ref = O.jes_acquisition(su, sc, X.cpu(), 1, mu.num_samples_for_acquisition)
    assert float((parts[0].detach().cpu() - ref).abs().max()) < 1e-6 * max(1.0, float(ref.abs().max()))
    x_next, fid = acq.get_nextpoint_coupled(maxiter=15)
    assert x_next.shape == (2,) and 0 <= fid < 2 and bool(((x_next >= 0) & (x_next <= 1)).all())


def test_minibatch_conditioned_loss_follows_the_loader_iterators():
    """batch_size < N: every model draws the next batch of ITS OWN shuffling loader per iteration, re-armed when it runs
    out (blackbox_mfdgp_fitter.py:281-285, :296-300), and the batch ELBO is rescaled by num_data / batch
    (:288, :303; KL inside scaled by batch / num_data).  Loss and gradients vs the oracle on the very batches drawn."""
    from torch.utils.data import DataLoader
    n_obj, n_con, N, B, P, T, d = 2, 1, 12, 5, 4, 10, 2
    fitter, probs = _fitter(n_obj, n_con, N)
    for _, _, h in fitter._handlers():
        h.batch_size = B
        h.train_loader = DataLoader(h.train_dataset, batch_size=B, shuffle=True)
    g = torch.Generator().manual_seed(7)
    pareto_set = torch.rand(P, d, dtype=torch.float64, generator=g)
    pareto_front = torch.randn(P, n_obj, dtype=torch.float64, generator=g) * 0.5
    fitter.set_pareto_solution(pareto_set, pareto_front)
    seen = {k: [] for k in range(n_obj + n_con)}
    for it in range(4):                   # 12 rows in batches of 5, 5, 2: the 4th draw re-arms the loader
        x_tilde = torch.rand(T, d, dtype=torch.float64, generator=g)
        torch.manual_seed(100 + it)
        batches = {(tag, i): fitter.next_conditioned_batch(h) for tag, i, h in fitter._handlers()}
        eps_all, objs, cons = {}, [], []
        for idx, (tag, i, h) in enumerate(fitter._handlers()):
            xb, yb, fb = batches[(tag, i)]
            nb = xb.shape[0]
            seen[idx].append(nb)
            e = torch.randn(nb + P + T, dtype=torch.float64, generator=g)
            eps_all[(tag, i)] = [None, e.to(DEV)]
            st = oracle_state(probs[idx], requires_grad=True)
            rec = {"state": st, "x": xb.cpu(), "y": yb.cpu()[:, 0], "fid": fb.cpu()[:, 0], "num_data": N,
                   "eps_batch": [None, e[:nb]], "eps_pareto": [None, e[nb:nb + P]], "eps_tilde": [None, e[nb + P:]]}
            (objs if tag == "OBJ" else cons).append(rec)
        loss_o = O.conditioned_loss(objs, cons, pareto_set, pareto_front, x_tilde, fitter.thresholds_cons, fitter.eps)
        loss_o.backward()
        for _, _, h in fitter._handlers():
            for p in h.mfdgp.parameters():
                p.grad = None
        loss = fitter.conditioned_loss(x_tilde.to(DEV), eps=eps_all, batches=batches)
        loss.backward()
        assert abs(float(loss) - float(loss_o)) / abs(float(loss_o)) < 1e-8, it
        for rec, (tag, i, h) in zip(objs + cons, fitter._handlers()):
            for l in range(2):
                vd = getattr(h.mfdgp, f"hidden_layer_{l}").variational_strategy._variational_distribution
                ref = rec["state"]["layers"][l]["m"].grad
                assert float((vd.variational_mean.grad.cpu() - ref).abs().max() / ref.abs().max()) < 1e-6, (it, tag, i, l)
    assert all(v == [5, 5, 2, 5] for v in seen.values()), seen
    # the training driver: mini-batches run eagerly (a host-side loader cannot be captured), a request for graphs is refused
    with pytest.raises(ValueError):
        fitter.train_conditioned_mfdgps(num_iters=2, use_graphs=True)
    fitter.lr_2 = 5e-3
    fitter.train_conditioned_mfdgps(num_iters=5)
    assert all(h.iter_train_loader is None for _, _, h in fitter._handlers())
