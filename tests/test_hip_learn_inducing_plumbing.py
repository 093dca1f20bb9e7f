"""Learnable inducing inputs through the training steps and every consumer of Z_x: captured against eager steps (full batch and
mini-batch), the natural-gradient optimiser's Adam group, what learning Z_x buys on the issue's four oracle cases, that every
reader of Z_x sees the trained values (layer path, one-launch predict groups, conditioned loss, RFF chain samples), the
parameter's identity through conversions and copies, and the refusals."""
import copy
import io

import numpy as np
import pytest
import torch

from mobocmf_amd.util import synthetic
from tests.helpers import to_t

pytestmark = pytest.mark.gpu
DEV = "cuda"
t = lambda a: to_t(a).to(DEV)


def _model(prob, learn, S=None, **kw):
    return synthetic.model_from_problem(prob, num_samples_for_training=S or prob["S"], device=DEV,
                                        **(dict(learn_inducing_locations=True) if learn else {}), **kw)


def _step(prob, model, use_graph=True, **kw):
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util.graphed_step import GraphedELBOStep
    elbo = VariationalELBOMF(model, prob["N"], prob["L"])
    return GraphedELBOStep(model, elbo, t(prob["x"]), t(prob["y"])[:, None], t(prob["fid"])[:, None], lr=1e-2, use_graph=use_graph,
                           fixed_eps=[None] + [t(e) for e in prob["eps"][1:]], **kw)


def test_graphed_step_equals_eager_step_with_learned_inducing_inputs():
    prob = synthetic.make_problem(d=3, L=2, M=20, N=60, S=2, seed=9)
    out = []
    for use_graph in (False, True):
        model = _model(prob, True)
        z0 = model.inducing_inputs.detach().clone()
        g = _step(prob, model, use_graph)
        assert (g.graph is not None) == use_graph
        ls = []
        for _ in range(6):
            l, _ = g.step()
            g.stream.synchronize()
            ls.append(float(l))
        g.check()
        assert float((model.inducing_inputs.detach() - z0).abs().max()) > 1e-3
        out.append((ls, model.inducing_inputs.detach().clone()))
    assert out[0][0] == out[1][0] and out[0][0][-1] < out[0][0][0]
    assert torch.equal(out[0][1], out[1][1])


def test_minibatch_step_equals_eager_step_with_learned_inducing_inputs():
    from mobocmf_amd import functional as F
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util.graphed_step import GraphedMiniBatchStep
    cfg, B = dict(d=3, L=2, M=20, N=60, S=2, seed=9), 25
    prob = synthetic.make_problem(**cfg)
    perm = np.random.default_rng(3).permutation(cfg["N"])
    out = []
    for use_graph in (False, True):
        model = _model(prob, True)
        eps = [None] + [t(e[:B * cfg["S"]].copy()) for e in prob["eps"][1:]]
        step = GraphedMiniBatchStep(model, VariationalELBOMF(model, cfg["N"], 2), t(prob["x"][perm]), t(prob["y"][perm])[:, None],
                                    t(prob["fid"][perm])[:, None], B, lr=1e-2, use_graph=use_graph, fixed_eps=eps,
                                    order_by_fidelity=True, sampler_state=F.minibatch_state(77, DEV))
        ls = []
        for _ in range(6):
            l, _ = step.step()
            step.stream.synchronize()
            ls.append(float(l))
        step.check()
        out.append((ls, model.inducing_inputs.detach().clone()))
        step.retire()
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])


def test_natgrad_optimizer_moves_the_inducing_inputs_with_adam():
    """Z_x belongs to the Adam group: Adam's first step moves every entry with a non-zero gradient by lr (|g| / (|g| + eps))."""
    prob = synthetic.make_problem(d=3, L=2, M=20, N=60, S=2, seed=9)
    ref = _model(prob, True)
    ref.set_check_pd(False)
    from tests.test_hip_model import hip_elbo
    (e, _), _ = hip_elbo(ref, prob, 2)
    (-e).backward()
    gz = ref.inducing_inputs.grad.clone()
    model = _model(prob, True)
    z0 = model.inducing_inputs.detach().clone()
    g = _step(prob, model, True, variational_optimizer="natgrad")
    g.step()
    g.stream.synchronize()
    g.check()
    dz = model.inducing_inputs.detach() - z0
    lr = 1e-2
    nz = gz != 0
    assert bool(nz.any()) and bool((dz[~nz] == 0).all())
    assert bool((torch.sign(dz[nz]) == -torch.sign(gz[nz])).all())
    want = lr * gz.abs() / (gz.abs() + 1e-8)
    assert float(((dz.abs() - want).abs()[nz] / lr).max()) < 1e-6


@pytest.mark.parametrize("cfg", [dict(d=2, L=2, M=8, N=96, seed=0), dict(d=2, L=2, M=8, N=96, seed=1),
                                 dict(d=3, L=2, M=16, N=128, seed=2), dict(d=4, L=2, M=12, N=150, seed=3)],
                         ids=lambda c: "d%d_M%d_N%d_seed%d" % (c["d"], c["M"], c["N"], c["seed"]))
def test_learned_inducing_inputs_reach_a_better_elbo_than_fixed_ones(cfg):
    """S = 1, fixed eps, lr = 1e-2, 300 captured steps: the float64 oracle's -ELBO with Z_x learned is 0.42 .. 0.73 of the
    fixed-Z value on these four cases, so a strict inequality needs no margin."""
    prob = synthetic.make_problem(S=1, **cfg)
    final = {}
    for learn in (False, True):
        g = _step(prob, _model(prob, learn), True)
        for _ in range(300):
            loss, _ = g.step()
        g.stream.synchronize()
        g.check()
        final[learn] = float(loss)
    print(f"{cfg}: -ELBO after 300 steps: fixed Z {final[False]:.6f}, learned Z {final[True]:.6f}, ratio {final[True] / final[False]:.3f}")
    assert final[True] < final[False]


def _trained_pair(M, S=3):
    """A: learned Z_x, 20 captured steps.  B: flag off, built on A's trained inducing inputs, every other parameter copied."""
    prob = synthetic.make_problem(d=2, L=2, M=M, N=3 * M, S=S, seed=4)
    A = _model(prob, True)
    g = _step(prob, A, True)
    for _ in range(20):
        g.step()
    g.stream.synchronize()
    g.check()
    A.set_check_pd(True)
    assert float((A.inducing_inputs.detach().cpu() - to_t(prob["Zx"])).abs().max()) > 1e-2
    B = _model(dict(prob, Zx=A.inducing_inputs.detach().cpu().numpy()), False)
    sa = A.state_dict()
    with torch.no_grad():
        for k, v in B.state_dict().items():
            if not k.endswith("_inducing_points"):
                v.copy_(sa[k])
    assert torch.equal(B.hidden_layer_0.variational_strategy.Zx, A.inducing_inputs.detach())
    assert torch.equal(B.hidden_layer_1.variational_strategy.Zx, A.inducing_inputs.detach())
    return prob, A, B


@pytest.mark.parametrize("M", [24, 48])
def test_every_reader_sees_the_trained_inducing_inputs(M):
    from mobocmf_amd.layers.rff import sample_chain_from_posterior
    from mobocmf_amd.util.coop_step import CoopPredictGroup
    from mobocmf_amd.util.tiny_step import TinyPredictGroup
    prob, A, B = _trained_pair(M)
    T, d = 7, 2
    X = torch.rand(T, d, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(DEV)
    for f in (0, 1):
        for m in (A, B):
            m.eval()
        (ma, va), (mb, vb) = A.predict_for_acquisition(X, f), B.predict_for_acquisition(X, f)
        for m in (A, B):
            m.train()
        assert torch.equal(ma, mb) and torch.equal(va, vb), f
    for cls in (CoopPredictGroup,) + ((TinyPredictGroup,) if M <= 32 else ()):
        assert cls.why_not(A, 1, T, d, speed_rule=False) is None, cls.why_not(A, 1, T, d, speed_rule=False)
        ga, gb = cls([A], 1, T, d), cls([B], 1, T, d)
        (ma, va), (mb, vb) = ga.acquisition_moments(X), gb.acquisition_moments(X)
        assert torch.equal(ma, mb) and torch.equal(va, vb), cls.__name__
    sa = sample_chain_from_posterior(A, nFeatures=40, generator=torch.Generator().manual_seed(5)).pack()
    sb = sample_chain_from_posterior(B, nFeatures=40, generator=torch.Generator().manual_seed(5)).pack()
    assert torch.equal(sa, sb)


def _cond_fitter(model, prob):
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter, MFDGPHandler
    from torch.utils.data import TensorDataset
    N = prob["N"]
    fitter = BlackBoxMFDGPFitter(2, N, device=DEV)
    fitter.verbose = False
    for o in range(3):      # two objectives and a constraint, each the same surrogate
        h = MFDGPHandler.__new__(MFDGPHandler)
        h.mfdgp, h.num_data, h.num_fidelities, h.batch_size = model, N, 2, N
        h.elbo = VariationalELBOMF(model, N, 2)
        h.train_dataset = TensorDataset(t(prob["x"]), t(prob["y"])[:, None], t(prob["fid"])[:, None])
        h.iter_train_loader = None
        (fitter.mfdgp_handlers_objs if o < 2 else fitter.mfdgp_handlers_cons)["bb%d" % o] = h
    fitter.num_obj, fitter.num_con = 2, 1
    fitter.thresholds_cons = torch.tensor([0.1], dtype=torch.float64)
    return fitter


def test_conditioned_loss_reads_the_trained_inducing_inputs():
    prob, A, B = _trained_pair(24, S=1)
    N, P, T = prob["N"], 5, 10
    g = torch.Generator().manual_seed(0)
    pareto_set = torch.rand(P, 2, dtype=torch.float64, generator=g)
    pareto_front = torch.randn(P, 2, dtype=torch.float64, generator=g) * 0.5
    x_tilde = torch.rand(T, 2, dtype=torch.float64, generator=g).to(DEV)
    eps = [torch.randn(N + P + T, dtype=torch.float64, generator=g).to(DEV) for _ in range(3)]
    losses = []
    for m in (A, B):
        fitter = _cond_fitter(m, prob)
        fitter.set_pareto_solution(pareto_set, pareto_front)
        eps_all = {(tag, i): [None, eps[k]] for k, (tag, i, _) in enumerate(fitter._handlers())}
        losses.append(float(fitter.conditioned_loss(x_tilde, eps=eps_all).detach()))
    assert losses[0] == losses[1] and np.isfinite(losses[0])
    # the conditioned fit keeps Z_x constant, as it keeps the kernel
    A.fix_variational_hypers_cond(True)
    assert not A.inducing_inputs.requires_grad
    A.fix_variational_hypers_cond(False)
    A.fix_variational_hypers(True)
    assert A.inducing_inputs.requires_grad
    A.fix_variational_hypers(False)
    assert A.inducing_inputs.requires_grad


def test_identity_and_invariants():
    import dill
    from mobocmf_amd.models import MFDGP
    prob = synthetic.make_problem(d=2, L=3, M=8, N=24, S=2, seed=1)
    off, on = _model(prob, False), _model(prob, True)      # model_from_problem: .double() then .to(DEV)

    def shared(m):
        return all(layer.variational_strategy.Zx is m.inducing_inputs for layer in m._layers())

    assert shared(on) and on.inducing_inputs.is_cuda and on.inducing_inputs.dtype == torch.float64
    assert shared(copy.deepcopy(on))
    buf = io.BytesIO()
    dill.dump(on, buf)
    assert shared(dill.loads(buf.getvalue()))
    assert sum(p is on.inducing_inputs for p in on.parameters()) == 1
    keys_on, keys_off = list(on.state_dict()), list(off.state_dict())
    assert keys_on.count("inducing_inputs") == 1 and sum(k.endswith("inducing_inputs") for k in keys_on) == 1
    assert "inducing_inputs" not in keys_off and not hasattr(off, "inducing_inputs")
    # layer 0's buffer of the same shape is gone (it IS the parameter now), under its own name and under the names the
    # layers above reach it by (previous_layer is a registered sub-module)
    assert set(keys_on) - set(keys_off) == {"inducing_inputs"}
    gone = set(keys_off) - set(keys_on)
    assert "hidden_layer_0.variational_strategy._inducing_points" in gone
    assert all(k.endswith("hidden_layer_0.variational_strategy._inducing_points") or
               k.endswith("previous_layer.variational_strategy._inducing_points") for k in gone)
    assert len(list(on.parameters())) == len(list(off.parameters())) + 1
    vs = on.hidden_layer_1.variational_strategy
    assert torch.equal(vs.inducing_points, torch.cat((on.inducing_inputs, vs.zf[:, None]), 1))
    assert on.hidden_layer_0.variational_strategy.inducing_points is on.inducing_inputs
    x, y, fid = to_t(prob["x"]), to_t(prob["y"])[:, None], to_t(prob["fid"])[:, None]
    with pytest.raises(ValueError):
        MFDGP(x, y, fid, num_fidelities=3, num_inducing=8, learn_inducing_locations=True, use_only_highest_fidelity=True)
    with pytest.raises(ValueError):
        MFDGP(x, y, fid, num_fidelities=3, num_inducing=8, learn_inducing_locations=True, warm_start="posterior",
              previously_trained_model=off)
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.parallel import RowShardedELBOStep
    with pytest.raises(ValueError):
        RowShardedELBOStep(on, VariationalELBOMF(on, 24, 3), t(prob["x"]), t(prob["y"])[:, None], t(prob["fid"])[:, None], lr=1e-2)
    # greedy-variance and first-rows initialisation both seed the parameter
    for sel in ("first", "greedy_variance"):
        m = MFDGP(x.to(DEV), y.to(DEV), fid.to(DEV), num_fidelities=3, num_inducing=6, inducing_selection=sel,
                  learn_inducing_locations=True)
        assert tuple(m.inducing_inputs.shape) == (6, 2) and m.inducing_inputs.requires_grad
        if sel == "first":
            assert torch.equal(m.inducing_inputs.detach().cpu().double(), x[:6])


def test_fitter_trains_forrester_with_learned_inducing_inputs():
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    x, y, fid = synthetic.forrester_problem(0)
    fitter = BlackBoxMFDGPFitter(2, 16, num_epochs_1=100, num_epochs_2=100, device=DEV, learn_inducing_locations=True,
                                 num_inducing=8)
    fitter.verbose = False
    assert not fitter._one_launch_allowed()
    fitter.initialize_mfdgp(to_t(x), to_t(y)[:, None], to_t(fid)[:, None], "obj1")
    h = fitter.mfdgp_handlers_objs["obj1"]
    z0 = h.mfdgp.inducing_inputs.detach().clone()
    xb, yb, fb = h.train_dataset.tensors
    e0 = h.elbo(h.mfdgp(xb), yb.T, fb)[0].item()
    fitter.train_mfdgps()
    e1 = h.elbo(h.mfdgp(xb), yb.T, fb)[0].item()
    assert e1 > e0 and float((h.mfdgp.inducing_inputs.detach() - z0).abs().max()) > 1e-3
    fc = fitter.copy_uncond()
    mc = fc.mfdgp_handlers_objs["obj1"].mfdgp
    assert mc is not h.mfdgp and all(l.variational_strategy.Zx is mc.inducing_inputs for l in mc._layers())
    assert torch.equal(mc.inducing_inputs, h.mfdgp.inducing_inputs)
    fitter.num_epochs_1 = fitter.num_epochs_2 = 10
    fitter.train_mfdgps(use_graphs=False)      # the eager loader moves Z_x too
    assert h.elbo(h.mfdgp(xb), yb.T, fb)[0].item() > e0
