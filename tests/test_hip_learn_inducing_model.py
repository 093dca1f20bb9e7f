"""MFDGP(learn_inducing_locations=True) against the oracle: the gradient of -ELBO with respect to the ONE shared Z_x
(``model.inducing_inputs``) equals the oracle's autograd gradient of ``raw["Zx"]``, every other gradient keeps its gate, and
five Adam steps that move Z_x too stay on the oracle's trajectory -- on the configurations, the metric and the gates of
tests/test_hip_model.py::test_raw_parameter_grads_and_adam_trajectory, once on the whole-call path (check_pd on) and once
on the batched chains + panel path (set_check_pd(False)); plus one case whose top layer has whole inactive column blocks."""
import pytest
import torch

from mobocmf_amd.util import synthetic
from oracle import mfdgp_oracle as O
from tests.helpers import to_t
from tests.test_hip_model import _model_param_for, _raw_from_model, hip_elbo, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"

CFGS = [dict(d=2, L=2, M=8, N=12, S=3, seed=0), dict(d=3, L=3, M=10, N=16, S=2, seed=7), dict(d=4, L=2, M=40, N=150, S=1, seed=3),
        dict(d=2, L=2, M=128, N=512, S=8, seed=0),
        # rows come sorted by descending fidelity (synthetic.make_problem): N' = 600 at layer 1, columns 150.. get no upstream
        # gradient, so the 128-column blocks 2, 3 and 4 of the top layer's dK are never written
        dict(d=4, L=2, M=40, N=600, S=1, seed=3)]
IDS = ["small2d", "3layer", "S1_reference_semantics", "C2", "sorted_by_fidelity"]


def _raw_with_Zx(model, L):
    raw = _raw_from_model(model, L)
    raw["Zx"] = model.inducing_inputs.detach().cpu().double().clone().requires_grad_(True)
    return raw


@pytest.mark.parametrize("check_pd", [True, False], ids=["whole_call", "chains_and_panels"])
@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_inducing_input_gradient_and_adam_trajectory(cfg, check_pd):
    prob = synthetic.make_problem(**cfg)
    S, L = cfg["S"], cfg["L"]
    gtol = 1e-4 if cfg["M"] >= 128 else 1e-6       # C2: cond(K_mm) ~ 1e9 bounds both implementations (test_hip_model.py)
    model = synthetic.model_from_problem(prob, num_samples_for_training=S, device=DEV, learn_inducing_locations=True)
    model.set_check_pd(check_pd)
    assert all(layer.variational_strategy.Zx is model.inducing_inputs for layer in model._layers())
    raw = _raw_with_Zx(model, L)
    x, y, fid = to_t(prob["x"]), to_t(prob["y"]), to_t(prob["fid"])
    eps = [None] + [to_t(e) for e in prob["eps"][1:]]
    e_o, _ = O.elbo(O.state_from_raw(raw), x, y, fid, eps=eps, S=S)
    (-e_o).backward()
    (e, _), _ = hip_elbo(model, prob, S)
    (-e).backward()
    assert rel(e, e_o) < 1e-8
    gz = rel(model.inducing_inputs.grad, raw["Zx"].grad)
    print(f"{cfg} check_pd={check_pd}: |g_Zx - oracle| / max|oracle| = {gz:.2e} (gate {gtol:g})")
    assert gz < gtol, gz
    for l in range(L):
        for key, t in raw["layers"][l].items():
            p = _model_param_for(model, l, key)
            gref = t.grad if key != "L_S" else torch.tril(t.grad)
            assert rel(p.grad.reshape(gref.shape), gref) < gtol, (l, key)
        assert rel(getattr(model, f"hidden_layer_likelihood_{l}").raw_noise.grad.reshape(()), raw["raw_noise"][l].grad) < gtol
    # Adam trajectory: 5 steps with Z_x among the leaves, same eps every step
    leaves = O.flatten_raw(raw) + [raw["Zx"]]
    opt_o = torch.optim.Adam(leaves, lr=1e-2)
    opt_h = torch.optim.Adam(model.parameters(), lr=1e-2)
    for p in leaves:
        p.grad = None
    z0 = model.inducing_inputs.detach().clone()
    for k in range(5):
        lo, _ = O.elbo_step(raw, opt_o, x, y, fid, eps, S, ref_equiv=False)
        opt_h.zero_grad()
        (e, _), _ = hip_elbo(model, prob, S)
        (-e).backward()
        opt_h.step()
        assert rel(-e, lo) < 100 * gtol, k
    assert float((model.inducing_inputs.detach() - z0).abs().max()) > 1e-3       # five steps of lr = 1e-2: it moved
    assert rel(model.inducing_inputs, raw["Zx"].detach()) < 100 * gtol
    for l in range(L):
        for key, t in raw["layers"][l].items():
            assert rel(_model_param_for(model, l, key).reshape(t.shape), t.detach()) < 100 * gtol, (l, key)
