"""The frozen-chain predict kernel (csrc/frozen_predict.hip) through PanelPredictGroup (util/panel_predict.py): moments and input
gradient of surrogates with 128 < M <= 512 against MFDGP.predict_for_acquisition through the layer entry points, the group's
freeze / thaw and reuse, the seeds' zeros, the variance floor, and the refusals.
(The componentwise gate of the kernel itself, on the chain state it reads: tests/test_hip_frozen_predict_conformance.py.)"""
import pytest
import torch

from mobocmf_amd import _lib
from mobocmf_amd.util import synthetic
from tests.test_hip_model import build_model, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"

# M, d, S, fidelity, T -- see the docstring of the test for why each is there
CASES = [dict(M=129, d=2, S=5, f=1, T=7), dict(M=160, d=1, S=25, f=1, T=5), dict(M=200, d=3, S=3, f=2, T=6),
         dict(M=256, d=2, S=4, f=0, T=20), dict(M=512, d=8, S=4, f=1, T=5), dict(M=130, d=2, S=2, f=1, T=1)]


def _bits(t):
    return t.detach().contiguous().view(torch.int64)


@pytest.mark.parametrize("c", CASES, ids=["M%d_d%d_S%d_f%d_T%d" % (c["M"], c["d"], c["S"], c["f"], c["T"]) for c in CASES])
def test_panel_predict_group_matches_predict_for_acquisition_and_its_input_gradient(c):
    """PanelPredictGroup -- MOBOCMF_STEP_FORWARD for the moments of three models, MOBOCMF_STEP_INPUT_GRADIENTS for d/dX -- against
    MFDGP.predict_for_acquisition through the layer entry points (pinned to the oracle in test_hip_model.py), with the
    weighted-sum construction of test_hip_coop_step.py and its tolerances for the same reference (d <= 3: cond(K_mm + 1e-6 I) ~
    1e9, either side carries cond * eps).  Shapes: M = 129 one row past the cooperative limit (127 padded rows; 35 columns
    straddle 16-column blocks and base rows); M = 160, T = 5, S = 25 the search's own, d = 1 the worst conditioning; M = 200
    three layers (two propagations); M = 256 fidelity 0 (no replicas), a multiple of 128; M = 512 the LDS limit; T = 1.
    Both sides read the same chain state: the differences observed on an MI355X are recorded in DESIGN.md 5.6.1."""
    from mobocmf_amd.util.panel_predict import PanelPredictGroup, fits_predict
    M, d, S, fidelity, T = c["M"], c["d"], c["S"], c["f"], c["T"]
    models = [build_model(synthetic.make_problem(d=d, L=max(2, fidelity + 1), M=M, N=M, S=S, seed=s), S_train=1, S_acq=S)
              for s in (1, 2, 3)]
    assert all(fits_predict(m, fidelity, T, d) for m in models)
    g = torch.Generator().manual_seed(3)
    X = torch.rand(T, d, dtype=torch.float64, generator=g).to(DEV)
    wm = torch.randn(len(models), T, dtype=torch.float64, generator=g).to(DEV)
    wv = torch.randn(len(models), T, dtype=torch.float64, generator=g).to(DEV)
    X2 = torch.rand(T, d, dtype=torch.float64, generator=g).to(DEV)

    def layer_path(Xq, grad):
        Xa = Xq.clone().requires_grad_(grad)
        ms, vs = [], []
        with torch.set_grad_enabled(grad):
            for m in models:
                m.eval()
                mu, v = m.predict_for_acquisition(Xa, fidelity)
                m.train()
                ms.append(mu), vs.append(v)
            ms, vs = torch.stack(ms), torch.stack(vs)
            if grad:
                ((ms * wm).sum() + (vs * wv).sum()).backward()
        return ms.detach(), vs.detach(), Xa.grad

    ref_m, ref_v, ref_g = layer_path(X, True)
    grp = PanelPredictGroup(models, fidelity, T, d)
    assert grp.moments.shape == (3, 2, T * (S if fidelity else 1)) and grp.gx.shape == (3, T, d) and grp.S == (S if fidelity else 1)

    def evaluate(group, Xq, grad=True):
        Xb = Xq.clone().requires_grad_(grad)
        mus, v = group.acquisition_moments(Xb)
        if grad:
            ((mus * wm).sum() + (v * wv).sum()).backward()
        return mus.detach(), v.detach(), Xb.grad

    mus, v, gX = evaluate(grp, X)
    hard = d <= 3
    errs = (rel(mus, ref_m), rel(v, ref_v), rel(gX, ref_g))
    print("panel predict", c, "relative differences (mean, var, d/dX):", errs)
    assert errs[0] < (1e-6 if hard else 1e-8) and errs[1] < (1e-5 if hard else 1e-7), errs
    assert errs[2] < (1e-4 if hard else 1e-6), errs
    assert not any(bool(w.any()) for w in grp.info_words)
    # a second evaluation at other points reuses the group
    m2, v2, g2 = evaluate(grp, X2)
    r2m, r2v, _ = layer_path(X2, False)
    assert rel(m2, r2m) < (1e-6 if hard else 1e-8) and rel(v2, r2v) < (1e-5 if hard else 1e-7)
    # two evaluations of the same X: the same bits (fixed summation order)
    m1, v1, g1 = evaluate(grp, X)
    assert torch.equal(_bits(m1), _bits(mus)) and torch.equal(_bits(v1), _bits(v)) and torch.equal(_bits(g1), _bits(gX))
    # inside freeze() ... thaw(): the chains are formed once, the results are the same bits
    grp.freeze()
    chains = grp._chains
    for Xq, want in ((X2, (m2, v2, g2)), (X, (mus, v, gX))):
        got = evaluate(grp, Xq)
        assert grp._chains is chains and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))
    grp.thaw()
    assert not grp._frozen and grp._chains is None
    # a group for values only: no seeds, no gx, the same moments
    vals = PanelPredictGroup(models, fidelity, T, d, want_gradients=False)
    assert vals.seeds is None and vals.gx is None
    mv, vv, _ = evaluate(vals, X, grad=False)
    assert torch.equal(_bits(mv), _bits(mus)) and torch.equal(_bits(vv), _bits(v))
    with pytest.raises(_lib.MobocmfError):
        vals._launch(_lib.STEP_INPUT_GRADIENTS)


def test_zero_seeds_give_exactly_zero_input_gradients():
    """STEP_INPUT_GRADIENTS with seeds that are zero on a whole model, on single test points and on single columns: gx is exactly
    zero for the model and for the test points all of whose columns carry no seed."""
    from mobocmf_amd.util.panel_predict import PanelPredictGroup
    M, d, S, T = 140, 2, 3, 6
    models = [build_model(synthetic.make_problem(d=d, L=2, M=M, N=M, S=S, seed=s), S_train=1, S_acq=S) for s in (4, 5)]
    grp = PanelPredictGroup(models, 1, T, d)
    g = torch.Generator().manual_seed(0)
    grp.x.copy_(torch.rand(T, d, dtype=torch.float64, generator=g))
    seeds = torch.randn(2, 2, T * S, dtype=torch.float64, generator=g).to(DEV)
    seeds[0] = 0.0                                 # model 0: nothing
    seeds[1, :, 2 * S:3 * S] = 0.0                 # model 1: test point 2 nothing ...
    seeds[1, :, 4 * S + 1] = 0.0                   # ... and one column of test point 4
    grp.seeds.copy_(seeds)
    grp.gx.fill_(float("nan"))
    grp._launch(_lib.STEP_INPUT_GRADIENTS)
    gx = grp.gx.cpu()
    assert bool((gx[0] == 0.0).all()) and bool((gx[1, 2] == 0.0).all())
    rest = torch.tensor([0, 1, 3, 4, 5])
    assert bool(torch.isfinite(gx[1]).all()) and bool((gx[1, rest] != 0.0).all())


def test_a_column_at_the_variance_floor_passes_no_variance_gradient():
    """A test point equal to an inducing input of a model with a tiny L_S (1e-7 I) and a tiny jitter (1e-12; d = 8 keeps K_mm well
    conditioned): k_nn - |A|^2 + |C|^2 ~ 1e-12 is under the floor.  The layer path hits the floor there (asserted first); the
    kernel reports the floor, and a variance-only seed yields exactly zero gx at that point but not at the others."""
    from mobocmf_amd.util.panel_predict import PanelPredictGroup
    M, d, T = 130, 8, 3
    model = build_model(synthetic.make_problem(d=d, L=2, M=M, N=M, S=2, seed=9), S_train=1, S_acq=2)
    layer = model.hidden_layer_0
    with torch.no_grad():
        layer.variational_strategy._variational_distribution.chol_variational_covar.copy_(1e-7 * torch.eye(M, dtype=torch.float64))
    layer.variational_strategy.jitter_val = 1e-12
    Z = layer.variational_strategy._inducing_points.detach()
    X = torch.rand(T, d, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).to(DEV)
    X[1] = Z[7]
    model.eval()
    with torch.no_grad():
        var_ref = layer(X).variance.reshape(-1)
    model.train()
    assert float(var_ref[1]) == 1e-10 and float(var_ref[0]) > 1e-10 and float(var_ref[2]) > 1e-10      # the precondition
    grp = PanelPredictGroup([model], 0, T, d)
    grp.x.copy_(X)
    grp.seeds.zero_()
    grp.seeds[0, 1] = 1.0                          # variance seeds only
    grp._launch(_lib.STEP_INPUT_GRADIENTS)
    var, gx = grp.moments[0, 1].cpu(), grp.gx[0].cpu()
    assert float(var[1]) == 1e-10 and rel(var, var_ref) < 1e-7
    assert bool((gx[1] == 0.0).all()) and bool(gx[0].any()) and bool(gx[2].any())
    grp.seeds[0, 0] = 1.0                          # with a mean seed the point moves again
    grp._launch(_lib.STEP_INPUT_GRADIENTS)
    assert bool(grp.gx[0, 1].any())


def test_refusals_name_the_reason_and_launch_nothing():
    from mobocmf_amd.util import panel_predict as PP
    cases = [(dict(M=128, d=2, S=3), "M = 128"), (dict(M=513, d=2, S=3), "M = 513"), (dict(M=130, d=2, S=1), "S = 1"),
             (dict(M=130, d=9, S=3), "d = 9")]
    for kw, word in cases:
        model = build_model(synthetic.make_problem(L=2, N=kw["M"], seed=0, **kw), S_train=1, S_acq=kw["S"])
        assert not PP.fits_predict(model, 1, 5, kw["d"])
        with pytest.raises(_lib.MobocmfError, match=word):
            PP.PanelPredictGroup([model], 1, 5, kw["d"])
