"""The split frozen-chain predict kernel (csrc/frozen_predict.hip, CW = 8) through SplitPredictGroup (util/panel_predict.py):
moments and input gradient of surrogates with 128 < M <= 1024 against MFDGP.predict_for_acquisition through the layer entry
points and against the 16-column kernel, the group's freeze / thaw and reuse, `work`, the seeds' zeros, the variance floor, and
the refusals.
(The componentwise gate of the kernel itself, on the chain state it reads: tests/test_hip_frozen_predict_conformance.py.)"""
import pytest
import torch

from mobocmf_amd import _lib
from mobocmf_amd.util import synthetic
from tests.test_hip_model import build_model, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"

# M, d, S, fidelity, T -- see the docstring of the test for why each is there
CASES = [dict(M=513, d=8, S=5, f=1, T=3), dict(M=1024, d=8, S=25, f=1, T=2), dict(M=640, d=3, S=9, f=2, T=3),
         dict(M=520, d=2, S=4, f=0, T=20), dict(M=130, d=2, S=48, f=1, T=1)]


def _bits(t):
    return t.detach().contiguous().view(torch.int64)


def _tols(d):
    """mean / variance / gradient against the layer path: those of tests/test_hip_panel_predict.py for the same reference."""
    return (1e-6, 1e-5, 1e-4) if d <= 3 else (1e-8, 1e-7, 1e-6)


def _models(M, d, S, fidelity, seeds):
    return [build_model(synthetic.make_problem(d=d, L=max(2, fidelity + 1), M=M, N=M, S=S, seed=s), S_train=1, S_acq=S)
            for s in seeds]


def _evaluate(group, Xq, wm, wv, grad=True):
    Xb = Xq.clone().requires_grad_(grad)
    mus, v = group.acquisition_moments(Xb)
    if grad:
        ((mus * wm).sum() + (v * wv).sum()).backward()
    return mus.detach(), v.detach(), Xb.grad


@pytest.mark.parametrize("c", CASES, ids=["M%d_d%d_S%d_f%d_T%d" % (c["M"], c["d"], c["S"], c["f"], c["T"]) for c in CASES])
def test_split_predict_group_matches_predict_for_acquisition_and_its_input_gradient(c):
    """SplitPredictGroup -- MOBOCMF_STEP_FORWARD for the moments of three models, MOBOCMF_STEP_INPUT_GRADIENTS for d/dX -- against
    MFDGP.predict_for_acquisition through the layer entry points, with the weighted-sum construction and the tolerances of
    tests/test_hip_panel_predict.py.  Shapes: M = 513 one row past the 16-column kernel's limit (33 row tiles, the last with one
    real row; one part with 5 of 8 columns live); M = 1024 the LDS limit with the search's own S = 25 (four parts, the last of
    one column); M = 640 three layers, two parts (8 + 1), partials through two propagations; M = 520 fidelity 0 (8 + 8 + 4 base
    rows, no reduction launch, no work); M = 130, S = 48: six parts, T = 1.  The differences observed on an MI355X are recorded
    in DESIGN.md 5.6.2."""
    from mobocmf_amd.util.panel_predict import SplitPredictGroup, fits_predict_split
    M, d, S, fidelity, T = c["M"], c["d"], c["S"], c["f"], c["T"]
    models = _models(M, d, S, fidelity, (1, 2, 3))
    assert all(fits_predict_split(m, fidelity, T, d) for m in models)
    g = torch.Generator().manual_seed(3)
    ncol = T * (S if fidelity else 1)
    X = torch.rand(T, d, dtype=torch.float64, generator=g).to(DEV)
    wm = torch.randn(len(models), T, dtype=torch.float64, generator=g).to(DEV)
    wv = torch.randn(len(models), T, dtype=torch.float64, generator=g).to(DEV)

    Xa = X.clone().requires_grad_(True)
    ms, vs = [], []
    for m in models:
        m.eval()
        mu, v = m.predict_for_acquisition(Xa, fidelity)
        m.train()
        ms.append(mu), vs.append(v)
    ref_m, ref_v = torch.stack(ms), torch.stack(vs)
    assert ref_m.shape == (3, T)
    ((ref_m * wm).sum() + (ref_v * wv).sum()).backward()
    ref_m, ref_v, ref_g = ref_m.detach(), ref_v.detach(), Xa.grad

    grp = SplitPredictGroup(models, fidelity, T, d)
    assert grp.moments.shape == (3, 2, ncol) and grp.gx.shape == (3, T, d) and grp.S == (S if fidelity else 1)
    assert (grp.work is None) if fidelity == 0 else (grp.work.shape == (3, (S + 7) // 8 * T * d))
    mus, v, gX = _evaluate(grp, X, wm, wv)
    tm, tv, tg = _tols(d)
    errs = (rel(mus, ref_m), rel(v, ref_v), rel(gX, ref_g))
    print("split predict", c, "relative differences (mean, var, d/dX):", errs)
    assert errs[0] < tm and errs[1] < tv and errs[2] < tg, errs
    assert not any(bool(w.any()) for w in grp.info_words)


def test_bitwise_repeats_freeze_thaw_and_the_values_only_group():
    from mobocmf_amd.util.panel_predict import SplitPredictGroup
    M, d, S, T = 513, 8, 5, 3
    models = _models(M, d, S, 1, (1, 2, 3))
    g = torch.Generator().manual_seed(4)
    X, X2 = (torch.rand(T, d, dtype=torch.float64, generator=g).to(DEV) for _ in range(2))
    wm, wv = (torch.randn(3, T, dtype=torch.float64, generator=g).to(DEV) for _ in range(2))
    grp = SplitPredictGroup(models, 1, T, d)
    first = _evaluate(grp, X, wm, wv)
    other = _evaluate(grp, X2, wm, wv)
    again = _evaluate(grp, X, wm, wv)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, first))
    assert not torch.equal(_bits(other[0]), _bits(first[0]))
    grp.freeze()
    chains = grp._chains
    for Xq, want in ((X2, other), (X, first)):
        got = _evaluate(grp, Xq, wm, wv)
        assert grp._chains is chains and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))
    grp.thaw()
    assert not grp._frozen and grp._chains is None
    vals = SplitPredictGroup(models, 1, T, d, want_gradients=False)
    assert vals.seeds is None and vals.gx is None and vals.work is None
    mv, vv, _ = _evaluate(vals, X, wm, wv, grad=False)
    assert torch.equal(_bits(mv), _bits(first[0])) and torch.equal(_bits(vv), _bits(first[1]))
    with pytest.raises(_lib.MobocmfError):
        vals._launch(_lib.STEP_INPUT_GRADIENTS)


def test_against_the_16_column_kernel():
    """The same models through both kernels (M = 160, d = 1, S = 25: four parts against two base-row blocks of 16 + 9 columns):
    the layer-path tolerances bound the difference; both run the same per-column algebra in the same k-tile order, so the
    printed difference is expected far smaller."""
    from mobocmf_amd.util.panel_predict import PanelPredictGroup, SplitPredictGroup
    M, d, S, T = 160, 1, 25, 5
    models = _models(M, d, S, 1, (1, 2, 3))
    g = torch.Generator().manual_seed(5)
    X = torch.rand(T, d, dtype=torch.float64, generator=g).to(DEV)
    wm, wv = (torch.randn(3, T, dtype=torch.float64, generator=g).to(DEV) for _ in range(2))
    a = _evaluate(SplitPredictGroup(models, 1, T, d), X, wm, wv)
    b = _evaluate(PanelPredictGroup(models, 1, T, d), X, wm, wv)
    errs = tuple(rel(p, q) for p, q in zip(a, b))
    print("split against the 16-column kernel, M = 160 d = 1 S = 25: (mean, var, d/dX)", errs)
    assert all(e < t for e, t in zip(errs, _tols(d))), errs


def test_work_is_written_before_it_is_read():
    from mobocmf_amd.util.panel_predict import SplitPredictGroup
    M, d, S, T = 140, 2, 11, 4
    grp = SplitPredictGroup(_models(M, d, S, 1, (6, 7)), 1, T, d)
    g = torch.Generator().manual_seed(6)
    grp.x.copy_(torch.rand(T, d, dtype=torch.float64, generator=g))
    grp.seeds.copy_(torch.randn(2, 2, T * S, dtype=torch.float64, generator=g))
    grp.freeze()
    grp._launch(_lib.STEP_INPUT_GRADIENTS)
    want = grp.gx.clone()
    assert bool(torch.isfinite(grp.work).all())
    grp.work.fill_(float("nan"))
    grp.gx.fill_(float("nan"))
    grp._launch(_lib.STEP_INPUT_GRADIENTS)
    grp.thaw()
    assert bool(torch.isfinite(grp.gx).all()) and torch.equal(_bits(grp.gx), _bits(want)) and bool(grp.gx.any())
    assert bool(torch.isfinite(grp.work).all())


def test_zero_seeds_give_exactly_zero_input_gradients():
    """S = 11 is two parts (8 + 3).  Seeds zero on a whole model, on all columns of a test point, and on all replicas of part 0
    of another test point: exact zeros for the first two, a finite non-zero gradient (part 1's) for the third."""
    from mobocmf_amd.util.panel_predict import SplitPredictGroup
    M, d, S, T = 140, 2, 11, 6
    grp = SplitPredictGroup(_models(M, d, S, 1, (4, 5)), 1, T, d)
    g = torch.Generator().manual_seed(0)
    grp.x.copy_(torch.rand(T, d, dtype=torch.float64, generator=g))
    seeds = torch.randn(2, 2, T * S, dtype=torch.float64, generator=g).to(DEV)
    seeds[0] = 0.0                                 # model 0: nothing
    seeds[1, :, 2 * S:3 * S] = 0.0                 # model 1: test point 2 nothing ...
    seeds[1, :, 4 * S:4 * S + 8] = 0.0             # ... and part 0 of test point 4
    grp.seeds.copy_(seeds)
    grp.gx.fill_(float("nan"))
    grp._launch(_lib.STEP_INPUT_GRADIENTS)
    gx = grp.gx.cpu()
    assert bool((gx[0] == 0.0).all()) and bool((gx[1, 2] == 0.0).all())
    rest = torch.tensor([0, 1, 3, 4, 5])
    assert bool(torch.isfinite(gx[1]).all()) and bool((gx[1, rest] != 0.0).all())


def test_a_column_at_the_variance_floor_passes_no_variance_gradient():
    """The construction of tests/test_hip_panel_predict.py at M = 513: a test point equal to an inducing input of a model with
    L_S = 1e-7 I and jitter 1e-12 (d = 8 keeps K_mm well conditioned)."""
    from mobocmf_amd.util.panel_predict import SplitPredictGroup
    M, d, T = 513, 8, 3
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
    grp = SplitPredictGroup([model], 0, T, d)
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
    cases = [(dict(M=128, d=2, S=3), "M = 128"), (dict(M=1025, d=2, S=3), "M = 1025"), (dict(M=130, d=2, S=1), "S = 1"),
             (dict(M=130, d=9, S=3), "d = 9")]
    for kw, word in cases:
        model = build_model(synthetic.make_problem(L=2, N=kw["M"], seed=0, **kw), S_train=1, S_acq=kw["S"])
        assert not PP.fits_predict_split(model, 1, 5, kw["d"])
        with pytest.raises(_lib.MobocmfError, match=word):
            PP.SplitPredictGroup([model], 1, 5, kw["d"])
