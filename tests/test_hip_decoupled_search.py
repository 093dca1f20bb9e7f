"""Decoupled evaluations on the device (util/acq_search.py DecoupledDeviceAcqSearch, JESMOC_MFDGP.get_nextpoint_decoupled,
BlackBoxMFDGPFitter(decoupled_evals=True)): the zero seeds of mobocmf_jes_mc_box_forward give a zero input gradient through every
kind of predict group; the engine against the host loop over the per-box value from the same raw candidates; the public surface
on the toy 2-D problem; the fitter's phases over unequal data sets."""
import os
import sys

import numpy as np
import pytest
import torch

from mobocmf_amd.util import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

# D_3: the largest relative difference between the per-(fidelity, box) winning values of DecoupledDeviceAcqSearch and of
# optimize_acqf_multistart over that box's value through the same models, at the sizes of test_engine_parity_per_box below,
# measured on an MI355X.  As for D_1 (tests/test_hip_acq_search.py) and D_2 (tests/test_hip_jes_mc.py) the
# engines differ in summation order only -- here also in the rows a launch holds: the device group evaluates B R rows, the host
# group R -- and the models' conditioning amplifies a one-ulp seed difference from the second iterate on.  At fidelity 0 (S = 1)
# exactly 0 in all four cases; at fidelity 1, M = 24: 8.3e-11 (K = 1) and 2.8e-11 (K = 2), M = 64: 2.4e-11 (K = 1) and 1.18e-10
# (K = 2).  Asserted at 100 D_3.
D3_MEASURED = 1.2e-10
PARITY_TOL = 100.0 * D3_MEASURED


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _bounds(d=2):
    return torch.stack([torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)]).to(DEV)


# ------------------------------------------------------------------ G3. zero seeds give a zero gradient
def _lightly_trained(M, seed, n, epochs=4):
    """``n`` surrogates of M = N inducing points carrying a synthetic problem's parameters, then a handful of Adam epochs on
    their own ELBO (the layer path): the variational parameters and hyper-parameters of a fit under way."""
    from mobocmf_amd import functional as F
    from mobocmf_amd.mlls import VariationalELBOMF
    from tests.helpers import to_t
    from tests.test_hip_model import build_model
    models = []
    for i in range(n):
        prob = synthetic.make_problem(d=2, L=2, M=M, N=M, S=5, seed=seed + i)
        model = build_model(prob, S_train=1, S_acq=5)
        elbo = VariationalELBOMF(model, M, 2)
        x, y, fid = to_t(prob["x"]).to(DEV), to_t(prob["y"])[:, None].to(DEV), to_t(prob["fid"])[:, None].to(DEV)
        opt = F.FusedAdam(list(model.parameters()), lr=1e-3)
        for _ in range(epochs):
            opt.zero_grad()
            (-elbo(model(x), y.T, fid)[0]).backward()
            opt.step()
        models.append(model)
    return models


def _group_of(kind, models, fidelity, T):
    from mobocmf_amd.util.coop_step import CoopPredictGroup
    from mobocmf_amd.util.panel_predict import PanelPredictGroup
    from mobocmf_amd.util.tiny_step import TinyPredictGroup
    return dict(tiny=TinyPredictGroup, coop=CoopPredictGroup, panel=PanelPredictGroup)[kind](models, fidelity, T, 2)


@pytest.mark.parametrize("kind,M,K", [("tiny", 24, 2), ("coop", 64, 2), ("panel", 129, 1)])
def test_models_outside_the_box_of_a_row_get_a_zero_gradient(kind, M, K):
    """One decoupled iterate through each kind of predict group (panel: M = 129, the smallest it takes), two black-boxes,
    fidelity 1 (S = 5 columns per row): gx[m, t] is exactly 0 for every model m outside the box of row t, finite and not all
    zero inside -- so mobocmf_ascent_adam_step's sum over all models is the gradient of the row's own term."""
    from mobocmf_amd import _lib
    from mobocmf_amd.util.acq_search import DecoupledDeviceAcqSearch
    B, R = 2, 3
    models = _lightly_trained(M, 500 + M, B * (1 + K))
    grp = _group_of(kind, models, 1, B * R)
    eng = DecoupledDeviceAcqSearch(grp, _bounds(), R, 0.02, num_pareto_samples=K)
    assert eng.box_of_point.tolist() == [0, 0, 0, 1, 1, 1] and eng.box_of_point.dtype == torch.int32
    X = torch.rand(B * R, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(M)).to(DEV)
    with torch.no_grad():
        grp.x.copy_(X)
        grp.gx.fill_(float("nan"))
        grp.seeds.fill_(float("nan"))
        eng.best_v.fill_(float("-inf"))
        grp.freeze()
        eng._iterate()
        torch.cuda.synchronize()
        grp.thaw()
    assert not bool(eng.info_words().any())
    gx, seeds = grp.gx.cpu(), grp.seeds.cpu()
    own = (torch.arange(B * (1 + K))[:, None] // (1 + K)) == eng.box_of_point.cpu()[None, :].long()      # (models, rows)
    assert bool((gx[~own] == 0.0).all()), gx[~own].abs().max()
    assert bool(torch.isfinite(gx[own]).all()) and bool((gx[own] != 0.0).any())
    S = grp.S
    own_cols = own[:, None, :, None].expand(-1, 2, -1, S).reshape(seeds.shape)
    assert bool((_bits(seeds)[~own_cols] == 0).all()) and bool(torch.isfinite(seeds[own_cols]).all())
    assert int(eng.steps_done[0]) == 1 and not torch.equal(grp.x.cpu(), X.cpu())      # the step was taken
    assert torch.equal(_bits(eng.best_v), _bits(eng.acq)) and torch.equal(eng.best_x.cpu(), X.cpu())
    with pytest.raises(_lib.MobocmfError):
        DecoupledDeviceAcqSearch(grp, _bounds(), R + 1, 0.02, num_pareto_samples=K)      # T != B R


# ------------------------------------------------------------------ G4. engine parity, per box
@pytest.mark.parametrize("M,seed", [(24, 100), (64, 200)], ids=["M24_one_workgroup", "M64_cooperative"])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("fidelity", [0, 1])
def test_engine_parity_per_box(M, seed, K, fidelity):
    """The set-up of tests/test_hip_jes_mc.py test_engine_parity_at_short_horizon_with_two_samples: two black-boxes, 5 restarts
    of 200 raw candidates, 10 iterations.  Reference: optimize_acqf_multistart over the per-box expression written HERE through
    ordinary predict groups (T = 200 and T = 5), one search per box from equal generator states -- nothing of the decoupled
    engine or of mobocmf_jes_mc_box_forward is in it."""
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import optimize_acqf_multistart
    from mobocmf_amd.util.acq_search import DecoupledDeviceAcqSearch
    from tests.test_hip_acq_search import _group
    from tests.test_hip_jes_mc import _models
    B, R = 2, 5
    models = _models(M, seed)[:B * (1 + K)]
    groups = {T: _group(models, fidelity, T) for T in (200, R, B * R)}
    bounds = _bounds()
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)

    def freeze(on):
        for grp in groups.values():
            grp.freeze() if on else grp.thaw()

    host, raws = [], []
    for p in range(B):
        calls = []

        def box_fn(X, p=p):
            X2 = X[:, 0, :] if X.dim() > 2 else X
            _, v = groups[X2.shape[0]].acquisition_moments(X2)
            u = p * (1 + K)
            box = None
            for k in range(1, K + 1):
                term = 0.5 * torch.clamp(torch.log(v[u]) - torch.log(v[u + k]), min=0.0)
                box = term if box is None else box + term
            out = (1.0 / K) * box
            calls.append((X2.detach().clone(), out.detach().clone()))
            return out

        freeze(True)
        cand_h, val_h = optimize_acqf_multistart(box_fn, bounds, num_restarts=R, raw_samples=200, maxiter=10, generator=gen())
        freeze(False)
        raw = calls[0][1].cpu()
        top = torch.sort(raw, descending=True).values[:R + 1]
        # precondition (torch.topk's tie order is unspecified, a box's JES is exactly 0 on part of the domain)
        assert float(top[R - 1]) > 0.0 and len(set(top.tolist())) == R + 1, (p, top)
        host.append((cand_h, val_h, calls[1][0]))
        raws.append((calls[0][0], raw))

    eng = DecoupledDeviceAcqSearch(groups[B * R], bounds, R, 0.02, num_pareto_samples=K)
    res = {}
    for graphed in (True, False):
        eng.use_graph = graphed
        Xraw = bounds[0] + (bounds[1] - bounds[0]) * torch.rand(200, 2, dtype=torch.float64, device=DEV, generator=gen())
        assert all(torch.equal(Xraw, r[0]) for r in raws)
        vals, top_v, top_i = eng.start_from_raw(groups[200], Xraw)
        if graphed:
            for p in range(B):      # the restarts chosen from the raw candidates: index-identical per box
                assert torch.equal(top_i[p].cpu(), torch.topk(raws[p][1], R).indices), p
                assert torch.equal(groups[B * R].x[p * R:(p + 1) * R], host[p][2])
                assert _rel(vals[p], raws[p][1]) <= PARITY_TOL
        cands, values = eng.run(None, 10)
        freeze(False)
        res[graphed] = [t.clone() for t in (cands, values, eng.best_x, eng.best_v, eng.steps_done, groups[B * R].x)]
        assert int(eng.steps_done[0]) == 10 and not bool(eng.info_words().any())
    assert len(eng._graphs) == 1
    for a, b in zip(res[True], res[False]):      # graphed and eager: the same launches
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
    cands, values = res[True][:2]
    assert cands.shape == (B, 2) and values.shape == (B,)
    diffs = [_rel(values[p], host[p][1]) for p in range(B)]
    print("decoupled engine parity M = %d K = %d fidelity %d: relative differences of the winning values per box" % (M, K, fidelity),
          diffs, "candidates", [_rel(cands[p], host[p][0][0]) for p in range(B)])
    assert max(diffs) <= PARITY_TOL, diffs
    assert bool((res[True][3].reshape(B, R).max(1).values.cpu() >= top_v[:, 0].cpu()).all())      # X_0 is scored too


# ------------------------------------------------------------------ G5. through the public surface
def _toy_acq():
    """The acquisition object of one toy BO iteration (14 + 6 points, obj1 / obj2 / con1), shared with tests/test_hip_acq_search.py."""
    from tests.test_hip_acq_search import _toy_acq as shared
    return shared("M20_one_workgroup")


def _decoupled(acq, engine, seed=5, maxiter=20):
    acq.search = engine
    try:
        return acq.get_nextpoint_decoupled(maxiter=maxiter, generator=torch.Generator(device=DEV).manual_seed(seed))
    finally:
        acq.search = "host"


def test_decoupled_device_search_through_the_public_surface():
    acq = _toy_acq()
    lo, hi = acq.standard_bounds[0], acq.standard_bounds[1]
    x, fidelity, name, is_con = _decoupled(acq, "device")
    assert acq.last_search_engine == {0: "device", 1: "device"}
    vals = dict(acq.last_decoupled_values)
    keys = [(f, n) for f in (0, 1) for n in ("obj1", "obj2", "con1")]
    assert list(vals) == keys and all(np.isfinite(v) and v >= 0.0 for v in vals.values()) and max(vals.values()) > 0.0
    weighed = [vals[k] / acq.costs_blackboxes[k[0]][k[1]] for k in keys]
    want = keys[int(np.argmax(weighed))]      # (np.argmax: the first of equal ones)
    assert (fidelity, name) == want and is_con == (name == "con1")
    eng = acq._decoupled_searches[fidelity]
    p = [n for n, _, _ in acq._boxes(fidelity)].index(name)
    assert x.shape == (2,) and torch.equal(_bits(x), _bits(eng.cand[p])) and bool((x >= lo).all()) and bool((x <= hi).all())
    for f in (0, 1):
        e = acq._decoupled_searches[f]
        assert (e.B, e.R, e.T) == (3, 5, 15) and int(e.steps_done[0]) == 20 and e is not acq.__dict__.get("_device_searches", {}).get(f)
        for q, (n, _, _) in enumerate(acq._boxes(f)):      # not below the box's best raw candidate; the value at the candidate
            assert vals[(f, n)] >= float(e.raw_values[q].max())
            again = float(acq._box_acq(e.cand[q:q + 1], f, q, n, n == "con1")[0])
            assert abs(vals[(f, n)] - again) <= 1e-9 * abs(again) + 1e-300, (f, n, vals[(f, n)], again)
    x2, f2, n2, c2 = _decoupled(acq, "device")
    assert (f2, n2, c2) == (fidelity, name, is_con) and torch.equal(_bits(x2), _bits(x))


def test_too_many_models_for_the_decoupled_device_engine_run_the_host_loop(monkeypatch):
    """3 black-boxes x 2 models against a bound of 2 x 2 (the library's is 2 x 32: 65 models are not built here)."""
    from mobocmf_amd import _lib
    acq = _toy_acq()
    monkeypatch.setattr(_lib, "ACQ_MAX_PAIRS", 2)
    x, fidelity, name, is_con = _decoupled(acq, "device", maxiter=2)
    assert acq.last_search_engine == {0: "host", 1: "host"}
    assert bool((x >= acq.standard_bounds[0]).all()) and bool((x <= acq.standard_bounds[1]).all())
    assert (fidelity, name) in acq.last_decoupled_values
    monkeypatch.setattr(_lib, "ACQ_MAX_PAIRS", 3)      # 6 models: exactly the bound
    _decoupled(acq, "device", maxiter=2)
    assert acq.last_search_engine == {0: "device", 1: "device"}


# ------------------------------------------------------------------ the fitter over unequal data sets
def test_fitter_phases_run_over_unequal_datasets():
    """decoupled_evals=True with 20, 21 and 23 rows per black-box: the unconditioned fit, Pareto sampling (unseeded and
    seeded), conditioned_copies (copy_uncond inside), the conditioned fit in one launch and graphed, recommend, and the
    decoupled search on both engines with two Pareto samples."""
    from bo_iteration_toy2d import blackboxes
    from bo_loop_decoupled_toy2d import choose, fit
    rng = np.random.default_rng(3)
    data = {}
    for k, name in enumerate(blackboxes()):
        n_low, n_high = 14 + k, 6 + k // 2
        data[name] = (rng.uniform(size=(n_low + n_high, 2)), np.concatenate([np.zeros(n_low), np.ones(n_high)]))
    sizes = [x.shape[0] for x, _ in data.values()]
    assert sizes == [20, 21, 23]
    fitter = fit(data, epochs=20, seed=0, grid=20)
    assert [h.num_data for _, _, h in fitter._handlers()] == sizes and fitter.x_train.shape == (sum(sizes), 2)
    assert fitter.objs_train is None and fitter.cons_train is None
    fitter.sample_and_store_pareto_solution(seed=3)
    seeded = fitter.pareto_set.clone()
    fitter.sample_and_store_pareto_solution(seed=3)
    assert torch.equal(fitter.pareto_set, seeded)
    acq, x, fidelity, name, is_con = choose(fitter, search="device", pareto_samples=2, cond_iters=6, acq_iters=5)
    assert acq.last_search_engine == {0: "device", 1: "device"} and len(acq.blackbox_mfdgp_fitters_cond) == 2
    assert x.shape == (2,) and bool((x >= 0).all()) and bool((x <= 1).all()) and (fidelity, name) in acq.last_decoupled_values
    assert len(acq._decoupled_searches[1].group.models) == 9
    acq.search = "host"
    xh, fh, nh, ch = acq.get_nextpoint_decoupled(maxiter=5)
    assert acq.last_search_engine == {0: "host", 1: "host"} and (fh, nh) in acq.last_decoupled_values
    graphed = acq.blackbox_mfdgp_fitters_cond[1]
    graphed.use_tiny_step = False
    graphed.train_conditioned_mfdgps(num_iters=3)      # the captured layer-path iteration
    rec_set, front, info = acq.blackbox_mfdgp_fitter_uncond.recommend(rng.uniform(size=(200, 2)), min_feasible_prob=0.5)
    assert rec_set.shape[1] == 2 and front.shape == (rec_set.shape[0], 2) and info["num_nan"] == 0
