"""The MES baseline's device acquisition search: ExactGPPredictGroup (util/exact_predict.py) against the models' own host
statement, MesDeviceAcqSearch (util/acq_search.py) against the host loop over the SAME group, and MESMOC_MFGP(search="device")
through its public surface."""
import pytest
import torch

from tests import mes_reference as M

pytestmark = pytest.mark.gpu

DEV = "cuda"

# Device engine against host loop over the same predict group: the two differ in the MES arithmetic (the kernel's analytic seeds
# against autograd through the torch statement, ulps apart times kappa) and in summation order.  D, the largest relative
# difference over best_x, best_v, the candidate and its value at the sizes of test_engine_parity_at_short_horizon, measured on an
# MI355X: 9.1e-13 (best_v at n = 130, fidelity 0; 1.8e-15 at n = 24, fidelity 1; exactly 0 in the other two
# cases, whose restarts end on the box's faces).  Asserted at 100 D.
D_MEASURED = 9.1e-13
PARITY_TOL = 100.0 * D_MEASURED
BEST = (0.3, -0.2, 0.1)      # mes_problem's best values of o0, o1 and threshold of c0


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


_models = {}


def _gpu_models(n):
    if n not in _models:
        _models[n] = M.mes_models(n, device=DEV)
    return _models[n]


def _groups(n, fidelity, want=(200, 5)):
    from mobocmf_amd.util.exact_predict import ExactGPPredictGroup
    models = list(_gpu_models(n).values())      # o0, o1, c0
    levels = [fidelity, fidelity, 1]            # the objectives at the searched level, the constraint at the top
    return {T: ExactGPPredictGroup(models, levels, T, 2, want_gradients=T == 5) for T in want}


def _bounds():
    return torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("n", [24, 130])
def test_group_moments_are_the_models_posterior_and_autograd_is_the_engines_gradient(n):
    """moments_at == _ExactMFGP.posterior (the torch statement: a fresh Cholesky) of every model at its level, to 1e-8 of the
    prior variance (n cond u, cond(K) in the hundreds at noise 0.1); d/dX of the MES statement through moments_at (autograd,
    one INPUT_GRADIENTS launch) == the engine's chain FORWARD -> mobocmf_mes_group_forward -> INPUT_GRADIENTS, gx summed."""
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as F
    grp = _groups(n, 0, want=(5,))[5]
    X = torch.rand(5, 2, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))
    with grp.frozen():
        assert not any(int(w) for w in torch.cat(grp.info_words).cpu())
        mom = grp.moments_at(X)
        for i, (model, level) in enumerate(zip(grp.models, grp.levels)):
            model.eval()
            with torch.no_grad():
                post = model.posterior(torch.cat([X, level * torch.ones(5, 1, dtype=torch.float64, device=DEV)], 1))
            model.train()
            kss = float(grp.host[i].kss)
            assert float((mom[i, 0] - post.mean).abs().max()) <= 1e-8 * kss
            assert float((mom[i, 1] - post.variance).abs().max()) <= 1e-8 * kss
        noise, best = grp.noise().detach(), torch.tensor(BEST, dtype=torch.float64, device=DEV)
        Xg = X.clone().requires_grad_(True)
        val = M.mes_torch(grp.moments_at(Xg), noise, best, 2, 1)
        (gx,) = torch.autograd.grad(val.sum(), Xg)
        grp.x.copy_(X)
        grp._launch(_lib.STEP_FORWARD)
        acq = torch.zeros(5, dtype=torch.float64, device=DEV)
        F.mes_group_forward(grp.moments, noise, best, 2, 1, 5, acq, seeds=grp.seeds)
        grp._launch(_lib.STEP_INPUT_GRADIENTS)
        mine = grp.gx.sum(0)
    assert float(val.detach().abs().max()) > 0 and float(gx.abs().max()) > 0
    assert _rel(acq, val) <= 1e-9 and _rel(mine, gx) <= 1e-9
    assert not grp._frozen
    assert torch.allclose(grp.noise(), torch.stack([m.likelihood.noise.reshape(()) for m in grp.models]).detach())


@pytest.mark.parametrize("n", [24, 130])
@pytest.mark.parametrize("fidelity", [0, 1])
def test_engine_parity_at_short_horizon(n, fidelity):
    """MesDeviceAcqSearch, graphed, eager and two iterates per graph, against optimize_acqf_multistart on the torch MES
    statement over the same groups' moments_at, from equal generator states: 5 restarts of 200 raw candidates, 10 iterations."""
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import optimize_acqf_multistart
    from mobocmf_amd.util.acq_search import MesDeviceAcqSearch
    groups = _groups(n, fidelity)
    bounds = _bounds()
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)
    noise, best = groups[5].noise().detach(), torch.tensor(BEST, dtype=torch.float64, device=DEV)
    calls = []

    def acq_fn(X):
        out = M.mes_torch(groups[X.shape[0]].moments_at(X), noise, best, 2, 1)
        calls.append((X.detach().clone(), out.detach().clone()))
        return out

    def freeze(on):
        for grp in groups.values():
            grp.freeze() if on else grp.thaw()

    freeze(True)
    cand_h, val_h = optimize_acqf_multistart(acq_fn, bounds, num_restarts=5, raw_samples=200, maxiter=10, generator=gen())
    freeze(False)
    raw = calls[0][1].cpu()
    top = torch.sort(raw, descending=True).values[:6]
    assert float(top[4]) > 0.0 and len(set(top.tolist())) == 6, top      # precondition: the restarts are well defined
    assert len(calls) == 12      # the raw candidates, X_0 ... X_10
    best_x, best_v = calls[1][0].clone(), calls[1][1].clone()
    for X, v in calls[2:]:       # the host loop's own tracking, on its own evaluations
        better = v > best_v
        best_v = torch.where(better, v, best_v)
        best_x[better] = X[better]
    assert torch.equal(cand_h[0], best_x[int(torch.argmax(best_v))]) and torch.equal(val_h, best_v.max())

    eng = MesDeviceAcqSearch(groups[5], bounds, 5, 0.02, best, 2, 1)
    res = {}
    for mode, (graphed, per) in dict(graph=(True, 1), eager=(False, 1), graph2=(True, 2)).items():
        eng.use_graph, eng.iters_per_graph = graphed, per
        Xraw = bounds[0] + (bounds[1] - bounds[0]) * torch.rand(200, 2, dtype=torch.float64, device=DEV, generator=gen())
        assert torch.equal(Xraw, calls[0][0])
        raw_d, top_v, top_i = eng.start_from_raw(groups[200], Xraw)
        if mode == "graph":
            assert torch.equal(top_i.cpu(), torch.topk(raw, 5).indices) and torch.equal(groups[5].x, calls[1][0])
            print("raw candidates: largest relative difference", _rel(raw_d, raw))
            assert _rel(raw_d, raw) <= PARITY_TOL
        cand, val = eng.run(None, 10)
        torch.cuda.synchronize()
        freeze(False)
        res[mode] = [t.clone() for t in (cand, val, eng.best_x, eng.best_v, eng.steps_done, groups[5].x)]
        assert int(eng.steps_done[0]) == 10
        assert not bool(eng.info_words().any())
    assert sorted(eng._graphs) == [1, 2]
    for other in ("eager", "graph2"):      # graphed, eager, two iterates per graph: the same launches
        for a, b in zip(res["graph"], res[other]):
            assert torch.equal(_bits(a) if a.dtype == torch.float64 else a, _bits(b) if b.dtype == torch.float64 else b), other
    cand, val, bx, bv = res["graph"][:4]
    diffs = dict(best_x=_rel(bx, best_x), best_v=_rel(bv, best_v), candidate=_rel(cand, cand_h), value=_rel(val, val_h))
    print("MES engine parity n = %d fidelity %d: largest relative differences" % (n, fidelity), diffs)
    assert max(diffs.values()) <= PARITY_TOL, diffs
    assert bool((bv.cpu() >= top_v.cpu()).all())      # X_0 is scored too


def _next_point(acq, engine, seed=5, maxiter=20):
    acq.search = engine
    return acq.get_nextpoint_coupled(maxiter=maxiter, generator=torch.Generator(device=DEV).manual_seed(seed))


def test_device_search_through_the_public_surface():
    acq = M.mes_problem(24, device=DEV, models=_gpu_models(24))
    lo, hi = acq.standard_bounds[0], acq.standard_bounds[1]
    cand_h, fid_h = _next_point(acq, "host")
    assert acq.last_search_engine == {0: "host", 1: "host"}
    cand_d, fid_d = _next_point(acq, "device")
    assert acq.last_search_engine == {0: "device", 1: "device"}
    print("public surface: host", cand_h.tolist(), fid_h, "device", cand_d.tolist(), fid_d)
    assert cand_d.shape == (2,) and bool((cand_d >= lo).all()) and bool((cand_d <= hi).all())
    assert torch.equal(cand_d, acq.last_search_candidates[fid_d][0])
    gen = torch.Generator(device=DEV).manual_seed(5)      # the draws of the call above, fidelity by fidelity
    with torch.no_grad():
        for f in (0, 1):
            Xraw = lo + (hi - lo) * torch.rand(200, 2, dtype=torch.float64, device=DEV, generator=gen)
            eng = acq._device_searches[f][1]
            assert int(eng.steps_done[0]) == 20 and not eng.group._frozen and not eng.raw_group._frozen
            c = acq.last_search_candidates[f]
            assert c.shape == (1, 2) and bool((c >= lo).all()) and bool((c <= hi).all())
            host_at = float(acq.coupled_acq(c, fidelity=f)[0])
            raw_best = float(acq.coupled_acq(Xraw, fidelity=f).max())
            # cannot fail through trajectory divergence: X_0 is scored, and the winner is the best of everything scored
            assert raw_best > 0 and host_at >= raw_best * (1.0 - 1e-9), (f, host_at, raw_best)
            assert abs(acq.last_search_values[f] - host_at) <= 1e-8 * abs(host_at), (f, acq.last_search_values[f], host_at)
    w = {f: acq.last_search_values[f] / acq.costs_blackboxes[f]["total"] for f in (0, 1)}
    assert fid_d == max(w, key=w.get)
    acq.search = "host"


def test_a_model_past_the_kernels_limit_keeps_the_host_engine_and_says_so():
    from mobocmf_amd.util.exact_predict import ExactGPPredictGroup
    models = dict(_gpu_models(24))
    models["o1"] = M.mes_models(513, device=DEV)["o1"]
    reason = ExactGPPredictGroup.why_not(models["o1"], 0, 5, 2)
    assert reason is not None and "513" in reason
    assert ExactGPPredictGroup.why_not(models["o0"], 0, 5, 2) is None
    assert "GPU" in ExactGPPredictGroup.why_not(M.mes_models(8)["o0"], 0, 5, 2)
    acq = M.mes_problem(24, device=DEV, models=models, search="device")
    cand, fid = acq.get_nextpoint_coupled(maxiter=1, generator=torch.Generator(device=DEV).manual_seed(5))
    assert acq.last_search_engine == {0: "host", 1: "host"} and set(acq.last_search_values) == {0, 1}
    assert cand.shape == (2,) and fid in (0, 1)
