"""JES averaged over K sampled Pareto sets on the device (mobocmf_jes_mc_group_forward in csrc/acq_search.hip,
DeviceAcqSearch(num_pareto_samples=K), JESMOC_MFDGP(num_pareto_samples=K)): the kernel against its float64 restatement
(tests/jes_mc_reference.py) and, at K = 1, bit for bit against what the retired pair kernel computed (tests/golden); the search
engine against the host loop over the same predict groups; the estimator through the public surface on the toy 2-D problem."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import acq_search_reference as R1
from tests import jes_mc_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

# Device engine against host engine with K = 2 conditioned surrogates per black-box, at the sizes and the horizon of
# tests/test_hip_acq_search.py::test_engine_parity_at_short_horizon (two black-boxes: the same six models).  As there, the two
# engines differ in summation order only and the difference is amplified by the models' conditioning once the iterates differ
# by an ulp, so the bound is a measurement: D_2, the largest relative difference over best_x, best_v, the candidate and its
# value, measured on an MI355X: at fidelity 0 (S = 1) 1.7e-11 at M = 24 and exactly 0 at M = 64 (with K = 2
# the seed of an unconditioned model, count * 0.5 / (K v), and autograd's sum of K products differ by an ulp, which K = 1 does
# not have); at fidelity 1 2.9e-11 at M = 24 and 2.8e-10 at M = 64 -- twice the K = 1 figure (1.4e-10).  Asserted at 100 D_2.
D2_MEASURED = 2.8e-10
PARITY_TOL = 100.0 * D2_MEASURED
GROUP_VS_LAYER = 1e-6      # the coupled value through a predict group against the layer path (tests/test_hip_coop_step.py)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


# ------------------------------------------------------------------ 1. the kernel against the restatement
SHAPES = [(1, 1, 1, 1), (3, 1, 5, 4), (1, 3, 1, 1), (2, 4, 5, 4), (3, 2, 67, 1), (2, 8, 200, 5)]


@pytest.mark.parametrize("n_boxes,K,T,S", SHAPES)
def test_jes_mc_group_forward_matches_the_reference(n_boxes, K, T, S):
    """Four complementary patterns of which conditioned samples pass the clamp (jes_mc_reference.mc_inputs): over them every
    black-box meets test points where none, some (K >= 2) and all of its K samples pass -- within each pattern where T >= 4."""
    from mobocmf_amd import functional as F
    seen = [set() for _ in range(n_boxes)]
    for flip in range(4):
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=10 * T + S + K, flip=flip)
        acq_ref, seeds_ref, scale = R.jes_mc_group_forward(mom, noise, K, T, S)
        count = R.passing(mom, noise, K, T, S).sum(1)      # (n_boxes, T)
        for p in range(n_boxes):
            kinds = {"none" if c == 0 else "all" if c == K else "some" for c in count[p].tolist()}
            assert T < 4 or kinds == ({"none", "some", "all"} if K >= 2 else {"none", "all"}), (p, flip, kinds)
            seen[p] |= kinds
        gu = seeds_ref[0::1 + K, 1].reshape(n_boxes, T, S)      # d acq / d var of the unconditioned model: count 0.5 / (K v_u S)
        assert bool((gu[count == 0] == 0.0).all()) and bool((gu[count > 0] > 0.0).all())
        md, nd = mom.to(DEV), noise.to(DEV)
        acq = torch.full((T,), float("nan"), dtype=torch.float64, device=DEV)
        seeds = torch.full_like(md, float("nan"))
        F.jes_mc_group_forward(md, nd, K, T, S, acq, seeds=seeds)
        acq2 = torch.full_like(acq, float("nan"))
        F.jes_mc_group_forward(md, nd, K, T, S, acq2)      # want_seeds = 0: the same values, nothing else written
        acq3, seeds3 = torch.full_like(acq, float("nan")), torch.full_like(md, float("nan"))
        F.jes_mc_group_forward(md, nd, K, T, S, acq3, seeds=seeds3)      # a repeat call: the same bits
        torch.cuda.synchronize()
        err = (acq.cpu() - acq_ref).abs()
        print("jes_mc_group_forward", (n_boxes, K, T, S), "flip", flip, "acq err / bound", float((err / (1e-14 * (1.0 + scale))).max()),
              "seeds rel", float((seeds.cpu() - seeds_ref).abs().max() / seeds_ref.abs().max().clamp_min(1e-300)))
        assert bool((err <= 1e-14 * (1.0 + scale)).all())
        assert float((seeds.cpu() - seeds_ref).abs().max()) <= 1e-12 * float(seeds_ref.abs().max())
        assert torch.equal(_bits(acq), _bits(acq2))
        assert torch.equal(_bits(acq), _bits(acq3)) and torch.equal(_bits(seeds), _bits(seeds3))
    want = {"none", "some", "all"} if K >= 2 else {"none", "all"}
    assert all(s == want for s in seen), seen


# ------------------------------------------------------------------ 2. K = 1: what the retired pair kernel computed, bit for bit
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jes_pair_kernel_bits.npz")
_golden = {}


def _recorded(key):
    if not _golden:
        _golden.update(np.load(_GOLDEN))
    return torch.from_numpy(_golden[key].copy()).view(torch.float64)


@pytest.mark.parametrize("n_pairs,T,S", [(3, 5, 4), (2, 67, 1), (32, 3, 2)])
def test_one_sample_reproduces_the_recorded_pair_kernel(n_pairs, T, S):
    """tests/golden/jes_pair_kernel_bits.npz (tools/record_jes_pair_golden.py): inputs and outputs of three consecutive calls of
    the one-thread-per-test-point kernel that mobocmf_jes_group_forward launched before it became the K = 1 case of
    mobocmf_jes_mc_group_forward, recorded on an MI355X.  Both entry points reproduce acq, seeds, best_v and best_x after
    every call; (32, 3, 2): 64 models, every lane of the wavefront busy."""
    from mobocmf_amd import functional as F
    d = 3
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
    best = {name: (torch.full((T,), float("-inf"), dtype=torch.float64, device=DEV), z(T, d)) for name in ("pair", "mc")}
    moved = []
    for call in range(3):      # (inputs: jes_mc_reference.mc_inputs(n_pairs, 1, T, S, seed=30 + call, flip=call), as recorded)
        rec = lambda name: _recorded("%d_%d_%d/%d/%s" % (n_pairs, T, S, call, name))
        md, nd, x = rec("moments").to(DEV), rec("noise").to(DEV), rec("x").to(DEV)
        want = [rec(name) for name in ("acq", "seeds", "best_v", "best_x")]
        for name in ("pair", "mc"):
            acq, seeds = z(T), torch.full_like(md, float("nan"))
            before = best[name][0].clone()
            if name == "pair":
                F.jes_group_forward(md, nd, T, S, acq, seeds=seeds, x=x, best_v=best[name][0], best_x=best[name][1])
            else:
                F.jes_mc_group_forward(md, nd, 1, T, S, acq, seeds=seeds, x=x, best_v=best[name][0], best_x=best[name][1])
            for got, w in zip((acq, seeds, best[name][0], best[name][1]), want):
                assert torch.equal(_bits(got), _bits(w)), (name, call)
            moved.append(int((acq > before).sum()))
        assert bool((want[1][0::2, 1] == 0.0).any()) and bool((want[1][0::2, 1] > 0.0).any())
    assert moved[0] == T and (T <= 5 or 0 < moved[-1] < T)


_KERNELS = os.path.join(os.path.dirname(_GOLDEN), "jes_kernels_bits.npz")
_kernels = {}


@pytest.mark.parametrize("n_boxes,K,T,S", [(2, 4, 5, 4), (3, 2, 9, 1), (1, 63, 3, 2)])
def test_coupled_launch_reproduces_the_recorded_bits(n_boxes, K, T, S):
    """tests/golden/jes_kernels_bits.npz (tools/record_jes_pair_golden.py --fixture kernels): three consecutive tracked calls of
    mobocmf_jes_mc_group_forward at K > 1, recorded on an MI355X while the coupled and the per-box launch were two kernels.
    The regenerated inputs are the stored ones bit for bit (a drifting generator fails here, not silently); then acq, seeds,
    best_v and best_x after every call are."""
    from mobocmf_amd import functional as F
    if not _kernels:
        _kernels.update(np.load(_KERNELS))
    d = 3
    g = torch.Generator().manual_seed(T)
    best_v = torch.full((T,), float("-inf"), dtype=torch.float64, device=DEV)
    best_x = torch.zeros(T, d, dtype=torch.float64, device=DEV)
    for call in range(3):
        rec = lambda name: torch.from_numpy(_kernels["%d_%d_%d_%d/%d/%s" % (n_boxes, K, T, S, call, name)].copy())
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=50 + call, flip=call)
        x = torch.rand(T, d, dtype=torch.float64, generator=g)
        for name, t in (("moments", mom), ("noise", noise), ("x", x)):
            assert torch.equal(_bits(t), rec(name)), (name, call)
        md = mom.to(DEV)
        acq, seeds = torch.full((T,), float("nan"), dtype=torch.float64, device=DEV), torch.full_like(md, float("nan"))
        F.jes_mc_group_forward(md, noise.to(DEV), K, T, S, acq, seeds=seeds, x=x.to(DEV), best_v=best_v, best_x=best_x)
        for name, got in (("acq", acq), ("seeds", seeds), ("best_v", best_v), ("best_x", best_x)):
            assert torch.equal(_bits(got), rec(name)), (name, call)


# ------------------------------------------------------------------ 3. tracking, bad arguments
def test_jes_mc_group_forward_tracks_the_best_iterate():
    """The three-call scenario of tests/test_hip_acq_search.py: the element-wise larger value and its row stay (strict), the -inf
    the caller starts from is replaced by any finite value, a NaN value never replaces anything."""
    from mobocmf_amd import functional as F
    n_boxes, K, T, S, d = 2, 3, 70, 2, 3
    g = torch.Generator().manual_seed(2)
    best_v = torch.full((T,), float("-inf"), dtype=torch.float64, device=DEV)
    best_x = torch.zeros(T, d, dtype=torch.float64, device=DEV)
    acq = torch.zeros(T, dtype=torch.float64, device=DEV)
    for call in range(3):
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=20 + call, flip=call)
        if call == 0:
            mom[2, 1, S:2 * S] = float("nan")      # test point 1 (a conditioned model): no value on the first call
        if call == 1:
            mom[0, 1, :S] = float("nan")           # test point 0 (an unconditioned model): no value on the second
        x = torch.rand(T, d, dtype=torch.float64, generator=g)
        prev_v, prev_x = best_v.cpu(), best_x.cpu()
        F.jes_mc_group_forward(mom.to(DEV), noise.to(DEV), K, T, S, acq, x=x.to(DEV), best_v=best_v, best_x=best_x)
        torch.cuda.synchronize()
        a, got_v, got_x = acq.cpu(), best_v.cpu(), best_x.cpu()
        acq_ref, _, scale = R.jes_mc_group_forward(mom, noise, K, T, S, want_seeds=False)
        ok = torch.isfinite(acq_ref)
        assert torch.equal(ok, torch.isfinite(a)) and bool(((a - acq_ref).abs()[ok] <= 1e-14 * (1.0 + scale[ok])).all())
        want_v, want_x = R1.track_best(a, x, prev_v, prev_x)      # the rule on the values the launch itself computed
        assert torch.equal(_bits(got_v), _bits(want_v)) and torch.equal(got_x, want_x)
        moved = a > prev_v
        if call == 0:
            assert bool(torch.isnan(a[1])) and float(got_v[1]) == float("-inf") and not bool(got_x[1].any())
            assert bool(torch.isfinite(got_v[0])) and bool(torch.isfinite(got_v[2:]).all()) and int(moved.sum()) == T - 1
        if call == 1:
            assert bool(torch.isnan(a[0])) and float(got_v[0]) == float(prev_v[0]) and torch.equal(got_x[0], prev_x[0])
            assert bool(moved[1]) and bool(torch.isfinite(got_v).all())
        if call >= 1:
            assert 0 < int(moved.sum()) < T


def test_jes_mc_group_forward_refuses_bad_arguments():
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as F
    z = lambda *s: torch.ones(*s, dtype=torch.float64, device=DEV)
    acq = z(1)
    with pytest.raises(_lib.MobocmfError):
        F.jes_mc_group_forward(z(4, 2, 1), z(4), 0, 1, 1, acq)           # K = 0
    with pytest.raises(_lib.MobocmfError):
        F.jes_mc_group_forward(z(66, 2, 1), z(66), 2, 1, 1, acq)         # 22 black-boxes x 3 models = 66 > 64
    with pytest.raises(_lib.MobocmfError):
        F.jes_mc_group_forward(z(5, 2, 1), z(5), 2, 1, 1, acq)           # not a multiple of 1 + K
    F.jes_mc_group_forward(z(64, 2, 1), z(64), 1, 1, 1, acq)             # 64 models: the most
    F.jes_mc_group_forward(z(64, 2, 1), z(64), 63, 1, 1, acq)
    torch.cuda.synchronize()
    assert float(acq[0]) == 0.0


# ------------------------------------------------------------------ 4. the engine at a fixed X, and against the host loop
_models_cache = {}


def _models(M, seed):
    """Two black-boxes x (unconditioned, two conditioned): the six models of tests/test_hip_acq_search.py, made once."""
    if (M, seed) not in _models_cache:
        from tests.test_hip_acq_search import _six_models
        _models_cache[(M, seed)] = _six_models(M, seed)
    return _models_cache[(M, seed)]


def _acq_over(models, groups, K=2):
    """A JESMOC_MFDGP over ``models`` (1 + K per black-box) whose coupled_acq evaluates through ``groups`` {(fidelity, T): group}."""
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP, _JES_MFDGP
    acq = JESMOC_MFDGP.__new__(JESMOC_MFDGP)
    acq.num_pareto_samples, acq.num_fidelities, acq.eval_highest_fidelity = K, 2, False
    acq.standard_bounds = torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device=DEV)
    boxes = [models[i:i + 1 + K] for i in range(0, len(models), 1 + K)]
    acq.objectives = {f: {"bb%d" % p: _JES_MFDGP(f, b[0], b[1:]) for p, b in enumerate(boxes)} for f in (0, 1)}
    acq.constraints = {0: {}, 1: {}}
    acq._tiny_groups = {(f, T, 2): grp for (f, T), grp in groups.items()}
    return acq


@pytest.mark.parametrize("M,seed", [(24, 100), (64, 200)], ids=["M24_one_workgroup", "M64_cooperative"])
@pytest.mark.parametrize("fidelity", [0, 1])
def test_engine_scores_what_coupled_acq_returns(M, seed, fidelity):
    """DeviceAcqSearch._score and JESMOC_MFDGP.coupled_acq at the same X over the SAME group: equal moments, so the values differ
    by the roundings of the two expressions; the input gradient the engine's seeds give (summed over the models) against
    autograd through the group."""
    from mobocmf_amd import _lib
    from mobocmf_amd.util.acq_search import DeviceAcqSearch
    from tests.test_hip_acq_search import _group
    models, T, K = _models(M, seed), 5, 2
    grp = _group(models, fidelity, T)
    acq = _acq_over(models, {(fidelity, T): grp})
    assert acq._group_models(list(acq.objectives[fidelity].values())) == models
    X = torch.rand(T, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(M + fidelity)).to(DEV)
    eng = DeviceAcqSearch(grp, acq.standard_bounds, T, 0.02, num_pareto_samples=K)
    with pytest.raises(_lib.MobocmfError):
        DeviceAcqSearch(grp, acq.standard_bounds, T, 0.02, num_pareto_samples=3)      # six models are no multiple of 1 + 3
    grp.x.copy_(X)
    eng.best_v.fill_(float("-inf"))
    eng._score(seeds=True)
    grp._launch(_lib.STEP_INPUT_GRADIENTS)
    torch.cuda.synchronize()
    got_v, got_g = eng.acq.clone(), grp.gx.sum(0)
    _, _, scale = R.jes_mc_group_forward(grp.moments.cpu(), eng.noise.cpu(), K, T, grp.S, want_seeds=False)
    Xg = X.clone().requires_grad_(True)
    val = acq.coupled_acq(Xg, fidelity=fidelity)
    val.sum().backward()
    err = (got_v - val.detach()).abs().cpu()
    hard = M >= 48      # (d = 2) tests/test_hip_coop_step.py: cond(K_mm + 1e-6 I) ~ 1e9 where dozens of inducing points crowd [0, 1]^2
    print("engine at a fixed X: M", M, "fidelity", fidelity, "value err / bound", float((err / (1e-14 * (1.0 + scale))).max()),
          "gradient rel", _rel(got_g, Xg.grad))
    assert float(val.detach().abs().max()) > 0.0
    assert bool((err <= 1e-14 * (1.0 + scale)).all())
    assert torch.equal(eng.best_v, got_v) and torch.equal(eng.best_x, X)
    assert _rel(got_g, Xg.grad) < (1e-4 if hard else 1e-6)


@pytest.mark.parametrize("M,seed", [(24, 100), (64, 200)], ids=["M24_one_workgroup", "M64_cooperative"])
@pytest.mark.parametrize("fidelity", [0, 1])
def test_engine_parity_at_short_horizon_with_two_samples(M, seed, fidelity):
    """DeviceAcqSearch(num_pareto_samples=2) against optimize_acqf_multistart on the expression coupled_acq evaluates over the
    same groups, from equal generator states: 5 restarts of 200 raw candidates, 10 iterations."""
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import optimize_acqf_multistart
    from mobocmf_amd.util.acq_search import DeviceAcqSearch
    from tests.test_hip_acq_search import _group
    models, K = _models(M, seed), 2
    groups = {T: _group(models, fidelity, T) for T in (200, 5)}
    acq = _acq_over(models, {(fidelity, T): g for T, g in groups.items()})
    bounds = acq.standard_bounds
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)
    calls = []

    def acq_fn(X):
        out = acq.coupled_acq(X, fidelity=fidelity)
        calls.append(((X[:, 0, :] if X.dim() > 2 else X).detach().clone(), out.detach().clone()))
        return out

    def freeze(on):
        for grp in groups.values():
            grp.freeze() if on else grp.thaw()

    freeze(True)
    cand_h, val_h = optimize_acqf_multistart(acq_fn, bounds, num_restarts=5, raw_samples=200, maxiter=10, generator=gen())
    freeze(False)
    raw = calls[0][1].cpu()
    top = torch.sort(raw, descending=True).values[:6]
    # precondition (torch.topk's tie order is unspecified, JES is exactly 0 on part of the box): the restarts are well defined
    assert float(top[4]) > 0.0 and len(set(top.tolist())) == 6, top
    assert len(calls) == 12      # the raw candidates, X_0 ... X_10
    best_x, best_v = calls[1][0].clone(), calls[1][1].clone()
    for X, v in calls[2:]:       # the host loop's own tracking, on its own evaluations
        better = v > best_v
        best_v = torch.where(better, v, best_v)
        best_x[better] = X[better]

    eng = DeviceAcqSearch(groups[5], bounds, 5, 0.02, num_pareto_samples=K)
    res = {}
    for graphed in (True, False):
        eng.use_graph = graphed
        Xraw = bounds[0] + (bounds[1] - bounds[0]) * torch.rand(200, 2, dtype=torch.float64, device=DEV, generator=gen())
        assert torch.equal(Xraw, calls[0][0])
        raw_d, top_v, top_i = eng.start_from_raw(groups[200], Xraw)
        if graphed:
            assert torch.equal(top_i.cpu(), torch.topk(raw, 5).indices) and torch.equal(groups[5].x, calls[1][0])
            assert _rel(raw_d, raw) <= PARITY_TOL
        cand, val = eng.run(None, 10)
        freeze(False)
        res[graphed] = [t.clone() for t in (cand, val, eng.best_x, eng.best_v, eng.steps_done, groups[5].x)]
        assert int(eng.steps_done[0]) == 10
        assert not bool(eng.info_words().any())
    assert len(eng._graphs) == 1
    for a, b in zip(res[True], res[False]):      # graphed and eager: the same launches
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
    cand, val, bx, bv = res[True][:4]
    diffs = dict(best_x=_rel(bx, best_x), best_v=_rel(bv, best_v), candidate=_rel(cand, cand_h), value=_rel(val, val_h))
    print("engine parity K = 2, M = %d fidelity %d: largest relative differences" % (M, fidelity), diffs)
    assert max(diffs.values()) <= PARITY_TOL, diffs
    assert bool((bv.cpu() >= top_v.cpu()).all())      # X_0 is scored too


# ------------------------------------------------------------------ 5. through the public surface
_toy = {}
_BOXES = (("obj1", False), ("obj2", False), ("con1", True))


def _params(fitter):
    return [p.detach().clone() for _, _, h in fitter._handlers() for p in h.mfdgp.parameters()]


def _add_boxes(acq):
    for f in range(2):
        for name, is_con in _BOXES:
            acq.add_blackbox(f, name, cost_evaluation=1.0 if f == 0 else 10.0, is_constraint=is_con)
    return acq


def _toy_acq():
    """One toy BO iteration (examples/bo_iteration_toy2d.py, 14 + 6 points) with K = 3 Pareto samples, made once; the fitter as
    it was handed to the acquisition (unconditioned, holding sample 0's Pareto solution) is kept aside."""
    if not _toy:
        from bo_iteration_toy2d import run
        from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
        original = BlackBoxMFDGPFitter.conditioned_copies

        def recording(self, K, seed=None, **kw):
            _toy["before"] = self.copy_uncond()
            return original(self, K, seed=seed, **kw)

        BlackBoxMFDGPFitter.conditioned_copies = recording
        try:
            _toy["fitter"], _toy["acq"] = run(epochs=60, cond_iters=30, acq_iters=8, grid=40, seed=0, verbose=False,
                                              pareto_samples=3, pareto_seed=1)[:2]
        finally:
            BlackBoxMFDGPFitter.conditioned_copies = original
    return _toy["acq"]


def _next_point(acq, engine, seed=5):
    acq.search = engine
    return acq.get_nextpoint_coupled(maxiter=20, generator=torch.Generator(device=DEV).manual_seed(seed))


def test_three_pareto_samples_three_conditioned_fits():
    acq = _toy_acq()
    assert acq.num_pareto_samples == 3 and len(acq.pareto_sets) == len(acq.pareto_fronts) == 3
    conds = acq.blackbox_mfdgp_fitters_cond
    assert len(conds) == 3 and conds[0] is _toy["fitter"] is acq.blackbox_mfdgp_fitter_cond
    assert len({id(c) for c in conds} | {id(acq.blackbox_mfdgp_fitter_uncond)}) == 4
    assert acq.pareto_set is acq.pareto_sets[0] and acq.pareto_front is acq.pareto_fronts[0]
    for k in range(3):
        assert conds[k].pareto_set is acq.pareto_sets[k] and acq.pareto_sets[k].shape[0] >= 1
        for j in range(k):      # three different samples
            assert acq.pareto_sets[k].shape != acq.pareto_sets[j].shape or not torch.equal(acq.pareto_sets[k], acq.pareto_sets[j])
    assert torch.equal(acq.pareto_sets[0], _toy["before"].pareto_set)      # sample 0: the solution the fitter already held
    before = _params(_toy["before"])
    assert all(torch.equal(a, b) for a, b in zip(_params(acq.blackbox_mfdgp_fitter_uncond), before))
    for k in range(3):           # every conditioned fitter has moved away from the unconditioned fit, each to its own place
        pk = _params(conds[k])
        assert any(not torch.equal(a, b) for a, b in zip(pk, before))
        for j in range(k):
            assert any(not torch.equal(a, b) for a, b in zip(pk, _params(conds[j])))
    jes = acq.objectives[1]["obj1"]
    assert len(jes.mfdgp_conds) == 3 and jes.mfdgp_cond is conds[0].get_model("obj1")
    assert [id(m) for m in jes.mfdgp_conds] == [id(c.get_model("obj1")) for c in conds]


def test_coupled_acq_is_the_mean_over_the_samples():
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP
    acq = _toy_acq()
    X = torch.rand(16, 2, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(16))
    singles = [_add_boxes(JESMOC_MFDGP(model=acq.blackbox_mfdgp_fitter_uncond, num_fidelities=2, model_cond=c,
                                       standard_bounds=acq.standard_bounds)) for c in acq.blackbox_mfdgp_fitters_cond]
    listed = _add_boxes(JESMOC_MFDGP(model=acq.blackbox_mfdgp_fitter_uncond, num_fidelities=2,
                                     model_cond=tuple(acq.blackbox_mfdgp_fitters_cond), standard_bounds=acq.standard_bounds))
    assert listed.num_pareto_samples == 3 and all(s.num_pareto_samples == 1 for s in singles)
    for f in (0, 1):
        with torch.no_grad():
            vals = []
            for s in singles:
                s.use_tiny_step = False
                vals.append(s.coupled_acq(X, fidelity=f))
            mean = (1.0 / 3) * ((vals[0] + vals[1]) + vals[2])
            acq.use_tiny_step = listed.use_tiny_step = False
            layer = acq.coupled_acq(X, fidelity=f)
            layer_listed = listed.coupled_acq(X, fidelity=f)
            acq.use_tiny_step = True
            grouped = acq.coupled_acq(X, fidelity=f)
        assert float(mean.abs().max()) > 0.0 and any(not torch.equal(vals[0], v) for v in vals[1:])
        print("coupled_acq K = 3 fidelity", f, "layer path vs mean of singles", _rel(layer, mean), "group vs mean", _rel(grouped, mean))
        assert _rel(layer, mean) <= 1e-13
        assert torch.equal(layer_listed, layer)      # model_cond as a tuple: the same object as num_pareto_samples = 3 built
        assert len(acq._tiny_groups[(f, 16, 2)].models) == 12
        assert _rel(grouped, mean) < GROUP_VS_LAYER


def test_device_search_with_three_samples_through_the_public_surface():
    acq = _toy_acq()
    lo, hi = acq.standard_bounds[0], acq.standard_bounds[1]
    cand, fid = _next_point(acq, "device")
    assert acq.last_search_engine == {0: "device", 1: "device"}
    assert cand.shape == (2,) and bool((cand >= lo).all()) and bool((cand <= hi).all())
    for f in (0, 1):
        eng = acq._device_searches[f]
        assert eng.K == 3 and len(eng.group.models) == 12 and int(eng.steps_done[0]) == 20
        assert acq.last_search_values[f] >= float(eng.raw_values.max())       # not below the best raw candidate
    val = acq.last_search_values[fid]
    again = float(acq.coupled_acq(cand[None], fidelity=fid)[0])      # the eager path (a group for T = 1)
    assert val > 0.0 and abs(val - again) <= GROUP_VS_LAYER * abs(again), (val, again)
    cand2, fid2 = _next_point(acq, "device")
    assert fid2 == fid and torch.equal(_bits(cand2), _bits(cand))
    acq.search = "host"


def test_too_many_models_for_the_device_engine_run_the_host_loop(monkeypatch):
    """3 black-boxes x (1 + 3) models against a bound of 2 x 5 (the library's is 2 x 32: 65 models are not built here)."""
    from mobocmf_amd import _lib
    acq = _toy_acq()
    monkeypatch.setattr(_lib, "ACQ_MAX_PAIRS", 5)
    acq.search = "device"
    cand, fid = acq.get_nextpoint_coupled(maxiter=2, generator=torch.Generator(device=DEV).manual_seed(5))
    assert acq.last_search_engine == {0: "host", 1: "host"}
    assert bool((cand >= acq.standard_bounds[0]).all()) and bool((cand <= acq.standard_bounds[1]).all())
    monkeypatch.setattr(_lib, "ACQ_MAX_PAIRS", 6)      # 12 models: exactly the bound
    acq.get_nextpoint_coupled(maxiter=2, generator=torch.Generator(device=DEV).manual_seed(5))
    assert acq.last_search_engine == {0: "device", 1: "device"}
    acq.search = "host"


def test_one_sample_is_the_default_and_zero_is_refused():
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP
    _toy_acq()
    with pytest.raises(ValueError):
        JESMOC_MFDGP(model=_toy["before"], num_fidelities=2, num_pareto_samples=0)
    with pytest.raises(ValueError):
        _toy["before"].conditioned_copies(0)
    cands = []
    for kw in (dict(), dict(num_pareto_samples=1)):
        fitter = _toy["before"].copy_uncond()
        torch.manual_seed(3)
        np.random.seed(3)
        acq = _add_boxes(JESMOC_MFDGP(model=fitter, num_fidelities=2, search="device",
                                      standard_bounds=_toy["acq"].standard_bounds, **kw))
        assert acq.num_pareto_samples == 1 and acq.blackbox_mfdgp_fitters_cond == [fitter] and acq.pareto_sets[0] is acq.pareto_set
        assert torch.equal(acq.pareto_set, _toy["before"].pareto_set)
        cands.append(_next_point(acq, "device"))
        assert acq.last_search_engine == {0: "device", 1: "device"} and acq._device_searches[1].K == 1
    assert cands[0][1] == cands[1][1] and torch.equal(_bits(cands[0][0]), _bits(cands[1][0]))
