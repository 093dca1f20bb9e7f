"""The acquisition search on the device (csrc/acq_search.hip, util/acq_search.py, JESMOC_MFDGP(search="device")): the three
kernels against their float64 restatements (tests/acq_search_reference.py), the search engine against the host loop
(optimize_acqf_multistart over the same predict groups), and the engine through the public surface."""
import os
import sys

import pytest
import torch

from mobocmf_amd.util import synthetic
from tests import acq_search_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

# Device engine against host engine: the two differ only in summation order (the moments over the S samples, the sum over the
# models' input gradients, the sum over the pairs) -- an ulp in the first gradient.  Once the iterates differ by an ulp, the model
# kernels' own rounding noise enters: M = 64 inducing points crowd [0, 1]^2 (cond(K_mm + 1e-6 I) ~ 1e9), and two evaluations at
# inputs an ulp apart differ by far more than the inputs do.  D, the largest relative difference over best_x, best_v, the candidate
# and its value at the sizes of test_engine_parity_at_short_horizon, measured on an MI355X: exactly 0 at fidelity 0
# (S = 1), 3.6e-11 at M = 24 and 1.37e-10 at M = 64, fidelity 1.  Asserted at 100 D.
D_MEASURED = 1.4e-10
PARITY_TOL = 100.0 * D_MEASURED


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


# ------------------------------------------------------------------ 1. mobocmf_jes_group_forward
def _jes_inputs(n_pairs, T, S, seed, flip):
    """Means ~ N(0, 1), variances ~ U(0.05, 2), noise ~ U(1e-3, 0.1); the conditioned model of pair p at test point t is
    rescaled so that v_c is about 2 v_u where (p + t + flip) is even (clamped: zero seeds) and about v_u / 2 elsewhere."""
    g = torch.Generator().manual_seed(seed)
    n = 2 * n_pairs
    mom = torch.empty(n, 2, T * S, dtype=torch.float64)
    mom[:, 0] = torch.randn(n, T * S, dtype=torch.float64, generator=g)
    mom[:, 1] = 0.05 + 1.95 * torch.rand(n, T * S, dtype=torch.float64, generator=g)
    noise = 1e-3 + 0.099 * torch.rand(n, dtype=torch.float64, generator=g)
    v, _ = R.model_v(mom, noise, T, S)
    vu, vc, tc = v[0::2], v[1::2], noise[1::2, None]
    even = ((torch.arange(n_pairs)[:, None] + torch.arange(T)[None, :] + flip) % 2) == 0
    r = torch.where(even, torch.tensor(2.0, dtype=torch.float64), torch.tensor(0.5, dtype=torch.float64))
    c2 = torch.maximum(r * vu - tc, 0.01 * vu) / (vc - tc)       # v_c -> c2 (v_c - tau_c) + tau_c
    c2 = c2[:, :, None].expand(n_pairs, T, S).reshape(n_pairs, T * S)
    mom[1::2, 0] *= c2.sqrt()
    mom[1::2, 1] *= c2
    return mom, noise


@pytest.mark.parametrize("n_pairs,T,S", [(1, 1, 1), (3, 5, 4), (2, 67, 1), (3, 200, 5)])
def test_jes_group_forward_matches_the_reference(n_pairs, T, S):
    from mobocmf_amd import functional as F
    kinds = set()
    for flip in (0, 1):      # complementary patterns: both kinds of pairs occur at every shape, also at (1, 1, 1)
        mom, noise = _jes_inputs(n_pairs, T, S, seed=10 * T + S, flip=flip)
        acq_ref, seeds_ref, scale = R.jes_group_forward(mom, noise, T, S)
        v, _ = R.model_v(mom, noise, T, S)
        clamped = v[1::2] > v[0::2]
        kinds |= set(clamped.reshape(-1).tolist())
        assert bool((seeds_ref[0::2, 1].reshape(n_pairs, T, S)[clamped] == 0.0).all())
        assert bool((seeds_ref[0::2, 1].reshape(n_pairs, T, S)[~clamped] > 0.0).all())
        md, nd = mom.to(DEV), noise.to(DEV)
        acq = torch.full((T,), float("nan"), dtype=torch.float64, device=DEV)
        seeds = torch.full_like(md, float("nan"))
        F.jes_group_forward(md, nd, T, S, acq, seeds=seeds)
        acq2 = torch.full_like(acq, float("nan"))
        F.jes_group_forward(md, nd, T, S, acq2)      # want_seeds = 0: the same values, nothing else written
        torch.cuda.synchronize()
        err = (acq.cpu() - acq_ref).abs()
        print("jes_group_forward", (n_pairs, T, S), "flip", flip, "acq err / bound", float((err / (1e-14 * (1.0 + scale))).max()),
              "seeds rel", float((seeds.cpu() - seeds_ref).abs().max() / seeds_ref.abs().max().clamp_min(1e-300)))
        assert bool((err <= 1e-14 * (1.0 + scale)).all())
        assert torch.equal(_bits(acq), _bits(acq2))
        assert float((seeds.cpu() - seeds_ref).abs().max()) <= 1e-12 * float(seeds_ref.abs().max())
    assert kinds == {True, False}


def test_jes_group_forward_tracks_the_best_iterate():
    """track = 1 over three calls with different iterates: the element-wise larger value and its row stay (the comparison is
    strict), the -inf the caller starts from is replaced by any finite value, a NaN value never replaces anything."""
    from mobocmf_amd import functional as F
    n_pairs, T, S, d = 2, 70, 2, 3
    g = torch.Generator().manual_seed(2)
    best_v = torch.full((T,), float("-inf"), dtype=torch.float64, device=DEV)
    best_x = torch.zeros(T, d, dtype=torch.float64, device=DEV)
    acq = torch.zeros(T, dtype=torch.float64, device=DEV)
    for call in range(3):
        mom, noise = _jes_inputs(n_pairs, T, S, seed=20 + call, flip=call % 2)
        if call == 0:
            mom[0, 1, S:2 * S] = float("nan")      # test point 1: no value on the first call
        if call == 1:
            mom[0, 1, :S] = float("nan")           # test point 0: no value on the second
        x = torch.rand(T, d, dtype=torch.float64, generator=g)
        prev_v, prev_x = best_v.cpu(), best_x.cpu()
        F.jes_group_forward(mom.to(DEV), noise.to(DEV), T, S, acq, x=x.to(DEV), best_v=best_v, best_x=best_x)
        torch.cuda.synchronize()
        a, got_v, got_x = acq.cpu(), best_v.cpu(), best_x.cpu()
        acq_ref, _, scale = R.jes_group_forward(mom, noise, T, S, want_seeds=False)
        ok = torch.isfinite(acq_ref)
        assert torch.equal(ok, torch.isfinite(a)) and bool(((a - acq_ref).abs()[ok] <= 1e-14 * (1.0 + scale[ok])).all())
        want_v, want_x = R.track_best(a, x, prev_v, prev_x)      # the rule on the values the launch itself computed
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


# ------------------------------------------------------------------ 2. mobocmf_ascent_adam_step
@pytest.mark.parametrize("T,d", [(1, 1), (5, 2), (67, 8)])
def test_ascent_adam_step_is_fused_adam_then_clamp_bit_for_bit(T, d):
    from mobocmf_amd import functional as F
    g = torch.Generator().manual_seed(T + d)
    lo = (0.2 + 0.1 * torch.rand(d, dtype=torch.float64, generator=g)).to(DEV)
    hi = (0.7 + 0.1 * torch.rand(d, dtype=torch.float64, generator=g)).to(DEV)
    x0 = (lo.cpu() + (hi - lo).cpu() * torch.rand(T, d, dtype=torch.float64, generator=g)).to(DEV)
    lr = 0.15
    p = x0.clone().requires_grad_(True)
    opt = F.FusedAdam([p], lr=lr)
    x, m, v = x0.clone(), torch.zeros_like(x0), torch.zeros_like(x0)
    steps = torch.zeros(1, dtype=torch.int64, device=DEV)
    clipped = 0
    for it in range(10):
        gx = torch.randn(1, T, d, dtype=torch.float64, generator=g).sign().to(DEV) * (0.5 + it)      # a steady push to the walls
        p.grad = -gx[0]
        opt.step()
        with torch.no_grad():
            clipped += int(((p < lo) | (p > hi)).sum())
            p.clamp_(min=lo, max=hi)
        F.ascent_adam_step(x, gx, lo, hi, m, v, steps, lr)
        assert torch.equal(_bits(x), _bits(p)), it
    assert clipped > 0 and int(steps[0]) == 10 and int(opt.steps_done) == 10
    assert torch.equal(_bits(m), _bits(opt.state[0]["exp_avg"])) and torch.equal(_bits(v), _bits(opt.state[0]["exp_avg_sq"]))


def test_ascent_adam_step_sums_the_models_in_order():
    from mobocmf_amd import functional as F
    g = torch.Generator().manual_seed(8)
    T, d, n_models, lr = 67, 8, 6, 0.05
    lo, hi = torch.full((d,), 0.1, dtype=torch.float64), torch.linspace(0.6, 0.9, d, dtype=torch.float64)
    x = lo + (hi - lo) * torch.rand(T, d, dtype=torch.float64, generator=g)
    m, v = torch.zeros(T, d, dtype=torch.float64), torch.zeros(T, d, dtype=torch.float64)
    xd, md, vd = x.to(DEV), m.to(DEV), v.to(DEV)
    steps = torch.zeros(1, dtype=torch.int64, device=DEV)
    worst = 0.0
    for step in range(1, 11):
        gx = torch.randn(n_models, T, d, dtype=torch.float64, generator=g)
        x, m, v = R.ascent_adam_step(x, gx, lo, hi, m, v, step, lr)
        F.ascent_adam_step(xd, gx.to(DEV), lo.to(DEV), hi.to(DEV), md, vd, steps, lr)
        worst = max(worst, _rel(xd, x))
    print("ascent_adam_step n_models = 6: largest relative difference", worst)
    assert worst <= 1e-15 and int(steps[0]) == 10
    assert bool((x == lo).any()) or bool((x == hi).any())


# ------------------------------------------------------------------ 3. mobocmf_select_topk
@pytest.mark.parametrize("n,k", [(200, 5), (5, 5), (4096, 64), (7, 1)])
@pytest.mark.parametrize("d", [1, 8])
def test_select_topk_matches_the_reference(n, k, d):
    from mobocmf_amd import functional as F
    g = torch.Generator().manual_seed(n + k + d)
    vals = torch.randint(0, max(2, n // 3), (n,), generator=g).double() * 0.25 - 3.0      # repeated values
    vals[-min(2, n - 1):] = float("nan")                                                   # trailing NaNs
    if n > 6:
        vals[3] = float("-inf")
    x = torch.randn(n, d, dtype=torch.float64, generator=g)
    want_v, want_i, want_x = R.select_topk(vals, k, x)
    assert len(set(vals[:-2].tolist())) < n - 2 or n <= 7
    out_v = torch.zeros(k, dtype=torch.float64, device=DEV)
    out_i = torch.zeros(k, dtype=torch.int64, device=DEV)
    out_x = torch.zeros(k, d, dtype=torch.float64, device=DEV)
    F.select_topk(vals.to(DEV), k, out_v, out_i, x=x.to(DEV), out_x=out_x)
    assert torch.equal(out_i.cpu(), want_i)
    assert torch.equal(_bits(out_v), _bits(want_v)) and torch.equal(out_x.cpu(), want_x)
    out_v2, out_i2 = torch.zeros_like(out_v), torch.zeros_like(out_i)
    F.select_topk(vals.to(DEV), k, out_v2, out_i2)      # without rows
    assert torch.equal(out_i2, out_i) and torch.equal(_bits(out_v2), _bits(out_v))
    if k == n:
        assert bool(torch.isnan(out_v[-1]))              # NaN last


# ------------------------------------------------------------------ 4. engine parity at short horizon
def _six_models(M, seed):
    from tests.test_hip_model import build_model
    return [build_model(synthetic.make_problem(d=2, L=2, M=M, N=M, S=5, seed=seed + i), S_train=1, S_acq=5) for i in range(6)]


def _group(models, fidelity, T):
    from mobocmf_amd.util.coop_step import CoopPredictGroup
    from mobocmf_amd.util.tiny_step import TinyPredictGroup
    M = models[0].hidden_layer_0.variational_strategy._inducing_points.shape[0]
    return (TinyPredictGroup if M <= 32 else CoopPredictGroup)(models, fidelity, T, 2)


@pytest.mark.parametrize("M,seed", [(24, 100), (64, 200)], ids=["M24_one_workgroup", "M64_cooperative"])
@pytest.mark.parametrize("fidelity", [0, 1])
def test_engine_parity_at_short_horizon(M, seed, fidelity):
    """DeviceAcqSearch, graphed and eager, against optimize_acqf_multistart on the expression coupled_acq evaluates over the
    same groups, from equal generator states: 5 restarts of 200 raw candidates, 10 iterations."""
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import optimize_acqf_multistart
    from mobocmf_amd.util.acq_search import DeviceAcqSearch
    models = _six_models(M, seed)
    groups = {T: _group(models, fidelity, T) for T in (200, 5)}
    bounds = torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device=DEV)
    gen = lambda: torch.Generator(device=DEV).manual_seed(11)
    calls = []

    def acq_fn(X):
        X2 = X[:, 0, :] if X.dim() > 2 else X
        _, v = groups[X2.shape[0]].acquisition_moments(X2)
        out = (0.5 * torch.clamp(torch.log(v[0::2]) - torch.log(v[1::2]), min=0.0)).sum(0)
        calls.append((X2.detach().clone(), out.detach().clone()))
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
    assert torch.equal(cand_h[0], best_x[int(torch.argmax(best_v))]) and torch.equal(val_h, best_v.max())

    eng = DeviceAcqSearch(groups[5], bounds, 5, 0.02)
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
    print("engine parity M = %d fidelity %d: largest relative differences" % (M, fidelity), diffs)
    assert max(diffs.values()) <= PARITY_TOL, diffs
    assert bool((bv.cpu() >= top_v.cpu()).all())      # X_0 is scored too


# ------------------------------------------------------------------ 5. / 6. through the public surface
_TOY = {"M20_one_workgroup": dict(), "M48_cooperative": dict(n_low=34, n_high=14)}
_toy_cache = {}


def _toy_acq(kind):
    """The acquisition object of one toy BO iteration (examples/bo_iteration_toy2d.py), made once per size."""
    if kind not in _toy_cache:
        from bo_iteration_toy2d import run
        _toy_cache[kind] = run(epochs=60, cond_iters=30, acq_iters=8, grid=40, seed=0, verbose=False, **_TOY[kind])[1]
    return _toy_cache[kind]


def _next_point(acq, engine, seed=5, highest=False):
    acq.search = engine
    fn = acq._get_nextpoint_coupled_highest_fidelity if highest else acq.get_nextpoint_coupled
    return fn(maxiter=20, generator=torch.Generator(device=DEV).manual_seed(seed))


@pytest.mark.parametrize("kind", list(_TOY))
def test_device_search_through_the_public_surface(kind):
    from mobocmf_amd.util.coop_step import CoopPredictGroup
    acq = _toy_acq(kind)
    lo, hi = acq.standard_bounds[0], acq.standard_bounds[1]
    Xs = [torch.rand(T, 2, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(T)) for T in (5, 16)]
    before = [acq.coupled_acq(X, fidelity=f).clone() for f in (0, 1) for X in Xs]
    cand_h, fid_h = _next_point(acq, "host")
    assert acq.last_search_engine == {0: "host", 1: "host"}
    cand_d, fid_d = _next_point(acq, "device")
    assert acq.last_search_engine == {0: "device", 1: "device"}
    print("public surface: host", cand_h.tolist(), fid_h, "device", cand_d.tolist(), fid_d, "rel", _rel(cand_d, cand_h))
    assert fid_d == fid_h
    assert _rel(cand_d, cand_h) <= PARITY_TOL
    assert cand_d.shape == (2,) and bool((cand_d >= lo).all()) and bool((cand_d <= hi).all())
    val_d = acq.last_search_values[fid_d]
    again = float(acq.coupled_acq(cand_d[None], fidelity=fid_d)[0])      # the eager path (a group for T = 1)
    assert abs(val_d - again) <= 1e-9 * abs(again), (val_d, again)
    for f in (0, 1):
        eng = acq._device_searches[f]
        assert acq.last_search_values[f] >= float(eng.raw_values.max())       # not below the best raw candidate
        assert int(eng.steps_done[0]) == 20
    cooperative = [g for g in acq._tiny_groups.values() if isinstance(g, CoopPredictGroup)]
    assert all(isinstance(acq._device_searches[f].group, CoopPredictGroup) == (kind == "M48_cooperative") for f in (0, 1))
    assert acq._device_searches[1].raw_group.T < acq.raw_samples == acq._device_searches[0].raw_group.T      # 200 x 25 columns: chunks
    assert all(not g._frozen and not g._chain_ready for g in cooperative)
    after = [acq.coupled_acq(X, fidelity=f) for f in (0, 1) for X in Xs]
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    acq.search = "host"


def test_device_search_reports_an_abandoned_wait_and_recovers():
    """With the status word of the search group set every in-launch wait gives up at its first poll (nothing hangs): the call
    raises at thaw() and returns no candidate; the next search on the same object is right."""
    from mobocmf_amd import functional as F
    from mobocmf_amd.util.coop_step import CoopPredictGroup
    acq = _toy_acq("M48_cooperative")
    top = acq.num_fidelities - 1
    cand0, fid0 = _next_point(acq, "device", highest=True)
    grp = acq._tiny_groups[(top, acq.num_restarts, 2)]
    assert isinstance(grp, CoopPredictGroup)
    sync = grp.in_launch_sync()
    sync.words[sync.status_index].fill_(1)
    torch.cuda.synchronize()
    got = None
    with pytest.raises(F.InLaunchWaitAbandoned):
        got = _next_point(acq, "device", highest=True)
    assert got is None and not bool(sync.words.any()) and not grp._frozen and not grp._chain_ready
    cand1, fid1 = _next_point(acq, "device", highest=True)
    assert fid1 == fid0 == top and torch.equal(cand1, cand0)
    acq.search = "host"
