"""The exact-GP device fit on the GPU (mobocmf_exact_fit_*, util/exact_fit.py: ExactGPFitStep, fit_exact_gps,
``_ExactMFGP.fit(engine="device")``) against tests/exact_fit_reference.py (which tests/test_exact_fit_cpu.py pins to CPU
autograd) and against the host loop on the torch statement of the likelihood.

Figures measured on the MI355X are recorded where they are asserted: the gradient sums' worst ratio in
tests/exact_fit_reference.py (EXACT_FIT_DEVICE_RATIO_MEASURED), the trajectories' differences in DESIGN.md 5.6.7."""
import copy

import numpy as np
import pytest
import torch

from tests import exact_fit_reference as R
from tests import mes_reference as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = lambda c: "%s-%d-%d-%d" % c      # noqa: E731
SETS = ((24, 2, 2), (130, 3, 3))       # mes_models(n, d, nf, seed=1)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _step(models, lr=0.05, num_iters=1):
    from mobocmf_amd.util.exact_fit import ExactGPFitStep
    return ExactGPFitStep(models, lr, num_iters=num_iters)


# ------------------------------------------------------------------------------------------------------------ 1. covariance
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_covariance_launch_matches_the_torch_statement_and_pads_for_the_factorisation(case):
    ref = R.make_model(*case)
    gpu = copy.deepcopy(ref).to(DEV)
    step = _step([gpu])
    n, npad = case[1], (case[1] + 127) // 128 * 128
    for change in (False, True):
        if change:      # in place, as the update launch writes them: the tables are formed on the device at every launch
            for m in (ref, gpu):
                with torch.no_grad():
                    m.likelihood.raw_noise.add_(0.5)
                    m.covar_module.cov_funct_noise.base_kernel.raw_lengthscale.mul_(1.25)
                    if case[0] == "MFGP_lin":
                        m.covar_module.rho.mul_(-0.5).add_(0.3)
        step.launch_covariance()
        K = step.covariance(0).cpu()
        assert tuple(K.shape) == (npad, npad)
        with torch.no_grad():
            K_ref = ref.covar_module(ref.x_train, ref.x_train) + ref.likelihood.noise * torch.eye(n, dtype=torch.float64)
        err = _rel(K[:n, :n], K_ref)
        print("covariance %s changed=%s: relative error %.3e" % (case, change, err))
        assert err < 1e-12
        assert not bool(K[n:, :n].any()) and not bool(K[:n, n:].any())
        assert torch.equal(K[n:, n:], torch.eye(npad - n, dtype=torch.float64))
    if case[0] == "MFGP_lin":      # the second launch saw the new rho
        assert _rel(K[:n, :n], torch.as_tensor(np.asarray(R.covariance(R.case_of(ref)), np.float64))) < 1e-12


# ------------------------------------------------------------------------------------------- 2. and 3. the gradient launches
_stepped = {}


def _one_step(case):
    """One step of the case's model on the device, and the reference on the device's own alpha and K^-1 (formed once)."""
    if case not in _stepped:
        ref = R.make_model(*case)
        gpu = copy.deepcopy(ref).to(DEV)
        step = _step([gpu])
        step.step()
        w = step.work(0)
        n = case[1]
        alpha, Kinv, sums, slab = w["alpha"].cpu().numpy(), w["Kinv"].cpu().numpy(), w["sums"].cpu().numpy(), w["slab"].cpu().numpy()
        res = step.read(1)
        c = R.case_of(ref)
        S, Rk = R.sums_ref(c, alpha, Kinv)
        _stepped[case] = dict(ref=ref, c=c, n=n, alpha=alpha, Kinv=Kinv, sums=sums, slab=slab, S=S, R=Rk, grads=step.gradients()[0],
                              loss=float(res.losses[0, 0]), info=step.info_word(0).cpu())
    return _stepped[case]


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_gradient_sums_componentwise_on_the_devices_alpha_and_inverse(case):
    s = _one_step(case)
    n = s["n"]
    assert int(s["info"]) == 0 and np.isfinite(s["loss"])
    assert abs(s["loss"] + R.mll_ref(s["c"])) <= 1e-9 * max(1.0, abs(s["loss"]))
    assert not s["alpha"][n:].any()
    total = np.zeros(R.SUMS)
    for row in s["slab"]:      # the update's sum: strip by strip
        total = total + row
    assert np.array_equal(total, s["sums"])
    err = np.abs(R.ld(s["sums"]) - s["S"])
    ratio = R._ratio(err, s["R"])
    print("gradient sums %s: worst |got - ref| / (u R) = %.2f (bound n^2 + C_T = %.0f)" % (case, ratio, n * n + R.EXACT_FIT_CT))
    assert np.all(err <= (n * n + R.EXACT_FIT_CT) * R.ld(R.U) * s["R"])
    d, nl = case[2], case[3]      # what does not exist is exactly zero
    for lo, cnt, size in ((R.S_LS_S, d, R.D_MAX), (R.S_LS_N, d, R.D_MAX), (R.S_SIG, nl, R.L_MAX), (R.S_NTAB, nl, R.L_MAX)):
        assert not s["sums"][lo + cnt:lo + size].any()


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_gradient_of_every_raw_parameter_matches_autograd(case):
    s = _one_step(case)
    ref = copy.deepcopy(s["ref"])
    (-ref.marginal_log_likelihood(hip=False)).backward()
    want = {k: p.grad for k, p in ref.named_parameters()}
    got = s["grads"]
    assert set(got) == set(want) and ("covar_module.rho" in got) == (case[0] == "MFGP_lin")
    for k, b in want.items():
        a = got[k].cpu()
        assert a.shape == b.shape, k
        diff, scale = float((a - b).abs().max()), float(b.abs().max())
        print("d(-mll)/d %s %s: |a - b| = %.3e, max|b| = %.3e" % (k, case, diff, scale))
        assert diff <= 1e-7 * max(1e-6, scale), k


# ----------------------------------------------------------------------------------------- 4. and 5. trajectory, best, restore
_host, _device = {}, {}


def _host_fits(shape, lr):
    """The host loop (fit()'s own, forced onto the torch statement) on the three models of a set: {name: (model, record)}."""
    if (shape, lr) not in _host:
        out = {}
        for name, base in M.mes_models(*shape, seed=1).items():
            m = copy.deepcopy(base).to(DEV)
            orig = m.marginal_log_likelihood
            m.marginal_log_likelihood = lambda hip=None, _o=orig: _o(hip=False)
            rec = {}
            m._fit_host(15, lr, record=rec)
            del m.marginal_log_likelihood
            out[name] = (m, rec)
        _host[(shape, lr)] = out
    return _host[(shape, lr)]


def _device_fits(shape, lr):
    """fit_exact_gps over the three models of a set: (models, result, parameter pointers before the fit)."""
    from mobocmf_amd.util.exact_fit import fit_exact_gps
    if (shape, lr) not in _device:
        models = {k: copy.deepcopy(m).to(DEV) for k, m in M.mes_models(*shape, seed=1).items()}
        ptrs = {k: [p.data_ptr() for p in m.parameters()] for k, m in models.items()}
        _device[(shape, lr)] = (models, fit_exact_gps(models, 15, lr), ptrs)
    return _device[(shape, lr)]


@pytest.mark.parametrize("shape", SETS)
def test_device_fit_follows_the_host_loop(shape):
    host = _host_fits(shape, 0.05)
    for name, base in M.mes_models(*shape, seed=1).items():
        m = copy.deepcopy(base).to(DEV)
        assert m.fit(num_iters=15, lr=0.05, engine="device") is m
        res, (hm, rec) = m.last_fit, host[name]
        assert res.engines == {0: "device"} and tuple(res.losses.shape) == (15, 1)
        with torch.no_grad():
            a, b = float(m._hip_factor().mll), float(hm._hip_factor().mll)
        dl = float((res.losses[:, 0] - torch.tensor(rec["losses"], dtype=torch.float64)).abs().max())
        dp = float((_flat(m) - _flat(hm)).abs().max())
        print("trajectory n = %d %s: final mll %.12g vs %.12g, parameters differ by %.3e, losses by %.3e" % (shape[0], name, a, b, dp, dl))
        assert abs(a - b) < 1e-6 * max(1.0, abs(b))
        assert dp < 1e-6
        for x, y in zip(res.losses[:, 0].tolist(), rec["losses"]):
            assert abs(x - y) <= 1e-9 * max(1.0, abs(y))
        assert a > -rec["losses"][0]      # the fit improved the likelihood


@pytest.mark.parametrize("shape", SETS)
def test_best_iterate_and_restore(shape):
    """lr = 0.5 overshoots: the host loop restores all three models (best at iterations 9 / 10 / 7 and 7 / 10 / 7); lr = 0.05
    descends to the end."""
    host = _host_fits(shape, 0.5)
    models, res, _ = _device_fits(shape, 0.5)
    want = {24: {"o0": 9, "o1": 10, "c0": 7}, 130: {"o0": 7, "o1": 10, "c0": 7}}[shape[0]]
    for name, (hm, rec) in host.items():
        assert rec["restored"] and rec["best_iteration"] == want[name] and rec["final"] > rec["best"] + 0.5, (name, rec)
        dp = float((_flat(models[name]) - _flat(hm)).abs().max())
        print("restore n = %d %s: best at %s (host %d), parameters differ by %.3e" % (shape[0], name, res.best_iteration[name],
                                                                                      rec["best_iteration"], dp))
        assert res.engines[name] == "device" and res.stopped_at[name] is None
        assert res.best_iteration[name] == rec["best_iteration"] and res.restored[name] is True
        assert abs(res.best_loss[name] - rec["best"]) <= 1e-6 * max(1.0, abs(rec["best"]))
        assert dp < 1e-6
    _, res, _ = _device_fits(shape, 0.05)
    for name in host:
        assert res.restored[name] is False and res.best_iteration[name] == 14 and res.stopped_at[name] is None


# ------------------------------------------------------------------------------------------------------------------ 6. stop
def test_a_non_finite_loss_stops_that_model_only():
    from mobocmf_amd.util.exact_fit import fit_exact_gps
    base = M.mes_models(24, 2, 2, seed=1)
    bad, good = copy.deepcopy(base["o1"]).to(DEV), copy.deepcopy(base["o0"]).to(DEV)
    bad.y_train[3] = float("nan")
    before = {k: _bits(_flat(m)) for k, m in (("bad", bad), ("good", good))}
    res = fit_exact_gps({"bad": bad, "good": good}, 5, 0.05)
    assert res.engines == {"bad": "device", "good": "device"}
    assert torch.equal(_bits(_flat(bad)), before["bad"])
    assert res.stopped_at["bad"] == 0 and res.restored["bad"] is False and res.best_iteration["bad"] is None
    assert bool(torch.isnan(res.losses[:, 0]).all())
    alone = copy.deepcopy(base["o0"]).to(DEV)
    alone.fit(num_iters=5, lr=0.05, engine="device")
    assert res.stopped_at["good"] is None and bool(torch.isfinite(res.losses[:, 1]).all())
    assert not torch.equal(_bits(_flat(good)), before["good"]) and torch.equal(_bits(_flat(good)), _bits(_flat(alone)))
    assert res.losses[4, 1] < res.losses[0, 1]


def test_update_launch_on_given_losses_and_a_given_slab():
    """The update entry point alone: loss words 3.0, 2.0, 2.5, NaN, 1.0 and a fixed slab (only the small kernel runs)."""
    from mobocmf_amd import _lib
    m = copy.deepcopy(R.make_model("MFGP_lin", 40, 1, 5)).to(DEV)
    c = R.case_of(m)
    step = _step([m], lr=0.1, num_iters=8)
    slab = step.work(0)["slab"]
    fixed = torch.linspace(-1.0, 1.5, slab.numel(), dtype=torch.float64).reshape(slab.shape)
    slab.copy_(fixed)
    sums = fixed.sum(0).numpy()
    names = R.param_names(m)
    order = [s for s in R.SLOTS if s in names]
    by_name = dict(m.named_parameters())
    cuts = np.cumsum([len(c["raw"][s]) for s in order])[:-1]
    current = lambda: torch.cat([by_name[names[s]].detach().reshape(-1) for s in order]).cpu()      # noqa: E731
    um = R.UpdateModel(np.concatenate([c["raw"][s] for s in order]), 0.1)
    snaps = []
    for loss in (3.0, 2.0, 2.5, float("nan"), 1.0):
        snaps.append(current())
        step.mll_word(0).fill_(-loss)
        step.info_word(0).zero_()
        step.launch_update(_lib.EXACT_FIT_STEP)
        # (the reference's gradient is taken at its CURRENT raw values: the slopes and the rho chain move with them)
        cur = dict(c, raw=dict(zip(order, np.split(np.asarray(um.raw, np.float64), cuts))))
        um.step(loss, 0, np.concatenate([R.chain(cur, sums)[s] for s in order]))
    after = current()
    assert not torch.equal(snaps[0], snaps[1]) and not torch.equal(snaps[2], snaps[3])
    assert torch.equal(_bits(snaps[3]), _bits(snaps[4])) and torch.equal(_bits(snaps[4]), _bits(after))      # nothing moves after the NaN
    assert float((after - torch.as_tensor(np.asarray(um.raw, np.float64))).abs().max()) < 1e-12
    got = step.gradients()[0]
    res = step.read(8)
    assert res.stopped_at[0] == 3 and res.best_iteration[0] == 1 and res.best_loss[0] == 2.0 and res.restored[0] is False
    assert res.losses[:3, 0].tolist() == [3.0, 2.0, 2.5] and bool(torch.isnan(res.losses[3:, 0]).all())
    assert step.iterations == [3] and set(got) == set(names.values())
    step.mll_word(0).fill_(float("nan"))
    step.launch_update(_lib.EXACT_FIT_FINISH)
    res = step.read(8)
    assert res.restored[0] is True and torch.equal(_bits(current()), _bits(snaps[1]))      # as they were before the second call


# ------------------------------------------------------------------------------------------ 7. independence and determinism
def test_models_fitted_together_equal_each_alone_and_two_runs_are_bitwise_equal():
    from mobocmf_amd.util.exact_fit import fit_exact_gps
    small, large = M.mes_models(24, 2, 2, seed=1), M.mes_models(130, 3, 3, seed=1)
    base = {"a": small["o0"], "b": large["o1"], "c": small["c0"]}      # (different n: the grids are sized for the largest)
    runs = []
    for _ in range(2):
        models = {k: copy.deepcopy(m).to(DEV) for k, m in base.items()}
        res = fit_exact_gps(models, 6, 0.05)
        runs.append(({k: _bits(_flat(m)) for k, m in models.items()}, _bits(res.losses)))
    assert all(torch.equal(runs[0][0][k], runs[1][0][k]) for k in base) and torch.equal(runs[0][1], runs[1][1])
    for i, (k, m) in enumerate(base.items()):
        alone = copy.deepcopy(m).to(DEV)
        alone.fit(num_iters=6, lr=0.05, engine="device")
        assert torch.equal(_bits(_flat(alone)), runs[0][0][k]), k
        assert torch.equal(_bits(alone.last_fit.losses[:, 0]), runs[0][1][:, i]), k


# -------------------------------------------------------------------------------------------------------------- 8. fallback
def test_a_model_past_the_limit_is_fitted_by_the_host_loop_and_says_so():
    from mobocmf_amd.util.exact_fit import fit_exact_gps, why_not
    models = {"fits": M.mes_models(24, 2, 2, seed=1, device=DEV)["o0"], "big": M.mes_models(513, 2, 2, seed=1, device=DEV)["o0"]}
    with torch.no_grad():
        start = {k: float(m.marginal_log_likelihood()) for k, m in models.items()}
    res = fit_exact_gps(models, 3, 0.05)
    assert res.engines == {"fits": "device", "big": "host"} and tuple(res.losses.shape) == (3, 2)
    with torch.no_grad():
        for k, m in models.items():
            assert float(m.marginal_log_likelihood()) > start[k], k
            assert abs(float(res.losses[0, res.names.index(k)]) + start[k]) <= 1e-8 * max(1.0, abs(start[k])), k
    reason = why_not(models["big"])
    assert reason.startswith("n = 513 training rows")
    with pytest.raises(RuntimeError) as e:
        models["big"].fit(num_iters=3, engine="device")
    assert reason in str(e.value)


# ------------------------------------------------------------------------------------------------------------- 9. aftermath
@pytest.mark.parametrize("lr", (0.05, 0.5))
def test_the_fitted_models_are_the_callers_own(lr):
    models, res, ptrs = _device_fits(SETS[0], lr)
    for name, m in models.items():
        assert [p.data_ptr() for p in m.parameters()] == ptrs[name]
        assert all(p.grad is None and p.requires_grad for p in m.parameters())
        want = -res.best_loss[name] if res.restored[name] else -res.final_loss[name]
        assert res.restored[name] == (lr == 0.5)
        with torch.no_grad():
            got = float(m.marginal_log_likelihood())
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (name, got, want)
    acq = M.mes_problem(*SETS[0], device=DEV, search="device", models=models)
    cand, fid = acq.get_nextpoint_coupled(maxiter=3, generator=torch.Generator(device=DEV).manual_seed(5))
    assert acq.last_search_engine == {0: "device", 1: "device"}
    assert cand.shape == (2,) and fid in (0, 1) and bool((cand >= 0).all()) and bool((cand <= 1).all())
