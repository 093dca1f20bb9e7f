"""The exact-GP device fit without a GPU: the engine switch of ``_ExactMFGP.fit``, ``why_not``'s sentences, the host-side
validation of the descriptors (mobocmf_exact_fit_work_bytes through ctypes), and the proofs of the tests' own reference
(tests/exact_fit_reference.py): its sums, chained to the raw parameters, against CPU autograd; its single-term rounding, from
which the gate of the GPU test takes C_T; its update rule against fit()'s loop."""
import ctypes

import numpy as np
import pytest
import torch

from tests import exact_fit_reference as R
from tests.mes_reference import mes_models


def test_fit_engine_must_be_host_or_device():
    m = mes_models(8)["o0"]
    with pytest.raises(ValueError):
        m.fit(num_iters=1, engine="bogus")


def test_fit_on_the_device_refuses_a_cpu_model_with_the_sentence_of_why_not():
    from mobocmf_amd.util import exact_fit
    m = mes_models(8)["o1"]
    before = [p.detach().clone() for p in m.parameters()]
    reason = exact_fit.why_not(m)
    assert reason == "the model is not on the GPU"
    with pytest.raises(RuntimeError, match=reason):
        m.fit(num_iters=1, engine="device")
    assert all(torch.equal(a, b) for a, b in zip(before, m.parameters()))


def test_host_engine_is_the_default_and_records_nothing_on_the_model():
    a, b = mes_models(10)["o1"], mes_models(10)["o1"]
    a.fit(num_iters=3, lr=0.05)
    b.fit(num_iters=3, lr=0.05, engine="host")
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert not hasattr(a, "last_fit")


def test_why_not_names_every_limit():
    from mobocmf_amd import gp
    from mobocmf_amd.models.mfgp import MFGP, MFGP_lin
    from mobocmf_amd.util.exact_fit import why_not

    def model(n, d, nf, cls=MFGP):
        g = torch.Generator().manual_seed(n + d)
        x = torch.cat([torch.rand(n, d, generator=g, dtype=torch.float64), (torch.arange(n) % nf).double()[:, None]], 1)
        return cls(x, torch.rand(n, generator=g, dtype=torch.float64), nf)

    ok = model(12, 2, 2)
    assert why_not(ok, on_gpu=False) is None and why_not(model(12, 2, 3, MFGP_lin), on_gpu=False) is None
    assert why_not(ok) == "the model is not on the GPU"
    assert why_not(model(513, 1, 2), on_gpu=False).startswith("n = 513 training rows")
    assert why_not(model(6, 33, 2), on_gpu=False).startswith("d = 33 input columns")
    assert why_not(model(12, 1, 9, MFGP_lin), on_gpu=False).startswith("9 fidelity levels")
    assert why_not(model(12, 2, 2).float(), on_gpu=False) == "not a float64 model"
    other = model(12, 2, 2)
    other.covar_module = gp.ScaleKernel(gp.RBFKernel(ard_num_dims=2))
    assert why_not(other, on_gpu=False) == "not an exact GP with an MFKernel or MFKernel_lin covariance"
    assert why_not(torch.nn.Linear(2, 2), on_gpu=False) == "not an exact GP with an MFKernel or MFKernel_lin covariance"

    class Odd(gp.Positive):
        pass

    odd = model(12, 2, 2)
    odd.likelihood.raw_noise_constraint = Odd()
    assert "constraint the device fit does not know" in why_not(odd, on_gpu=False)


def test_descriptor_validation_is_done_on_the_host():
    from mobocmf_amd import _lib
    lib = _lib.load()

    def rc(n=40, d=3, nl=3, kernel=_lib.EXACT_FIT_KERNEL_LIN, n_models=1, out=True):
        rec, nb = _lib.ExactFitModel(), ctypes.c_size_t(0)
        rec.n, rec.d, rec.n_levels, rec.kernel, rec.cap = n, d, nl, kernel, 5
        return lib.mobocmf_exact_fit_work_bytes(ctypes.byref(rec), n_models, ctypes.byref(nb) if out else None), nb.value

    code, nbytes = rc()
    npad, strips = 128, 3
    assert code == _lib.OK and nbytes >= 8 * (3 * npad * npad + npad + (strips + 1) * _lib.EXACT_FIT_SUMS)
    assert rc(n=512, d=32, nl=8, n_models=64)[0] == _lib.OK
    for bad in (dict(n=0), dict(n=513), dict(d=0), dict(d=33), dict(nl=0), dict(nl=9), dict(n_models=0), dict(n_models=65),
                dict(kernel=2), dict(out=False)):
        assert rc(**bad)[0] == _lib.BAD_ARG, bad
    # the launches validate the whole table before any HIP call: no table, no models, a record with no pointers
    rec = (_lib.ExactFitModel * 1)()
    rec[0].n, rec[0].d, rec[0].n_levels, rec[0].kernel, rec[0].cap = 8, 2, 2, 0, 5
    table = ctypes.cast(rec, ctypes.c_void_p)
    for name in ("mobocmf_exact_fit_covariance", "mobocmf_exact_fit_prepare", "mobocmf_exact_fit_gradient"):
        fn = getattr(lib, name)
        assert fn(None, None, 1, None) == _lib.BAD_ARG and fn(table, table, 0, None) == _lib.BAD_ARG
        assert fn(table, table, 65, None) == _lib.BAD_ARG and fn(table, table, 1, None) == _lib.BAD_ARG
    assert lib.mobocmf_exact_fit_update(table, table, 1, _lib.EXACT_FIT_STEP, 0.05, 0.9, 0.999, 1e-8, None) == _lib.BAD_ARG


def test_python_constants_match_the_header():
    """The relations between the constants; their values are the compiler's (tests/test_abi_cpu.py)."""
    from mobocmf_amd import _lib
    assert _lib.EXACT_FIT_SUMS == 2 * (_lib.MAX_D + 1) + 1 + 2 * _lib.EXACT_FIT_MAX_LEVELS == R.SUMS
    assert _lib.EXACT_FIT_MAX_MODELS == 2 * _lib.ACQ_MAX_PAIRS
    assert (_lib.EXACT_FIT_S_OS_S, _lib.EXACT_FIT_S_LS_S, _lib.EXACT_FIT_S_OS_N, _lib.EXACT_FIT_S_LS_N, _lib.EXACT_FIT_S_TAU,
            _lib.EXACT_FIT_S_SIG, _lib.EXACT_FIT_S_NTAB) == (R.S_OS_S, R.S_LS_S, R.S_OS_N, R.S_LS_N, R.S_TAU, R.S_SIG, R.S_NTAB)


_ratios = {}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%s-%d-%d-%d" % c)
def test_reference_sums_chained_to_the_raw_parameters_equal_autograd(case):
    """Pins the GPU test's reference: the longdouble sums on (alpha, K^-1) of the case, through the chain rule, against torch
    autograd of the plain statement to 1e-10 relative per tensor; the covariance and the table restatements on the way."""
    m = R.make_model(*case)
    c = R.case_of(m)
    with torch.no_grad():
        K_t = m.covar_module(m.x_train, m.x_train) + m.likelihood.noise * torch.eye(c["n"], dtype=torch.float64)
    K = np.asarray(R.covariance(c), np.float64)
    assert np.abs(K - K_t.numpy()).max() <= 1e-13 * np.abs(K).max()
    alpha, Kinv = R.given_from_float64(c)
    S, Rk = R.sums_ref(c, alpha, Kinv)
    assert np.all(Rk >= np.abs(S))
    g = R.chain(c, S)
    v = m.marginal_log_likelihood(hip=False)
    assert abs(float(v) - R.mll_ref(c)) <= 1e-10 * max(1.0, abs(float(v)))
    (-v).backward()
    names, params = R.param_names(m), dict(m.named_parameters())
    assert set(names.values()) == set(params) and ("rho" in names) == (case[0] == "MFGP_lin")
    for slot, name in names.items():
        b = params[name].grad.reshape(-1).numpy()
        a = np.asarray(g[slot], np.float64)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (slot, np.abs(a - b).max(), np.abs(b).max())
    _ratios[case] = R.term_ratio(c, np.asarray(alpha, np.float64), np.asarray(Kinv, np.float64))
    print("single-term ratio of the float64 restatement %s: %.2f" % (case, _ratios[case]))
    assert _ratios[case] <= R.EXACT_FIT_TERM_RATIO_MEASURED
    if len(_ratios) == len(R.CASES):      # the recorded figure is the measured one, rounded up
        assert max(_ratios.values()) > 0.9 * R.EXACT_FIT_TERM_RATIO_MEASURED
    assert R.EXACT_FIT_CT == 4.0 * R.EXACT_FIT_TERM_RATIO_MEASURED


def test_reference_update_rule_is_fit_s_loop():
    """UpdateModel on the losses and gradients autograd gives walks fit()'s trajectory, best iterate and restore included."""
    for lr, restored in ((0.05, False), (0.5, True)):
        m = mes_models(24, 2, 2, seed=1)["o1"]
        names = [k for k, _ in m.named_parameters()]
        flat = lambda: np.concatenate([p.detach().reshape(-1).numpy() for p in m.parameters()])
        um = R.UpdateModel(flat(), lr)
        probe = mes_models(24, 2, 2, seed=1)["o1"]
        for it in range(15):
            with torch.no_grad():
                for p, q in zip(probe.parameters(), np.split(np.asarray(um.raw, np.float64), np.cumsum([p.numel() for p in probe.parameters()])[:-1])):
                    p.copy_(torch.as_tensor(q).reshape(p.shape))
            for p in probe.parameters():
                p.grad = None
            loss = -probe.marginal_log_likelihood(hip=False)
            loss.backward()
            um.step(float(loss), 0, np.concatenate([p.grad.reshape(-1).numpy() for p in probe.parameters()]))
        with torch.no_grad():
            for p, q in zip(probe.parameters(), np.split(np.asarray(um.raw, np.float64), np.cumsum([p.numel() for p in probe.parameters()])[:-1])):
                p.copy_(torch.as_tensor(q).reshape(p.shape))
            um.finish(float(-probe.marginal_log_likelihood(hip=False)), 0)
        seen = R.host_loop(m, 15, lr)
        assert um.restored == seen["restored"] == restored and um.best_it == seen["best_iteration"], names
        assert np.abs(np.asarray(um.raw, np.float64) - flat()).max() < 1e-9
        assert np.abs(np.array(um.losses) - np.array(seen["losses"])).max() < 1e-9 * max(1.0, np.abs(seen["losses"]).max())
    um = R.UpdateModel(np.ones(3), 0.1)
    for loss in (3.0, 2.0, 2.5, float("nan"), 1.0):
        um.step(loss, 0, np.ones(3))
    assert um.stopped_at == 3 and um.best_it == 1 and um.it == 3 and um.losses == [3.0, 2.0, 2.5]
