"""CPU-only checks of the device acquisition search: the float64 restatements of its three kernels (tests/acq_search_reference.py)
against torch.autograd, torch.optim.Adam and torch.topk; the entry points' argument validation (host code, no device); and the
fall-back of ``JESMOC_MFDGP(search="device")`` to the host loop where no one-launch group applies."""
import contextlib
import ctypes
import pickle

import pytest
import torch

from tests import acq_search_reference as R


def _moments(n_pairs, T, S, seed):
    g = torch.Generator().manual_seed(seed)
    n = 2 * n_pairs
    mom = torch.empty(n, 2, T * S, dtype=torch.float64)
    mom[:, 0] = torch.randn(n, T * S, dtype=torch.float64, generator=g)
    mom[:, 1] = 0.05 + 1.95 * torch.rand(n, T * S, dtype=torch.float64, generator=g)
    mom[1::2, 1] *= torch.where(torch.rand(n_pairs, 1, dtype=torch.float64, generator=g) < 0.5, 0.3, 3.0)
    noise = 1e-3 + 0.099 * torch.rand(n, dtype=torch.float64, generator=g)
    return mom, noise


@pytest.mark.parametrize("S", [1, 4])
def test_reference_seeds_equal_autograd_of_the_acquisition_moments(S):
    n_pairs, T = 4, 9
    mom, noise = _moments(n_pairs, T, S, seed=S)
    n = 2 * n_pairs
    leaf = mom.clone().requires_grad_(True)
    # TinyPredictGroup.acquisition_moments, then JESMOC_MFDGP.coupled_acq
    mean, var = leaf[:, 0], leaf[:, 1] + noise[:, None]
    if S == 1:
        v = var
    else:
        mu = mean.reshape(n, T, S)
        mus = mu.mean(2)
        v = (var.reshape(n, T, S) + mu * mu).mean(2) - mus * mus
    acq = (0.5 * torch.clamp(torch.log(v[0::2]) - torch.log(v[1::2]), min=0.0)).sum(0)
    (want,) = torch.autograd.grad(acq.sum(), leaf)
    got_acq, seeds, _ = R.jes_group_forward(mom, noise, T, S)
    assert float((got_acq - acq.detach()).abs().max()) <= 1e-14 * (1.0 + float(acq.detach().abs().max()))
    assert float((seeds - want).abs().max()) <= 1e-14 * float(want.abs().max())
    clamped = (seeds[0::2, 1] == 0.0).all(1)
    assert bool(clamped.any()) and not bool(clamped.all())      # both kinds of pairs occur
    if S == 1:
        assert not bool(seeds[:, 0].any())


def test_reference_adam_and_clamp_equal_torch_optim_adam():
    g = torch.Generator().manual_seed(3)
    T, d, n_models = 7, 3, 4
    lo, hi = torch.tensor([0.0, -1.0, 0.2], dtype=torch.float64), torch.tensor([1.0, 1.0, 0.8], dtype=torch.float64)
    x0 = lo + (hi - lo) * torch.rand(T, d, dtype=torch.float64, generator=g)
    p = x0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=0.05)
    x, m, v = x0.clone(), torch.zeros(T, d, dtype=torch.float64), torch.zeros(T, d, dtype=torch.float64)
    clipped = False
    for step in range(1, 21):
        gx = torch.randn(n_models, T, d, dtype=torch.float64, generator=g)
        s = gx[0].clone()
        for k in range(1, n_models):
            s = s + gx[k]
        p.grad = -s
        opt.step()
        with torch.no_grad():
            clipped |= bool(((p < lo) | (p > hi)).any())
            p.clamp_(min=lo, max=hi)
        x, m, v = R.ascent_adam_step(x, gx, lo, hi, m, v, step, 0.05)
        assert float((x - p.detach()).abs().max()) <= 1e-15 * float(p.detach().abs().max()), step
    assert clipped


def test_reference_topk_order_ties_and_nans():
    g = torch.Generator().manual_seed(5)
    vals = torch.randperm(50, generator=g).double() * 0.37 - 4.0      # distinct
    x = torch.randn(50, 3, dtype=torch.float64, generator=g)
    want = torch.topk(vals, 7)
    v, i, rows = R.select_topk(vals, 7, x)
    assert torch.equal(v, want.values) and torch.equal(i, want.indices) and torch.equal(rows, x[want.indices])
    nan, inf = float("nan"), float("inf")
    vals = torch.tensor([1.0, nan, 3.0, 3.0, -inf, 1.0, nan, 3.0], dtype=torch.float64)
    v, i, _ = R.select_topk(vals, 8)
    assert i.tolist() == [2, 3, 7, 0, 5, 4, 1, 6]
    assert v[:6].tolist() == [3.0, 3.0, 3.0, 1.0, 1.0, -inf] and bool(torch.isnan(v[6:]).all())
    best_v, best_x = R.track_best(torch.tensor([nan, 2.0, 1.0]), torch.ones(3, 2), torch.tensor([0.0, -inf, 1.0]), torch.zeros(3, 2))
    assert best_v.tolist() == [0.0, 2.0, 1.0] and best_x[:, 0].tolist() == [0.0, 1.0, 0.0]


def test_entry_points_refuse_bad_arguments_without_a_device():
    from mobocmf_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)      # never dereferenced: every call below is refused before any device call

    def jes(moments=p, noise=p, n_pairs=2, T=3, S=2, acq=p, want_seeds=1, seeds=p, track=1, x=p, d=2, best_v=p, best_x=p):
        return lib.mobocmf_jes_group_forward(moments, noise, n_pairs, T, S, acq, want_seeds, seeds, track, x, d, best_v, best_x, None)

    for kw in (dict(n_pairs=0), dict(n_pairs=33), dict(T=0), dict(S=0), dict(moments=None), dict(noise=None), dict(acq=None),
               dict(seeds=None), dict(x=None), dict(best_v=None), dict(best_x=None), dict(d=0), dict(d=33), dict(want_seeds=2),
               dict(track=-1), dict(T=1 << 20, S=1 << 10)):
        assert jes(**kw) == _lib.BAD_ARG, kw

    def adam(x=p, gx=p, n_models=2, T=3, d=2, lo=p, hi=p, m=p, v=p, steps=p):
        return lib.mobocmf_ascent_adam_step(x, gx, n_models, T, d, lo, hi, m, v, 0.01, 0.9, 0.999, 1e-8, steps, None)

    for kw in (dict(x=None), dict(gx=None), dict(lo=None), dict(hi=None), dict(m=None), dict(v=None), dict(steps=None),
               dict(n_models=0), dict(n_models=65), dict(T=0), dict(T=4097), dict(d=0), dict(d=33)):
        assert adam(**kw) == _lib.BAD_ARG, kw

    def topk(vals=p, n=10, k=3, x=p, d=2, out_vals=p, out_idx=p, out_x=p):
        return lib.mobocmf_select_topk(vals, n, k, x, d, out_vals, out_idx, out_x, None)

    for kw in (dict(k=0), dict(k=65, n=100), dict(k=4, n=3), dict(n=4097), dict(vals=None), dict(out_vals=None), dict(out_idx=None),
               dict(x=None), dict(out_x=None), dict(d=0), dict(d=33)):
        assert topk(**kw) == _lib.BAD_ARG, kw
    assert (_lib.ACQ_MAX_PAIRS, _lib.TOPK_MAX_K, _lib.TOPK_MAX_N) == (32, 64, 4096)


def test_device_search_on_cpu_models_runs_the_host_loop():
    """CPU surrogates fit no one-launch group: ``search="device"`` runs the host loop, says so in ``last_search_engine``, and
    returns what ``search="host"`` returns from an equal generator state.  (The models' arithmetic has no CPU path, so the
    per-black-box value is a stand-in; the engine choice looks only at where the models and the bounds live.)"""
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP, _JES_MFDGP
    from tests.test_host_cpu import _forrester_model

    class Stub(_JES_MFDGP):
        def forward(self, X):
            X = X[:, 0, :] if X.dim() > 2 else X
            return 1.0 + self.fidelity - ((X - 0.3) ** 2).sum(-1)
        __call__ = forward

        @contextlib.contextmanager
        def frozen(self):
            yield self

    model = _forrester_model()[0]
    with pytest.raises(ValueError):
        JESMOC_MFDGP(None, search="graph")
    acq = JESMOC_MFDGP.__new__(JESMOC_MFDGP)
    assert acq.search == "host"      # the default, also for objects made without the constructor
    acq.num_fidelities, acq.eval_highest_fidelity = 2, False
    acq.standard_bounds = torch.tensor([[0.0], [1.0]], dtype=torch.float64)
    acq.objectives = {f: {"bb0": Stub(f, model, model)} for f in (0, 1)}
    acq.constraints = {0: {}, 1: {}}
    acq.costs_blackboxes = {0: {"total": 1.0}, 1: {"total": 10.0}}
    out = {}
    for engine in ("host", "device"):
        acq.search = engine
        cand, fidelity = acq.get_nextpoint_coupled(maxiter=15, generator=torch.Generator().manual_seed(7))
        assert acq.last_search_engine == {0: "host", 1: "host"}
        out[engine] = (cand, fidelity)
    assert out["host"][1] == out["device"][1] == 0      # 1 / 1 > 2 / 10
    assert torch.equal(out["host"][0], out["device"][0])
    assert abs(float(out["device"][0][0]) - 0.3) < 0.05
    acq.search = "nope"
    with pytest.raises(ValueError):
        acq.get_nextpoint_coupled(maxiter=1)
    state = pickle.loads(pickle.dumps({k: v for k, v in acq.__getstate__().items() if k not in ("objectives",)}))
    assert "_device_searches" not in state and "_tiny_groups" not in state
