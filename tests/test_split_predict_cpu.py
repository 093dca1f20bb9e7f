"""CPU-only checks of the split frozen-chain predict path (mobocmf_frozen_predict_split, util/panel_predict.py SplitPredictGroup):
the gate and the constants, the bytes of `work`, the host-side argument checks of the entry point, and the identity its input
gradient rests on -- the backward below the top layer is linear in what the layer above sends back, so the gradients of the
parts of a test point's replicas add up to the gradient of all of them."""
import ctypes

import pytest
import torch

from mobocmf_amd import _lib
from mobocmf_amd.util import panel_predict as PP
from mobocmf_amd.util import synthetic
from oracle import mfdgp_oracle as O
from tests import panel_predict_reference as R
from tests.helpers import oracle_state
from tests.test_panel_predict_cpu import _cpu_model, _fake_chain, _packed

PART = 8      # replicas of a part, columns of a panel
IDENTITY_JITTER = 2e-2      # test_the_parts_gradients_add_up_to_the_whole: rounding two orders under its bound


def test_constants_and_gate():
    assert _lib.FROZEN_SPLIT_MAX_M == 1024 and PP.SPLIT_MAX_M == 1024 and PP.MAX_M == 512
    for M in (129, 513, 1024):
        model = _cpu_model(M, 2, 3)
        assert PP.fits_predict_split(model, 1, 5, 2, on_gpu=False) and PP.why_not_split(model, 1, 5, 2, on_gpu=False) is None
        assert PP.fits_predict_split(model, 0, 200, 2, on_gpu=False)
        assert PP.fits_predict(model, 1, 5, 2, on_gpu=False) == (M <= 512)      # the 16-column gate is where it was
    ok = _cpu_model(513, 2, 3)
    assert "layer 2" in PP.why_not_split(ok, 2, 5, 2, on_gpu=False)
    assert "on the GPU" in PP.why_not_split(ok, 1, 5, 2)
    for model, d, word in ((_cpu_model(128, 2, 3), 2, "M = 128"), (_cpu_model(1025, 2, 3), 2, "M = 1025"),
                           (_cpu_model(513, 2, 1), 2, "S = 1"), (_cpu_model(513, 9, 3), 9, "d = 9")):
        assert not PP.fits_predict_split(model, 1, 5, d, on_gpu=False)
        assert word in PP.why_not_split(model, 1, 5, d, on_gpu=False)
    assert PP.fits_predict_split(_cpu_model(513, 2, 1), 0, 5, 2, on_gpu=False)      # no replicas below layer 1


def _sizes(L, M, d, S, T):
    rec = _lib.FrozenPredictModel()
    rec.L, rec.M, rec.d, rec.S, rec.T = L, M, d, S, T
    return rec


def test_work_bytes():
    lib = _lib.load()

    def wb(rec, mode):
        n = ctypes.c_size_t(7)
        rc = lib.mobocmf_frozen_predict_split_work_bytes(ctypes.byref(rec), mode, ctypes.byref(n))
        return rc, n.value

    assert wb(_sizes(2, 513, 2, 25, 5), _lib.STEP_INPUT_GRADIENTS) == (_lib.OK, 4 * 5 * 2 * 8)
    assert wb(_sizes(2, 513, 2, 25, 5), _lib.STEP_FORWARD) == (_lib.OK, 0)
    assert wb(_sizes(1, 513, 2, 1, 5), _lib.STEP_INPUT_GRADIENTS) == (_lib.OK, 0)
    assert wb(_sizes(2, 1024, 8, 48, 1), _lib.STEP_INPUT_GRADIENTS) == (_lib.OK, 6 * 8 * 8)
    assert wb(_sizes(3, 640, 3, 9, 3), _lib.STEP_INPUT_GRADIENTS) == (_lib.OK, 2 * 3 * 3 * 8)
    for mode in (_lib.STEP_GRADIENTS, _lib.STEP_UPDATE, _lib.STEP_COUPLED, 7):
        assert wb(_sizes(2, 513, 2, 25, 5), mode)[0] == _lib.BAD_ARG
    assert wb(_sizes(2, 1025, 2, 25, 5), _lib.STEP_INPUT_GRADIENTS)[0] == _lib.BAD_ARG
    assert lib.mobocmf_frozen_predict_split_work_bytes(ctypes.byref(_sizes(2, 513, 2, 25, 5)), _lib.STEP_FORWARD, None) == _lib.BAD_ARG


def test_host_side_argument_checks_of_the_split_launch():
    """Every refusal is made on the host, before any HIP call: there is no device here, and none is needed."""
    lib = _lib.load()
    M, d, S, T = 200, 3, 4, 6
    chains = [_fake_chain(0, M, d), _fake_chain(1, M, d), _fake_chain(1, M, d)]
    samples = [None, torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)]
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    x, mom, seeds, gx, work = z(T, d), z(2, T * S), z(2, T * S), z(T, d), z(T * d)
    host = (_lib.FrozenPredictModel * 1)()
    PP.describe(host[0], chains, samples, S, T, d, x, mom[0], mom[1], seeds[0], seeds[1], gx, work)
    assert host[0].work == work.data_ptr()
    two = (_lib.FrozenPredictModel * 1)()
    PP.describe(two[0], chains[:2], samples[:2], S, T, d, x, mom[0], mom[1], seeds[0], seeds[1], gx, work)

    def launch(mutate, mode=_lib.STEP_INPUT_GRADIENTS, n=1, base=host):
        B = (_lib.FrozenPredictModel * 1)()
        ctypes.memmove(B, base, ctypes.sizeof(base))
        mutate(B[0])
        p = ctypes.cast(B, ctypes.c_void_p)
        return lib.mobocmf_frozen_predict_split(p, p, n, mode, None)

    def setter(name, value, index=None):
        def f(b):
            if index is None:
                setattr(b, name, value)
            else:
                getattr(b, name)[index] = value
        return f

    bad = [setter("M", 1025), setter("M", 0), setter("d", 9), setter("S", 1), setter("S", _lib.MAX_XDIV + 1), setter("L", 4),
           setter("T", 0), setter("T", _lib.ACQ_MAX_COLUMNS // S + 1), setter("x", None), setter("top_mean", None),
           setter("top_var", None), setter("grad", None), setter("seed_gmean", None), setter("seed_gvar", None),
           setter("work", None), setter("kind", 1, 0), setter("kind", 0, 2), setter("chain", None, 1), setter("zf", None, 1),
           setter("samples", None, 2), setter("hyp", None, 0), setter("Zx", None, 2)]
    for m in bad:
        assert launch(m) == _lib.BAD_ARG
    assert launch(setter("S", 1), base=two) == _lib.BAD_ARG and launch(setter("work", None), base=two) == _lib.BAD_ARG
    for m in (setter("x", None), setter("top_var", None), setter("M", 1025), setter("chain", None, 2)):
        assert launch(m, mode=_lib.STEP_FORWARD) == _lib.BAD_ARG
    for mode in (_lib.STEP_GRADIENTS, _lib.STEP_UPDATE, _lib.STEP_COUPLED, _lib.STEP_FORWARD | _lib.STEP_CHAIN_VALID, 7):
        assert launch(lambda b: None, mode=mode) == _lib.BAD_ARG
    assert launch(lambda b: None, n=0) == _lib.BAD_ARG and launch(lambda b: None, n=257) == _lib.BAD_ARG
    # the 16-column entry point keeps its limit
    p = ctypes.cast(host, ctypes.c_void_p)
    host[0].M = 513
    assert lib.mobocmf_frozen_predict(p, p, 1, _lib.STEP_INPUT_GRADIENTS, None) == _lib.BAD_ARG


@pytest.mark.parametrize("L", [2, 3])
def test_the_parts_gradients_add_up_to_the_whole(L, monkeypatch):
    """The kernel's backward (tests/panel_predict_reference.py) with the seeds masked to the replicas of part p, summed over the
    parts, is the unmasked gradient: S = 11 is two parts (8 + 3).  Then the same with one column of part 1 forced to the variance
    floor, which then passes no variance gradient: the gate depends on the forward alone, so the identity
    holds there too, and the floored gradient differs from the unfloored one.

    Bound: relative 1e-12 (largest difference over the largest entry).  The identity is exact algebra for ANY chain state
    (L^-1, U, a); what a float64 evaluation adds is rounding through L^-1 and L^-T, eps cond(L) = eps sqrt(cond(K_mm + jitter I)).
    40 inducing points in [0, 1]^2 under the library's jitter 1e-6 have cond ~ 1e8, and the restatement then differs from itself
    (autograd against the kernel's formulas, and the parts against the whole alike) by 2e-12 .. 5e-11 over eight problem seeds
    and two hosts: no float64 evaluation separates the identity from rounding at 1e-12 there.  The chains of this test are
    therefore formed with the jitter for which 100 eps cond(L) <= 1e-12: cond(L) <= 45, cond(K_mm + jitter I) <= 2e3, and with
    lambda_max(K_mm) <= trace ~ 40 that is jitter = 2e-2 (measured: <= 2e-14 over six problem seeds, and eps sqrt(cond) holds in
    between: ~5e-13 at jitter 1e-4, ~1e-13 at 1e-3).  Sizes, reference and bound are unchanged by that."""
    M, d, S, T = 40, 2, 11, 3
    st = oracle_state(synthetic.make_problem(d=d, L=L, M=M, N=M, S=S, seed=20 + L))
    chains = [R.chain_state(_packed(lay["hyp"]), 1 if l else 0, O.inducing_inputs(st, l), lay["m"], lay["L_S"], IDENTITY_JITTER)
              for l, lay in enumerate(st["layers"])]
    assert all(float(torch.linalg.cond(torch.linalg.inv(ch["Linv"]))) <= 45.0 for ch in chains)      # (the premise of the bound)
    g = torch.Generator().manual_seed(L)
    X = torch.rand(T, d, dtype=torch.float64, generator=g)
    wm, wv = torch.randn(T * S, dtype=torch.float64, generator=g), torch.randn(T * S, dtype=torch.float64, generator=g)
    replica = torch.arange(T * S) % S
    masks = [(replica // PART == p).double() for p in range((S + PART - 1) // PART)]
    assert len(masks) == 2 and float(sum(masks).min()) == 1.0 == float(sum(masks).max())

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max())

    def measure():
        whole = R.input_gradient_by_the_kernels_formulas(chains, st["samples"], X, S, wm, wv)
        parts = [R.input_gradient_by_the_kernels_formulas(chains, st["samples"], X, S, wm * mk, wv * mk) for mk in masks]
        assert all(bool(p.abs().max() > 0) for p in parts)
        return whole, rel(parts[0] + parts[1], whole)

    free, err_free = measure()
    # replica 9 of test point 1 -- a column of part 1 -- at the floor, in the top layer (L = 2) or the one below it (L = 3)
    col, target, columns = 1 * S + 9, chains[1], R.layer_columns

    def forced(ch, rows):
        mean, var, saved = columns(ch, rows)
        if ch is target:
            raw = saved["raw"].clone()
            raw[col] = 0.5 * R.MIN_VARIANCE
            var, saved = raw.clamp_min(R.MIN_VARIANCE), dict(saved, raw=raw)
        return mean, var, saved

    monkeypatch.setattr(R, "layer_columns", forced)
    assert float(R.predict(chains, st["samples"], X, S)[2][1][2][col]) == R.MIN_VARIANCE
    floored, err_floored = measure()
    assert rel(floored[1], free[1]) > 1e-9      # the column's variance seed no longer arrives (rounding is ~1e-14)
    assert rel(floored[[0, 2]], free[[0, 2]]) <= 1e-12      # ... and the other test points do not notice
    print("parts add up, L = %d: relative difference %.3e, with a floored column %.3e" % (L, err_free, err_floored))
    assert err_free <= 1e-12 and err_floored <= 1e-12, (err_free, err_floored)
