"""CPU-only checks of the frozen-chain predict path (csrc/frozen_predict.hip, util/panel_predict.py): its float64 restatement
(tests/panel_predict_reference.py) against the oracle's dense evaluation, the gate, the descriptor builder and the host-side
argument checks of the entry points."""
import ctypes

import pytest
import torch

from mobocmf_amd import _lib
from mobocmf_amd import functional as F
from mobocmf_amd.util import panel_predict as PP
from mobocmf_amd.util import synthetic
from oracle import mfdgp_oracle as O
from tests import panel_predict_reference as R
from tests.helpers import oracle_state

# The restatement and the oracle run the same whitened algebra on the same float64 inputs; they differ in how L^-1 is applied
# (an explicit inverse here, as the kernel has it; triangular solves there).  tests/test_warm_start_cpu.py bounds the same oracle
# on problems of this size (M <= 20, d = 2 .. 3) at 1e-8, about 100x what it observed; the same bound is used here.
TOL = 1e-8


def _packed(h):
    if "alpha" in h:
        return torch.cat([h["alpha"].reshape(1), h["ls"].reshape(-1)])
    return torch.cat([h[k].reshape(-1) for k in ("a1", "af", "nu", "a2", "lsf", "ls1", "ls2")])


def _rel(a, b):
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("L,d", [(2, 2), (3, 3)])
def test_reference_matches_the_oracle(L, d):
    M, S, T = 20, 3, 7
    st = oracle_state(synthetic.make_problem(d=d, L=L, M=M, N=26, S=S, seed=4 + L))
    chains = [R.chain_state(_packed(lay["hyp"]), 1 if l else 0, O.inducing_inputs(st, l), lay["m"], lay["L_S"], O.JITTER)
              for l, lay in enumerate(st["layers"])]
    g = torch.Generator().manual_seed(L)
    X = torch.rand(T, d, dtype=torch.float64, generator=g)
    worst = {}
    for fidelity in range(L):
        ncol = T * (S if fidelity else 1)
        wm, wv = torch.randn(ncol, dtype=torch.float64, generator=g), torch.randn(ncol, dtype=torch.float64, generator=g)
        mean, var, _ = R.predict(chains[:fidelity + 1], st["samples"], X, S)
        Xo = X.clone().requires_grad_(True)
        Xt = Xo.repeat_interleave(S, 0) if fidelity else Xo
        mo, vo = O.model_forward(st, Xt, training=False, eval_mode=True, max_fidelity=fidelity)[fidelity]
        ((mo * wm).sum() + (vo * wv).sum()).backward()
        gx = R.input_gradient(chains[:fidelity + 1], st["samples"], X, S, wm, wv)
        gk = R.input_gradient_by_the_kernels_formulas(chains[:fidelity + 1], st["samples"], X, S, wm, wv)
        worst[fidelity] = (_rel(mean, mo), _rel(var, vo), _rel(gx, Xo.grad), _rel(gk, gx))
        assert max(worst[fidelity][:3]) <= TOL, worst
        assert worst[fidelity][3] <= 1e-12, worst      # the kernel's backward formulas ARE the autograd gradient
    print("panel predict reference vs oracle, L = %d: (mean, var, gradient, formulas) per fidelity" % L, worst)


def test_variance_floor_passes_no_variance_gradient_in_the_reference():
    """A test point ON an inducing input of a model with a tiny L_S (1e-7 I) and a tiny jitter (1e-12; d = 8 keeps K_mm well
    conditioned): k_nn - |A|^2 + |C|^2 ~ 1e-12 lands under 1e-10, the variance is the floor and only the mean's gradient remains."""
    prob = synthetic.make_problem(d=8, L=1, M=12, N=12, S=1, seed=1)
    st = oracle_state(prob)
    lay = st["layers"][0]
    ch = R.chain_state(_packed(lay["hyp"]), 0, st["Zx"], lay["m"], 1e-7 * torch.eye(12, dtype=torch.float64), 1e-12)
    X = torch.stack([st["Zx"][3], torch.full((8,), 0.5, dtype=torch.float64)])
    mean, var, per = R.predict([ch], [None], X, 1)
    assert float(per[0][3]["raw"][0]) < 1e-10 < float(per[0][3]["raw"][1]) and float(var[0]) == 1e-10
    ones, zeros = torch.ones(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    g = R.input_gradient_by_the_kernels_formulas([ch], [None], X, 1, zeros, ones)
    assert not bool(g[0].any()) and bool(g[1].any())


# ------------------------------------------------------------------ the gate and the descriptor builder
def _cpu_model(M, d, S, L=2):
    from mobocmf_amd import gp
    from mobocmf_amd.models import MFDGP
    from tests.helpers import to_t
    prob = synthetic.make_problem(d=d, L=L, M=M, N=M, S=S, seed=0)
    model = MFDGP(to_t(prob["x"]), to_t(prob["y"])[:, None], to_t(prob["fid"])[:, None], num_fidelities=L,
                  inducing_points=to_t(prob["Zx"]), num_samples_for_acquisition=S, num_samples_for_training=1)
    model.double()
    for l in range(L):
        lik = getattr(model, f"hidden_layer_likelihood_{l}")
        lik.raw_noise_constraint = gp.Interval(1e-8, 1.0)
        lik.noise = torch.tensor(1e-3, dtype=torch.float64)
    return model


def test_fits_predict_limits_and_reasons():
    ok = _cpu_model(129, 2, 3)
    assert PP.fits_predict(ok, 1, 5, 2, on_gpu=False) and PP.fits_predict(ok, 0, 200, 2, on_gpu=False)
    assert PP.why_not(ok, 1, 5, 2, on_gpu=False) is None
    assert not PP.fits_predict(ok, 1, 5, 2)      # (parameters on the host)
    assert "on the GPU" in PP.why_not(ok, 1, 5, 2)
    assert "layer 2" in PP.why_not(ok, 2, 5, 2, on_gpu=False)
    assert "T S" in PP.why_not(ok, 1, _lib.ACQ_MAX_COLUMNS // 3 + 1, 2, on_gpu=False)
    for model, d, word in ((_cpu_model(128, 2, 3), 2, "M = 128"), (_cpu_model(513, 2, 3), 2, "M = 513"),
                           (_cpu_model(130, 2, 1), 2, "S = 1"), (_cpu_model(130, 9, 3), 9, "d = 9")):
        assert not PP.fits_predict(model, 1, 5, d, on_gpu=False)
        assert word in PP.why_not(model, 1, 5, d, on_gpu=False)
    assert PP.fits_predict(_cpu_model(130, 2, 1), 0, 5, 2, on_gpu=False)      # no replicas below layer 1: S does not matter
    assert PP.MIN_M == _lib.COOP_MAX_M + 1 and PP.MAX_M == _lib.FROZEN_MAX_M == 512


def test_every_group_class_gates_with_its_own_why_not():
    """The classmethod every predict group has (util/predict_group.py) is the module-level gate of its kernel: None or a
    sentence, the one-workgroup class with its speed rule only where asked."""
    from mobocmf_amd.util import coop_step as CS
    from mobocmf_amd.util import tiny_step as TS
    from mobocmf_amd.util.predict_group import PredictGroup
    classes = (TS.TinyPredictGroup, CS.CoopPredictGroup, PP.PanelPredictGroup, PP.SplitPredictGroup)
    assert all(issubclass(c, PredictGroup) for c in classes) and not issubclass(PP.PanelPredictGroup, TS.TinyPredictGroup)
    takes = {16: (True, True, False, False), 32: (True, True, False, False), 33: (False, True, False, False),
             128: (False, True, False, False), 129: (False, False, True, True), 513: (False, False, False, True)}
    for M, want in takes.items():
        model = _cpu_model(M, 2, 3)
        got = [c.why_not(model, 1, 5, 2, on_gpu=False) for c in classes]
        assert tuple(g is None for g in got) == want and all(g is None or isinstance(g, str) for g in got), (M, got)
        host = [c.why_not(model, 1, 5, 2) for c in classes]      # (parameters on the host: no class takes it)
        assert all(isinstance(h, str) for h in host) and all("on the GPU" in h for h, g in zip(host, got) if g is None)
    assert PP.PanelPredictGroup.why_not(_cpu_model(513, 2, 3), 1, 5, 2, on_gpu=False) == PP.why_not(_cpu_model(513, 2, 3), 1, 5, 2, on_gpu=False)
    wide = _cpu_model(32, 2, 25)      # 100 x 25 columns: within the kernel's limit, beyond what one workgroup is quick at
    assert TS.TinyPredictGroup.why_not(wide, 1, 100, 2, on_gpu=False) is None
    assert "speed rule" in TS.TinyPredictGroup.why_not(wide, 1, 100, 2, on_gpu=False, speed_rule=True)


def _fake_chain(kind, M, d):
    """A FrozenChain of host tensors with the library's own state size (nothing is computed)."""
    lib = _lib.load()
    desc = F.make_desc(kind, d, M, 1, 1, 1, False, F.JITTER, F.MIN_VARIANCE)
    bb, nb = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(lib.mobocmf_chain_block_bytes(ctypes.byref(desc), ctypes.byref(bb), ctypes.byref(nb)), "chain_block_bytes")
    Mp = (M + 127) // 128 * 128
    assert nb.value == (6 * Mp * Mp + 2 * Mp) * 8      # L, L^-1, L^-T, U, U^T, L_S, then a and m: the order the kernel indexes
    fc = F.FrozenChain()
    fc.kind, fc.d, fc.M = kind, d, M
    fc.state = torch.zeros(nb.value, dtype=torch.uint8)
    fc.Zx, fc.zf = torch.zeros(M, d, dtype=torch.float64), (torch.zeros(M, dtype=torch.float64) if kind else None)
    fc.hyp = torch.ones(5 + 2 * d if kind else 1 + d, dtype=torch.float64)
    fc.info = torch.zeros((), dtype=torch.int32)
    return fc


def test_descriptor_builder_and_host_side_argument_checks():
    lib = _lib.load()
    M, d, S, T = 200, 3, 4, 6
    chains = [_fake_chain(0, M, d), _fake_chain(1, M, d), _fake_chain(1, M, d)]
    samples = [None, torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)]
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    x, mom, seeds, gx = z(T, d), z(2, T * S), z(2, T * S), z(T, d)
    host = (_lib.FrozenPredictModel * 1)()
    rec = host[0]
    keep = PP.describe(rec, chains, samples, S, T, d, x, mom[0], mom[1], seeds[0], seeds[1], gx)
    assert (rec.L, rec.M, rec.d, rec.S, rec.T) == (3, M, d, S, T) and list(rec.kind) == [0, 1, 1]
    assert [rec.chain[l] for l in range(3)] == [c.state.data_ptr() for c in chains] and len(set(rec.chain[:])) == 3
    assert rec.zf[0] is None and rec.samples[0] is None and rec.zf[2] == chains[2].zf.data_ptr()
    assert rec.top_var == mom[1].data_ptr() and rec.grad == gx.data_ptr() and rec.work is None and len(keep) == 3 * 3 + 2 * 2
    two = (_lib.FrozenPredictModel * 1)()
    PP.describe(two[0], chains[:1], samples[:1], S, T, d, x, mom[0], mom[1])
    assert two[0].L == 1 and two[0].S == 1 and two[0].chain[1] is None and two[0].seed_gmean is None
    with pytest.raises(_lib.MobocmfError):
        PP.describe(two[0], [chains[1]], samples[:1], S, T, d, x, mom[0], mom[1])      # layer 0 must be of kind 0
    wb = ctypes.c_size_t(7)
    assert lib.mobocmf_frozen_predict_work_bytes(ctypes.byref(rec), _lib.STEP_INPUT_GRADIENTS, ctypes.byref(wb)) == _lib.OK
    assert wb.value == 0
    assert lib.mobocmf_frozen_predict_work_bytes(ctypes.byref(rec), _lib.STEP_UPDATE, ctypes.byref(wb)) == _lib.BAD_ARG

    # every refusal is made on the host, before any HIP call: there is no device here, and none is needed
    def launch(mutate, mode=_lib.STEP_INPUT_GRADIENTS, n=1):
        B = (_lib.FrozenPredictModel * 1)()
        ctypes.memmove(B, host, ctypes.sizeof(host))
        mutate(B[0])
        p = ctypes.cast(B, ctypes.c_void_p)
        return lib.mobocmf_frozen_predict(p, p, n, mode, None)

    def setter(name, value, index=None):
        def f(b):
            if index is None:
                setattr(b, name, value)
            else:
                getattr(b, name)[index] = value
        return f

    bad = [setter("M", 513), setter("M", 0), setter("d", 9), setter("S", 1), setter("S", _lib.MAX_XDIV + 1), setter("L", 4),
           setter("T", 0), setter("T", _lib.ACQ_MAX_COLUMNS // S + 1), setter("x", None), setter("top_mean", None),
           setter("grad", None), setter("seed_gvar", None), setter("kind", 1, 0), setter("kind", 0, 2), setter("chain", None, 1),
           setter("zf", None, 1), setter("samples", None, 2), setter("hyp", None, 0), setter("Zx", None, 2)]
    for m in bad:
        assert launch(m) == _lib.BAD_ARG
    for mode in (_lib.STEP_GRADIENTS, _lib.STEP_UPDATE, _lib.STEP_COUPLED, _lib.STEP_FORWARD | _lib.STEP_CHAIN_VALID, 7):
        assert launch(lambda b: None, mode=mode) == _lib.BAD_ARG
    assert launch(lambda b: None, n=0) == _lib.BAD_ARG and launch(lambda b: None, n=257) == _lib.BAD_ARG
