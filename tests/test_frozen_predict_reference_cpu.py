"""CPU proof behind tests/test_hip_frozen_predict_conformance.py ("The given-chain bound"): on every case the
GPU file runs, with chains formed on the host -- the measured ratios behind FROZEN_RATIO_MEASURED, the conditions on the
inputs (the conditioning of the uniform-Z_x family, the floor columns where they are meant to be, every floor decision robust),
the planted defects the gate has to report, and the ties to the whole-model reference and to the torch restatement."""
import time

import numpy as np
import pytest
import torch

from tests import frozen_predict_reference as F
from tests import kernel_reference as R
from tests import panel_predict_reference as P

pytestmark = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason="numpy.longdouble is no wider than float64 here")

NAMES = F.FROZEN_NAMES["input"]
_chains = {}


def _host(name, mc):
    if name not in _chains:
        _chains[name] = F.host_chains(mc)
    return _chains[name]


def _cases(max_m=None):
    return {n: mc for n, mc in F.all_frozen_cases().items() if max_m is None or mc["M"] <= max_m}


def test_frozen_constants_are_the_measured_ones(capsys):
    """Per group the worst err / (u S) of the float64 run of frozen_predict_ref against the longdouble one over every case of
    the GPU file: recorded a quarter above it (between 1.1 and 1.5 x: the figure moves by a few per cent with the host's BLAS
    blocking), FROZEN_C = 4 x recorded.  Rows without seeds are exactly zero in both runs and have S = 0.  Prints per case the
    ratios, the medians of S / |value| -- what the gate can see -- and the time of the reference."""
    worst, lines = {g: (0.0, None) for g in F.FROZEN_GROUPS}, []
    for name, mc in _cases().items():
        ch = _host(name, mc)
        t0 = time.time()
        ref, S = F.frozen_predict_ref(mc, ch), F.frozen_predict_ref(mc, ch, shadow=True)
        dt = time.time() - t0
        got = F.frozen_predict_ref(mc, ch, dtype=np.float64)
        bad, w, _ = F.frozen_gate(got, ref, S, NAMES)
        assert all(nz == 0 for _, _, nz in bad), (name, bad)
        for g, v in w.items():
            if v > worst[g][0]:
                worst[g] = (v, name)
        off = np.arange(mc["rows"][0]) % 3 == 1
        assert np.all(np.asarray(ref["g_x"])[off] == 0) and np.all(np.asarray(S["g_x"])[off] == 0) and np.all(got["g_x"][off] == 0), name
        assert np.all(np.asarray(S["g_x"])[~off] > 0), name
        med = {}
        for k in NAMES:
            r, s = np.abs(np.asarray(ref[k], np.float64)).ravel(), np.asarray(S[k], np.float64).ravel()
            med[k] = float(np.median(s[r > 0] / r[r > 0]))
        lines.append("%-28s forward %.2f gram %.2f u S   S / |value| medians: mean %.1e var %.1e g_x %.1e   reference %.1f s"
                     % (name, w["forward"], w["gram"], med["top_mean"], med["top_var"], med["g_x"], dt))
        assert dt < 20.0, (name, dt)
    with capsys.disabled():
        print()
        print("\n".join(lines))
        for g, (v, name) in worst.items():
            print("frozen group %-8s measured %.2f u S (%s), recorded %.2f" % (g, v, name, F.FROZEN_RATIO_MEASURED[g]))
    for g, (v, _) in worst.items():
        assert 1.1 * v <= F.FROZEN_RATIO_MEASURED[g] <= 1.5 * v, (g, v)
        assert F.FROZEN_C[g] == 4 * F.FROZEN_RATIO_MEASURED[g]


def test_the_inputs_meet_their_conditions():
    """The uniform-Z_x family has the workload's conditioning -- cond(K_mm + jitter I) between 5e7 and 2e9 in every layer --
    and the lattice family stays below LAYER_COND_MAX up to M = 257; the floor family has exactly the last base row's column of
    its layer 0 on the floor and no other; no other case has a floored column.  (Every floor decision's robustness is asserted
    by frozen_predict_ref itself, on every longdouble run.)"""
    for name, mc in _cases(257).items():
        ch = _host(name, mc)
        for l, c in enumerate(ch):
            L = np.linalg.inv(c["Linv"])
            cond = np.linalg.cond(L @ L.T)
            if "uniform" in name:
                assert 5e7 <= cond <= 2e9, (name, l, cond)
            elif not name.startswith("M200"):                                  # (d = 4, uniform points at layer_case's lengthscales: 6e4)
                assert cond <= R.LAYER_COND_MAX, (name, l, cond)
        floored = [a.tolist() for a in F.floored_columns(mc, ch)]
        want = [[] for _ in range(mc["L"])]
        if name.startswith("floor"):
            want[0] = [mc["rows"][0] - 1]
        assert floored == want, (name, floored)


@pytest.mark.parametrize("defect", F.FROZEN_DEFECTS)
def test_the_gate_reports_every_planted_defect(defect):
    """Each defect, planted in the float64 run of the restatement, violates the gate on at least one case (M <= 257: the
    defects are not about size); the clean float64 run of the same cases passes it."""
    caught = []
    for name, mc in _cases(257).items():
        ch = _host(name, mc)
        ref, S = F.frozen_predict_ref(mc, ch), F.frozen_predict_ref(mc, ch, shadow=True)
        assert F.frozen_gate(F.frozen_predict_ref(mc, ch, dtype=np.float64), ref, S, NAMES)[0] == [], name
        dmc, dch = F.with_defect(mc, ch, defect)
        if dmc is mc and dch is ch:
            continue
        if F.frozen_gate(F.frozen_predict_ref(dmc, dch, dtype=np.float64), ref, S, NAMES)[0]:
            caught.append(name)
    assert caught, defect
    if defect == "floor_gate_ignored":
        assert all(n.startswith("floor") for n in caught), caught
    if defect == "eps_replica_shifted":
        assert caught == ["M130_L3_d2_S17_T3"], caught


def test_agrees_with_the_whole_model_reference_on_the_small_cases():
    """M <= 32: frozen_predict_ref on host-formed chains (factors and hyper-parameters rounded to float64) against model_ref,
    which forms its own factors in longdouble, inside MODEL_C under the whole model's shadow."""
    n = 0
    for name, mc in _cases(32).items():
        got = F.frozen_predict_ref(mc, _host(name, mc))
        bad, _, report = R.model_gate(got, R.model_ref(mc), R.model_ref(mc, shadow=True), NAMES, R.MODEL_C[mc["L"]])
        assert bad == [], (name, bad, report)
        n += 1
    assert n >= 4


def test_agrees_with_the_torch_restatement():
    """tests/panel_predict_reference.py (torch float64: its own kernel statements, autograd for the Gram backward) on the same
    host-formed chains, inside the new gate; M <= 257."""
    t = lambda a: torch.tensor(np.array(a), dtype=torch.float64)
    for name, mc in _cases(257).items():
        ch = _host(name, mc)
        layers = F.host_layers(mc)
        chains = []
        for l, (lc, c) in enumerate(zip(layers, ch)):
            Z = t(lc["Zx"]) if l == 0 else torch.cat([t(lc["Zx"]), t(lc["zf"])[:, None]], 1)
            chains.append(dict(kind=lc["kind"], hyp=t(c["hyp"]), Z=Z, Linv=t(c["Linv"]), U=t(c["U"]), a=t(c["a"])))
        S_ = mc["S"] if mc["L"] > 1 else 1
        samples = [None] + [t(s) for s in mc["samples"][1:]]
        X = t(mc["x"])
        with torch.no_grad():
            mean, var, _ = P.predict(chains, samples, X, S_)
        gx = P.input_gradient_by_the_kernels_formulas(chains, samples, X, S_, t(mc["seed_gmean"]), t(mc["seed_gvar"]))
        got = dict(top_mean=mean.numpy(), top_var=var.numpy(), g_x=gx.numpy())
        bad, _, report = F.frozen_gate(got, F.frozen_predict_ref(mc, ch), F.frozen_predict_ref(mc, ch, shadow=True), NAMES)
        assert bad == [], (name, bad, report)
