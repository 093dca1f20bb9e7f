"""The proof on the CPU that the gate of tests/rff_reference.py is neither fitted to the device nor blind: a float64
restatement in the kernels' summation orders against the longdouble one on every case the GPU file runs -- the measured
ratios behind RFF_RATIO_MEASURED --, the planted defects the gate has to report, the one-step model's conditions on every
refinement case, and the ties of the longdouble statement to the numpy oracle's feature maps and to central differences."""
import numpy as np
import pytest

from oracle import rff_oracle as RO
from tests import kernel_reference as R
from tests import rff_reference as F

pytestmark = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason="numpy.longdouble is no wider than float64 here")


def _refine_points(c):
    return F._clamp(c["x0"].reshape(-1, c["d"]))


def _runs():
    """(label, case, x, order, nw, names) of every float64 run that is measured: the eval cases in the order of
    rff_eval_chains_kernel, the value_grad cases in a wavefront's, every chain of the refine cases at the clamped starts in
    ro_chain<DB, NW>'s."""
    for name in F.EVAL_CASES:
        yield "eval " + name, F.eval_case(name), None, "eval", 1, ("value",)
    for name in F.VG_CASES:
        yield "value_grad " + name, F.vg_case(name), None, "vg", 1, F.RFF_GROUPS
    for name in F.REFINE_CASES:
        c = F.refine_case(name)
        yield "refine " + name, c, _refine_points(c), "refine", c["nw"], F.RFF_GROUPS


def test_rff_constants_are_the_measured_ones(capsys):
    """Per group the worst err / (u S) of the float64 run against the longdouble one over every case: recorded a quarter
    above it (between 1.1 and 1.5 x), RFF_C = 4 x recorded.  The kind 1 layers on a given fprev (mobocmf_rff_eval) and the
    one-step model of the refinement (its merit gradient; fs and slack_min at the float64 run's own xs) are measured too.
    Prints per case the ratios and the median S / |value|: what the gate can see."""
    worst = {g: (0.0, None) for g in F.RFF_GROUPS}

    def note(label, w):
        for g, v in w.items():
            if v > worst[g][0]:
                worst[g] = (v, label)

    with capsys.disabled():
        print()
        for label, c, x, order, nw, names in _runs():
            ref, S = F.rff_chain_ref(c, x), F.rff_chain_ref(c, x, shadow=True)
            _, w, _ = F.rff_gate(F.rff_chain_ref(c, x, dtype=np.float64, order=order, nw=nw), ref, S, names)
            note(label, w)
            print("%-34s %s   median S / |.|: %s" % (label, "  ".join("%s %.2f" % kv for kv in w.items()),
                                                      "  ".join("%s %.3g" % (g, F.seen(ref, S, g)) for g in names)))
        for name in F.EVAL1_CASES:
            c, k, l, fp = F.eval1_case(name)
            ref, S = F.rff_layer1_ref(c, k, l, fp), F.rff_layer1_ref(c, k, l, fp, shadow=True)
            _, w, _ = F.rff_gate(F.rff_layer1_ref(c, k, l, fp, dtype=np.float64, order="eval"), ref, S, ("value",))
            note("eval kind 1 " + name, w)
            print("%-34s value %.2f   median S / |.|: value %.3g" % ("eval kind 1 " + name, w["value"], F.seen(ref, S, "value")))
        for name in F.REFINE_CASES:
            c = F.refine_case(name)
            bad, w, report = F.rff_refine_gate(c, F.rff_refine_step_f64(c))
            assert bad == [], (name, bad)
            note("refine step " + name, dict(value=w["value"]))
            for p in range(c["P"]):                                           # the merit gradient, combined per thread
                x = F._clamp(c["x0"][p])
                hp, lo = F._merit_at(c, p, x, np.longdouble), F._merit_at(c, p, x, np.float64, "refine", c["nw"])
                _, wg, _ = F.rff_gate(dict(grad=lo["g"]), dict(grad=hp["g"]), dict(grad=hp["S_g"]), ("grad",))
                note("merit gradient %s problem %d" % (name, p), wg)
                report += "  merit gradient %d: %.2f" % (p, wg["grad"])
            print("%-34s %s" % ("refine step " + name, report))
        for g, (v, label) in worst.items():
            print("rff group %-6s measured %.3f u S (%s), recorded %.3f" % (g, v, label, F.RFF_RATIO_MEASURED[g]))
    for g, (v, _) in worst.items():
        assert 1.1 * v <= F.RFF_RATIO_MEASURED[g] <= 1.5 * v, (g, v)
        assert F.RFF_C[g] == 4 * F.RFF_RATIO_MEASURED[g]


def test_the_cases_are_what_their_names_say():
    """The cancelling case: sum |theta cos| is about 1e6 x |f| (within 0.5e6 .. 2e6) at every point; the short-lengthscale case: arguments of order 1e3;
    a NaN word in front of every operand and behind the last; the mixed launch has depths 1, 3, 2, every F edge, and layers that differ in F within a chain."""
    c = F.eval_case("cancel_d3_F65_n5_L1")
    op = c["ops"][0][0]
    mag = (np.abs(op["theta"])[None, :] * np.abs(np.cos(c["x"] @ op["W1"].T + op["b1"]))).sum(1) * op["s0"]
    f = np.abs(np.asarray(F.rff_chain_ref(c)["value"][0], np.float64))
    assert np.all((mag / f > 0.5e6) & (mag / f < 2e6)), (mag / f)
    c = F.eval_case("short_d2_F65_n257_L2")
    a = np.abs(c["x"] @ c["ops"][0][0]["W1"].T)
    assert 300 < np.median(a) < 3000 and a.max() > 1e3
    for c in [F.eval_case(n) for n in F.EVAL_CASES] + [F.vg_case(n) for n in F.VG_CASES] + [F.refine_case(n) for n in F.REFINE_CASES]:
        p = c["params"]
        assert np.isnan(p[0]) and np.isnan(p[-1])
        for chain, ops in zip(c["layers"], c["ops"]):
            for e, op in zip(chain, ops):
                for name in ("W1", "b1", "theta") + (("Wf", "W2", "b2") if e["kind"] else ()):
                    n = np.size(op[name])
                    assert np.isnan(p[e[name] - 1]) and np.isnan(p[e[name] + n]) and np.isfinite(p[e[name]:e[name] + n]).all()
                    assert np.array_equal(p[e[name]:e[name] + n], np.ravel(op[name]))
    assert [len(Fs) for Fs in F.MIXED] == [1, 3, 2] and all(len(set(Fs)) == len(Fs) for Fs in F.MIXED)
    assert {f for Fs in F.MIXED for f in Fs} == {1, 63, 64, 65, 129} and len({Fs[-1] for Fs in F.MIXED}) > 1


def test_one_step_model_conditions_hold_on_every_start():
    """rff_refine_step_ref asserts, in longdouble, that every decision of the kernel clears its own gate at every start; here it
    runs on every case, nothing is left out, both kinds of start occur, and exactly one component is clamped."""
    starts, kinds, clamped = 0, set(), 0
    for name, kw in F.REFINE_CASES.items():
        c = F.refine_case(name)
        model = F.rff_refine_step_ref(c)
        assert len(model) == c["P"] == (2 if kw["C"] else 1)
        for p, m in enumerate(model):
            assert m["xs"].shape == (F.REFINE_R, c["d"]) and m["feasible"] == (p == 0)
            starts += m["xs"].shape[0]
            kinds.add((m["feasible"], min(kw["C"], 1)))
            clamped += int(m["clamped"].sum())
            assert np.all(m["xs_bound"][~m["clamped"]] > 0) and np.all(m["xs_bound"] < 1e-12)
    assert starts == sum(F.REFINE_R * (2 if kw["C"] else 1) for kw in F.REFINE_CASES.values())
    assert kinds == {(True, 0), (True, 1), (False, 1)} and clamped == 1


def _defect_runs(defect):
    """The float64 runs a defect is planted in: (label, violations of the gate with the defect, without it)."""
    if defect in ("wave_value_dropped", "wave_grad_dropped", "merit_sign_flipped"):
        for name in F.REFINE_CASES:
            c = F.refine_case(name)
            yield "refine step " + name, F.rff_refine_gate(c, F.rff_refine_step_f64(c, defect))[0], F.rff_refine_gate(c, F.rff_refine_step_f64(c))[0]
        if defect == "merit_sign_flipped":
            return
    for label, c, x, order, nw, names in _runs():
        ref, S = F.rff_chain_ref(c, x), F.rff_chain_ref(c, x, shadow=True)
        run = lambda df: F.rff_gate(F.rff_chain_ref(c, x, dtype=np.float64, order=order, nw=nw, defect=df), ref, S, names)[0]
        yield label, run(defect), run(None)
    for name in F.EVAL1_CASES:
        c, k, l, fp = F.eval1_case(name)
        ref, S = F.rff_layer1_ref(c, k, l, fp), F.rff_layer1_ref(c, k, l, fp, shadow=True)
        run = lambda df: F.rff_gate(F.rff_layer1_ref(c, k, l, fp, dtype=np.float64, order="eval", defect=df), ref, S, ("value",))[0]
        yield "eval kind 1 " + name, run(defect), run(None)


@pytest.mark.parametrize("defect", F.RFF_DEFECTS)
def test_the_gate_reports_every_planted_defect(defect):
    """Each defect, planted in the float64 run, violates the gate on at least one case; the clean float64 run passes on all."""
    caught = []
    for label, bad, clean in _defect_runs(defect):
        assert clean == [], (label, clean)
        if bad:
            caught.append(label)
    print(defect, "reported on", caught)
    assert caught, defect
    if defect in ("wave_value_dropped", "wave_grad_dropped"):                # value and gradient separately: each on a one-step case
        assert any(l.startswith("refine step") for l in caught), caught


def test_agrees_with_the_oracle_feature_maps():
    """The values of the float64 run of the statement against theta @ Phi of oracle/rff_oracle.py (alpha = s^2 F / 2, nu = 1),
    layer by layer, inside 1e-13 sum |theta||Phi| (+ the layer below's difference through |D|)."""
    for c in (F.eval_case("mixed_d3_K3_n257"), F.eval_case("d8_F65_n257_L2"), F.vg_case("d9_F65_n5_L3")):
        run = F.rff_chain_ref(c, dtype=np.float64)
        for k, ops in enumerate(c["ops"]):
            f = None
            for l, op in enumerate(ops):
                Fn = op["F"]
                al = lambda s: s * s * Fn / 2.0
                if l == 0:
                    Phi = RO.layer0_features(c["x"], op["W1"], op["b1"][:, None], al(op["s0"]))
                else:
                    Phi = RO.layer1_features(c["x"], f, op["W1"], op["Wf"], op["W2"], op["b1"][:, None], op["b2"][:, None],
                                             al(op["s0"]), (op["s1"] / op["s0"]) ** 2, al(op["s2"]), 1.0)
                f = op["theta"] @ Phi
                got = run["layers"][k][l]["value"]
                assert np.all(np.abs(got - f) <= 1e-12 * (np.abs(op["theta"]) @ np.abs(Phi) + 1)), (c["name"], k, l)
                f = got


def test_gradient_and_D_agree_with_central_differences():
    """The longdouble gradient of every layer against central differences of the longdouble value (h = 2^-20: the truncation
    is h^2 |f'''| / 6 ~ 1e-10 at these lengthscales, the rounding u_ld |f| / h ~ 1e-13)."""
    h = 2.0 ** -20
    for c in (F.vg_case("mixed_d3_K3_n5"), F.vg_case("d9_F65_n5_L3"), F.vg_case("d2_F63_n3_L2")):
        ref = F.rff_chain_ref(c)
        for k in range(c["d"]):
            e = np.zeros(c["d"])
            e[k] = h
            up, dn = F.rff_chain_ref(c, c["x"] + e), F.rff_chain_ref(c, c["x"] - e)
            for ch in range(c["K"]):
                for l in range(len(c["chains"][ch])):
                    fd = (up["layers"][ch][l]["value"] - dn["layers"][ch][l]["value"]) / (2 * R.ld(h))
                    g = ref["layers"][ch][l]["grad"][:, k]
                    scale = np.abs(ref["layers"][ch][l]["grad"]).max() + 1
                    assert np.all(np.abs(fd - g) <= 1e-6 * scale), (c["name"], ch, l, k, float(np.abs(fd - g).max()))
