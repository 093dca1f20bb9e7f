"""CPU proof behind tests/test_hip_layer_conformance.py ("The layer bound"): on every case the GPU tests run, the
conditions on the inputs, both measured ratios behind LAYER_RATIO_MEASURED, and the hand-derived longdouble backward."""
import numpy as np
import pytest

from tests import kernel_reference as R

pytestmark = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason="numpy.longdouble is no wider than float64 here")


def _runs():
    """Every (case, tag) the GPU tests compare against the reference: the cases with their full upstream gradient, the
    separate upstream gradients, the column-activity patterns."""
    out = [(R.layer_case(*k), "all") for k in R.all_layer_cases()]
    for k in R.LAYER_UPSTREAM_CASES:
        c = R.layer_case(*k)
        out += [(R.with_upstream(c, c["g_mean"], None, 0.0, tag="mean"), "mean"), (R.with_upstream(c, None, c["g_var"], 0.0, tag="var"), "var"),
                (R.with_upstream(c, None, None, c["g_kl"], tag="kl"), "kl"),
                (R.with_upstream(c, c["g_mean"], c["g_var"], 1e-4, tag="kl_small"), "kl_small")]
    for k in R.LAYER_ACTIVITY_CASES:
        out += [(R.activity_case(R.layer_case(*k), p)[0], p) for p in R.LAYER_ACTIVITY]
    return out


def test_every_case_meets_the_conditions_on_the_inputs():
    """cond(K_mm + jitter I) <= 1e3; no clamp decision within 1e-9 of a rounding error: |k_nn - q| >= 1e-9 (k_nn + q) and
    |varraw - min_var| >= 1e-9 S_var in every column; the columns meant to clamp have k_nn - q below half the (negative) jitter; the floor cases
    have columns on the floor and columns above it."""
    for k in R.all_layer_cases():
        c = R.layer_case(*k)
        Kmm = R._gram(c["kind"], R._gram_operands(c)[0], 1, R._f64)[0] + c["jitter"] * np.eye(c["M"])
        assert np.linalg.cond(Kmm) <= R.LAYER_COND_MAX, k
        st, sst = R._layer_forward(c, R._f64)
        s = st["knn"] - st["q"]
        assert np.all(np.abs(s) >= R.LAYER_MARGIN * (st["knn"] + st["q"])), k
        assert np.all(np.abs(st["varraw"] - c["min_var"]) >= R.LAYER_MARGIN * sst["varraw"]), k
        n = c["clamp"] * c["xdiv"]
        if n:
            assert np.all(s[:n] < 0) and np.all(-s[:n] >= -0.5 * R.CLAMP_JITTER) and np.any(s > 0), k
        else:
            assert c["branch"] == 1 or np.all(s > 0), k
        on_floor = int((st["varraw"] < c["min_var"]).sum())
        assert (0 < on_floor < c["Np"]) if c["floor"] else on_floor == 0, k


def test_layer_constants_are_the_measured_ones(capsys):
    """The worst err / (u S) per output group of the float64 run of layer_ref and of float64 autograd over the oracle, against
    the longdouble reference, over every run of the GPU tests: LAYER_RATIO_MEASURED records the larger of the two (recorded >=
    measured, recorded <= 2 x measured), so the oracle's autograd -- an independent derivation of the backward -- agrees with
    the hand-derived one within a quarter of the gate.  Components with S = 0 are exactly zero in both."""
    worst = {g: {"restatement": 0.0, "oracle": 0.0} for g in R.LAYER_GROUPS}
    strength = {}
    for c, tag in _runs():
        ref, S, names = R.layer_ref(c), R.layer_ref(c, shadow=True), R.layer_names(c)
        for who, got in (("restatement", R.layer_ref(c, np.float64)), ("oracle", R.layer_oracle(c))):
            for k, (ratio, nonzero) in R.layer_ratios(got, ref, S, names).items():
                assert nonzero == 0, (c["key"], who, k)
                g = R.layer_group(k)
                worst[g][who] = max(worst[g][who], ratio)
        for k in names:
            r, s = np.abs(np.asarray(ref[k], np.float64)).ravel(), np.asarray(S[k], np.float64).ravel()
            if (r > 0).any():
                strength.setdefault(k, []).append(float(np.median(s[r > 0] / r[r > 0])))
    with capsys.disabled():
        print()
        for g, w in worst.items():
            print("layer group %-8s restatement %.2f u S, oracle %.2f u S (recorded %.1f)" % (g, w["restatement"], w["oracle"], R.LAYER_RATIO_MEASURED[g]))
        for k, v in strength.items():
            print("S / |value| medians of %-6s %.3g .. %.3g" % (k, min(v), max(v)))
    for g, w in worst.items():
        measured = max(w.values())
        assert measured <= R.LAYER_RATIO_MEASURED[g] <= 2 * measured, (g, w)
        assert R.LAYER_C[g] == 4 * R.LAYER_RATIO_MEASURED[g]


def _objective(c):
    st = R._layer_forward(c, R.ld)[0]
    return (R.ld(c["g_mean"]) * st["mean"]).sum() + (R.ld(c["g_var"]) * st["var"]).sum() + R.ld(c["g_kl"]) * st["kl"]


def test_longdouble_backward_matches_central_differences():
    """The hand-derived backward against central differences of the longdouble forward (step 1e-6 of the input's scale,
    Richardson once): 20 random components per output on the three smallest cases agree to 1e-9 S."""
    inputs = {"g_m": "m", "g_LS": "L_S", "g_hyp": "hyp", "g_x": "x", "g_f": "f", "g_zf": "zf"}
    small = sorted(R.LAYER_CASES, key=lambda k: k[2] * k[3] * k[4])[:3]
    for k in small:
        c = R.layer_case(*k)
        ref, S = R.layer_ref(c), R.layer_ref(c, shadow=True)
        rng = np.random.default_rng(5)
        for name in R.layer_names(c)[3:]:
            src = c[inputs[name]]
            idx = np.argwhere(np.tril(np.ones(src.shape)) > 0) if name == "g_LS" else np.argwhere(np.ones(src.shape) > 0)
            for i in idx[rng.permutation(len(idx))[:20]]:
                i = tuple(i)
                def D(h):
                    vals = []
                    for sgn in (1, -1):
                        a = R.ld(src).copy()
                        a[i] += sgn * h
                        vals.append(_objective(dict(c, **{inputs[name]: a})))
                    return (vals[0] - vals[1]) / (2 * h)
                h = R.ld(1e-6) * max(abs(float(src[i])), 0.1)
                fd = (4 * D(h / 2) - D(h)) / 3
                assert abs(fd - ref[name][i]) <= R.ld(1e-9) * S[name][i], (k, name, i, float(fd), float(ref[name][i]))


def test_the_checker_trips_on_small_defects():
    """Defects of the size the old 1e-7 gates let through: one component of g_hyp off by 1e-10 of its S, one entry of g_LS
    off by 1e-12 S, one column of mean in a padded tail off by 1e-11 S, and a backward whose Phi keeps its whole diagonal."""
    c = R.layer_case(*R.LAYER_CASES[10])                        # kind 0, M = 129, N' = 300: the last column block is partial
    ref, S, names = R.layer_ref(c), R.layer_ref(c, shadow=True), R.layer_names(c)
    good = {k: np.asarray(ref[k], np.float64) for k in names}
    assert R.layer_gate(good, ref, S, names)[0] == []

    def bumped(name, idx, rel):
        g = {k: v.copy() for k, v in good.items()}
        g[name][idx] += rel * float(S[name][idx])
        return g

    assert [b[0] for b in R.layer_gate(bumped("g_hyp", 1, 1e-10), ref, S, names)[0]] == ["g_hyp"]
    assert [b[0] for b in R.layer_gate(bumped("g_LS", (100, 3), 1e-12), ref, S, names)[0]] == ["g_LS"]
    assert [b[0] for b in R.layer_gate(bumped("mean", 299, 1e-11), ref, S, names)[0]] == ["mean"]
    g = {k: v.copy() for k, v in good.items()}
    g["g_LS"][3, 100] = 1e-300                                  # S = 0 there: only an exact zero passes
    assert [b[0] for b in R.layer_gate(g, ref, S, names)[0]] == ["g_LS"]
    st, sst = R._layer_forward(c, R.ld)
    wrong = R._layer_backward(c, st, sst, R.ld, phi_diag=1.0)[0]
    g = dict(good, g_hyp=np.asarray(wrong["g_hyp"], np.float64))
    assert [b[0] for b in R.layer_gate(g, ref, S, names)[0]] == ["g_hyp"]
