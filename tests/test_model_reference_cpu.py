"""CPU proof behind tests/test_hip_one_launch_conformance.py ("The model bound"): on every case the GPU file runs,
the conditions on every layer's inputs, both measured ratios behind MODEL_RATIO_MEASURED per depth and group, the hand-composed
longdouble backward against central differences and against the oracle's autograd, and mutations of the checker's input."""
import time

import numpy as np
import pytest

from tests import kernel_reference as R

pytestmark = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason="numpy.longdouble is no wider than float64 here")


def _what(mc):
    return "input" if mc["predict"] else "gradients"


def test_every_layer_of_every_case_meets_the_conditions_on_the_inputs():
    """cond(K_mm + jitter I) <= LAYER_COND_MAX for every Z~_l = [Z_x, m_{l-1}]; in every layer every clamp decision and every
    floor decision LAYER_MARGIN away from a rounding error: |k_nn - q| and varraw - min_var at least 1e-9 of the magnitudes they
    are formed from (k_nn + q, k_nn + q + r) AND at least a thousand gates C_forward u S_var of the composed shadow, which at
    L >= 2 also carries the error of f; no column on the floor; the rows meant to clamp are clamped in every layer that holds
    them, with half the jitter as margin; without such rows no column clamps."""
    for name, kw in R.all_model_cases().items():
        mc = R.model_case(**kw)
        for l, (lc, st, sst) in enumerate(R._model_forward(mc, R._f64)):
            assert np.linalg.cond(st["Kmm"]) <= R.LAYER_COND_MAX, (name, l)
            s = st["knn"] - st["q"]
            gates = 1e3 * R.MODEL_C[mc["L"]]["forward"] * R.U * sst["varraw"]
            assert np.all(np.abs(s) >= np.maximum(R.LAYER_MARGIN * (st["knn"] + st["q"]), gates)), (name, l)
            assert np.all(st["varraw"] - lc["min_var"] >= np.maximum(R.LAYER_MARGIN * (st["knn"] + st["q"] + st["r"]), gates)), (name, l)
            n = min(mc["clamp"], mc["rows"][l]) * lc["xdiv"]
            assert np.all(s[:n] < 0) and np.all(-s[:n] >= -0.5 * R.CLAMP_JITTER), (name, l, s[:n])
            # (under the negative jitter a row that happens to lie as close to an inducing row clamps too, by the same margins)
            assert mc["branch"] == 1 or ((n == lc["Np"] or np.any(s[n:] > 0)) if mc["clamp"] else np.all(s > 0)), (name, l)
        assert mc["predict"] or mc["kl_scale"] not in (0.0, 1.0)
    assert any(0.0 not in set(R.model_case(**kw)["fid"].tolist()) for kw in R.MODEL_TINY_CASES.values())          # a level no row has
    assert any(1.0 not in set(R.model_case(**kw)["fid"].tolist()) and kw["L"] == 3 for kw in R.MODEL_TINY_CASES.values())


def test_model_constants_are_the_measured_ones(capsys):
    """Per depth L and output group the worst err / (u S) of the float64 run of model_ref and of float64 autograd over the
    oracle against the longdouble reference, over every case of the GPU file: recorded >= measured (so the oracle's autograd,
    an independent derivation of the composed backward, agrees with the hand-composed one within a quarter of the gate) and
    recorded <= 2 x measured.  Components with S = 0 are exactly zero in both.  Prints the medians of S / |value| per output."""
    t0 = time.time()
    worst = {L: {g: {"restatement": 0.0, "oracle": 0.0} for g in R.MODEL_GROUPS} for L in (1, 2, 3)}
    strength = {L: {} for L in (1, 2, 3)}
    for name, kw in R.all_model_cases().items():
        mc = R.model_case(**kw)
        ref, S, names = R.model_ref(mc), R.model_ref(mc, shadow=True), R.model_names(mc, _what(mc))
        for who, got in (("restatement", R.model_ref(mc, np.float64)), ("oracle", R.model_oracle(mc))):
            for k, (ratio, nonzero) in R.layer_ratios(got, ref, S, names).items():
                assert nonzero == 0, (name, who, k)
                g = R.model_group(k)
                worst[mc["L"]][g][who] = max(worst[mc["L"]][g][who], ratio)
        for k in names:
            r, s = np.abs(np.asarray(ref[k], np.float64)).ravel(), np.asarray(S[k], np.float64).ravel()
            if (r > 0).any():
                strength[mc["L"]].setdefault(k, []).append(float(np.median(s[r > 0] / r[r > 0])))
    with capsys.disabled():
        print()
        for L, t in worst.items():
            for g, w in t.items():
                print("model L = %d group %-8s restatement %.2f u S, oracle %.2f u S (recorded %.2f)" % (L, g, w["restatement"], w["oracle"], R.MODEL_RATIO_MEASURED[L][g]))
            for k, v in strength[L].items():
                print("  L = %d  S / |value| medians of %-8s %.3g .. %.3g" % (L, k, min(v), max(v)))
        print("measured in %.1f s" % (time.time() - t0))
    for L, t in worst.items():
        for g, w in t.items():
            measured = max(w.values())
            assert measured <= R.MODEL_RATIO_MEASURED[L][g] <= 2 * measured, (L, g, w)
            assert R.MODEL_C[L][g] == 4 * R.MODEL_RATIO_MEASURED[L][g]


def _perturbed(mc, key, l, idx, h):
    a = R.ld(mc[key] if l is None else mc[key][l]).copy()
    a[idx] += h
    return dict(mc, **{key: a if l is None else [a if i == l else v for i, v in enumerate(mc[key])]})


def test_longdouble_backward_matches_central_differences():
    """The hand-composed backward -- through the ELBO, the propagation, g_zf[l] -> g_m[l-1], softplus and Interval -- against
    central differences of the longdouble forward (step 1e-6 of the input's scale, Richardson once): 6 random components per
    block of the flat gradient on the three smallest training cases (one with clamped rows, row weights and seeds among them)
    and the input gradient of the smallest prediction case agree to 1e-9 S."""
    cases = R.all_model_cases()
    size = lambda kw: kw["M"] ** 2 * kw["L"] + kw["M"] * sum(kw["rows"]) * kw["S"]
    train = sorted((n for n, kw in cases.items() if not kw.get("predict")), key=lambda n: size(cases[n]))[:3] + ["weights_seeds", "clamp"]
    for name in train + ["M7_L1_d2"]:
        mc = R.model_case(**cases[name])
        ref, S = R.model_ref(mc), R.model_ref(mc, shadow=True)
        rng = np.random.default_rng(5)
        if mc["predict"]:
            blocks = [("g_x", "x", None)]
        else:
            blocks = [(k, {"g_hyp": "raw", "g_m": "m", "g_LS": "L_S"}[k.rstrip("0123456789")], int(k[-1])) for k, _, _ in R.model_layout(mc)[:-1]]
            blocks += [("g_noise", "raw_noise", None)]
        for out, key, l in blocks:
            src = np.asarray(mc[key] if l is None else mc[key][l], np.float64)
            idx = np.argwhere(np.tril(np.ones(src.shape)) > 0) if key == "L_S" else np.argwhere(np.ones(src.shape) > 0)
            for i in idx[rng.permutation(len(idx))[:6]]:
                i = tuple(i)
                D = lambda h: (R._model_run(_perturbed(mc, key, l, i, h), R.ld, True) - R._model_run(_perturbed(mc, key, l, i, -h), R.ld, True)) / (2 * h)
                h = R.ld(1e-6) * max(abs(float(src[i])), 0.1)
                fd = (4 * D(h / 2) - D(h)) / 3
                assert abs(fd - ref[out][i]) <= R.ld(1e-9) * S[out][i], (name, out, i, float(fd), float(ref[out][i]), float(S[out][i]))


def test_the_checker_trips_on_small_defects():
    """Defects the normwise 1e-5 gates let through: one lengthscale-gradient component off by 1e-10 S, one L_S entry off by 1e-12
    S, g_m of layer 1 replaced by layer 0's, the g_zf share of g_m[l-1] dropped, a non-zero in an upper triangle, and the noise
    gradient of the level no row has made non-zero."""
    mc = R.named_model_case("M17_L2_d1")                       # level 0 has no row
    ref, S, names = R.model_ref(mc), R.model_ref(mc, shadow=True), R.model_names(mc, "gradients")
    C = R.MODEL_C[mc["L"]]
    good = {k: np.asarray(ref[k], np.float64).copy() for k in names}
    assert R.model_gate(good, ref, S, names, C)[0] == []
    assert S["g_noise"][0] == 0 and S["g_noise"][1] > 0

    def tripped(change):
        g = {k: v.copy() for k, v in good.items()}
        change(g)
        return [b[0] for b in R.model_gate(g, ref, S, names, C)[0]]

    def bump(name, idx, rel):
        def f(g):
            g[name][idx] += rel * float(S[name][idx])
        return f

    def swap_m(g):
        g["g_m1"] = g["g_m0"].copy()

    def drop_share(g):
        g["g_m0"] = g["g_m0"] - np.asarray(ref["g_zf1"], np.float64)

    def upper(g):
        g["g_LS1"][2, 9] = 1e-300

    def noise(g):
        g["g_noise"][0] = 1e-300

    assert tripped(bump("g_hyp1", 5, 1e-10)) == ["g_hyp1"]                              # ls1[0] of layer 1
    assert tripped(bump("g_hyp0", 1, 1e-10)) == ["g_hyp0"]
    assert tripped(bump("g_LS0", (9, 2), 1e-12)) == ["g_LS0"]
    assert tripped(swap_m) == ["g_m1"] and tripped(drop_share) == ["g_m0"]
    assert tripped(upper) == ["g_LS1"] and tripped(noise) == ["g_noise"]
    # the same on a three-layer case at M = 5, where all layers' m share a wavefront of the cooperative gradient assembly
    mc = R.named_model_case("M5_L3_d2")
    ref, S, names = R.model_ref(mc), R.model_ref(mc, shadow=True), R.model_names(mc, "gradients")
    good = {k: np.asarray(ref[k], np.float64).copy() for k in names}
    for l in (1, 2):
        g = {k: v.copy() for k, v in good.items()}
        g["g_m%d" % l] = good["g_m0"].copy()
        assert [b[0] for b in R.model_gate(g, ref, S, names, R.MODEL_C[3])[0]] == ["g_m%d" % l]
