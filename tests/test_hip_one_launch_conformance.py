"""mobocmf_tiny_elbo_step and mobocmf_coop_elbo_step -- the whole ELBO step in one launch (tiny_step.hip, coop_step.hip) --
through the C ABI directly, every component of out, top_mean / top_var, the flat gradient and the input gradient within
C_g u S of the longdouble model reference (tests/kernel_reference.py, model_ref; DESIGN.md 5.5, "The model bound"), exact zeros
where S = 0, on both sides of every switch of the two launch geometries; Adam's arithmetic on the device's own gradient;
nothing written that a mode does not own; the refused arguments.  The constants are measured on the CPU
(tests/test_model_reference_cpu.py), never on the device."""
import numpy as np
import pytest

from tests import kernel_reference as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason="numpy.longdouble is no wider than float64 here")]

KERNELS = ("tiny", "coop")
TINY_NAMES = list(R.MODEL_TINY_CASES) + list(R.MODEL_FEATURE_CASES)
# (case, wgs_per_model): 0 = the library's choice; 8 at M = 5, L = 3 is more than the widest phase has tasks (3 chain blocks)
COOP_RUNS = [(n, 0) for n in R.MODEL_COOP_CASES] + [("M5_L3_d2", 1), ("M5_L3_d2", 3), ("M5_L3_d2", 8), ("M65_L2_d8_N272", 1),
                                                    ("M65_L2_d8_N272", 3)] + [(n, 0) for n in R.MODEL_FEATURE_CASES]
# the restated switches (kernel_reference.tiny_geometry / coop_geometry): the cases named for a side are on it
TINY_SIDES = {"M1_L1_d1": (16, 256, True), "M7_L2_d2_S3": (16, 256, True), "M16_L3_d8_S8": (16, 512, True), "M16_L1_d2": (16, 256, True),
              "M16_L2_d8_wide": (16, 512, False), "M17_L2_d1": (32, 256, True), "M20_L3_d2_S3": (32, 256, True),
              "M32_L2_d8_S3": (32, 512, False), "M32_L1_d8_512": (32, 256, True), "M32_L1_d8_544": (32, 512, True)}
COOP_SIDES = {"M5_L3_d2": [(True, 1)] * 3, "M16_L1_d1_N129": [(False, 1)], "M17_L2_d8_N130": [(False, 1), (True, 3)],
              "M48_L2_d8_S8": [(True, 4), (False, 1)], "M64_L2_d2_N128": [(True, 8), (True, 1)], "M65_L2_d8_N272": [(False, 2), (True, 7)],
              "M127_L2_d8_N144": [(False, 1), (False, 1)], "M16_L2_d8_N1040": [(False, 4), (True, 2)]}


def _call(kernel, mcs, mode, wgs=0, **kw):
    return R.coop_direct(mcs, mode, wgs, **kw) if kernel == "coop" else R.tiny_direct(mcs, mode, **kw)


def _gate(mc, r, what, label):
    """Asserts the gate on model ``mc``'s results ``r`` and prints the worst err / (u S) per group with its share."""
    ref, S, names = R.model_ref(mc), R.model_ref(mc, shadow=True), R.model_names(mc, what)
    bad, worst, report = R.model_gate(R.model_got(mc, r, what), ref, S, names, R.MODEL_C[mc["L"]])
    print("%s: %s" % (label, report))
    assert bad == [], (label, bad)
    return worst


def _clean(call, i=0):
    assert call.rc == 0 and call.status == 0, (call.rc, call.status)
    assert call.guards[i], "a guard behind an output of model %d was written" % i
    assert (call.res[i]["info"] == 0).all(), call.res[i]["info"]


def _upper_zero(mc, r):
    for k, v in R.model_split(mc, r["grad"]).items():
        if k.startswith("g_LS"):
            assert not np.triu(v, 1).any(), k


def test_the_cases_sit_on_the_sides_they_are_named_for():
    for n, side in TINY_SIDES.items():
        assert R.tiny_geometry([R.named_model_case(n)]) == side, n
    for n, side in COOP_SIDES.items():
        assert R.coop_geometry(R.named_model_case(n)) == side, n
    assert R.tiny_geometry([R.named_model_case(n) for n in R.MODEL_GROUP_CASES["tiny"]])[0] == 32


@pytest.mark.parametrize("name", TINY_NAMES)
def test_tiny_gradients(name):
    """GRADIENTS: out, top_mean / top_var and the whole flat gradient inside the gate, the strict upper triangles exactly
    zero, parameters, Adam state, steps_done and the rng words bitwise unchanged."""
    mc = R.named_model_case(name)
    call = R.OneLaunch([mc], False, adam_seed=3, steps=7)
    before = call.snapshot()
    call.launch(R.STEP_GRADIENTS)
    _clean(call)
    _gate(mc, call.res[0], "gradients", "tiny %s MR %d, %d threads, pool in LDS %s" % ((name,) + R.tiny_geometry([mc])))
    _upper_zero(mc, call.res[0])
    assert call.changed(before) == [[]]


@pytest.mark.parametrize("name,wgs", COOP_RUNS)
def test_coop_gradients(name, wgs):
    mc = R.named_model_case(name)
    call = R.OneLaunch([mc], True, adam_seed=3, steps=7)
    before = call.snapshot()
    call.launch(R.STEP_GRADIENTS, wgs)
    _clean(call)
    assert call.wgs_used == wgs if wgs else 1 <= call.wgs_used <= 32
    _gate(mc, call.res[0], "gradients", "coop %s wgs %d (hblk, ks) %s" % (name, call.wgs_used, R.coop_geometry(mc)))
    _upper_zero(mc, call.res[0])
    assert call.changed(before) == [[]]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["M7_L2_d2_S3", "M32_L2_d8_S3", "weights_seeds"])
def test_forward_training_branch(kernel, name):
    """FORWARD with branch = 0: the forward group; nothing but out, top_*, info and work written."""
    mc = R.named_model_case(name)
    call = R.OneLaunch([mc], kernel == "coop", adam_seed=3, steps=7)
    before = call.snapshot()
    call.launch(R.STEP_FORWARD)
    _clean(call)
    _gate(mc, call.res[0], "forward", "%s FORWARD %s" % (kernel, name))
    assert call.changed(before) == [[]] and set(call.written[0]) <= {"out", "top_mean", "top_var", "info", "work"}


def _predict_names(kernel):
    return [n for n in R.MODEL_PREDICT_CASES if kernel == "coop" or R.MODEL_PREDICT_CASES[n]["M"] <= 32]


@pytest.mark.parametrize("kernel,name", [(k, n) for k in KERNELS for n in _predict_names(k)])
def test_prediction_forward_and_input_gradients(kernel, name):
    """branch = 1, eps tiled over the test points.  FORWARD: the forward group, nothing else written.  INPUT_GRADIENTS: the N x d
    gradient in the Gram-derived group, rows without a seed exactly zero, nothing but grad (N d doubles), out, top_*, info and
    work written; coop: the same launch once more with MOBOCMF_STEP_CHAIN_VALID, bitwise equal."""
    mc = R.named_model_case(name)
    call = R.OneLaunch([mc], kernel == "coop", adam_seed=3, steps=7)
    before = call.snapshot()
    call.launch(R.STEP_FORWARD)
    _clean(call)
    _gate(mc, call.res[0], "forward", "%s FORWARD branch 1 %s" % (kernel, name))
    assert call.changed(before) == [[]] and set(call.written[0]) <= {"out", "top_mean", "top_var", "info", "work"}
    call.launch(R.STEP_INPUT_GRADIENTS)
    _clean(call)
    _gate(mc, call.res[0], "input", "%s INPUT_GRADIENTS %s" % (kernel, name))
    gx = call.res[0]["g_x"]
    unseeded = np.arange(mc["N"]) % 3 == 1
    assert not gx[unseeded].any() and gx[~unseeded].all()
    assert call.changed(before) == [[]]
    if kernel == "coop":
        first = {k: v.copy() for k, v in call.res[0].items()}
        call.launch(R.STEP_INPUT_GRADIENTS | R.STEP_CHAIN_VALID, keep=("work", "info"))             # (the chain is not formed again: nor is info)
        _clean(call)
        for k in ("g_x", "top_mean", "top_var"):
            assert np.array_equal(call.res[0][k], first[k]), k
        assert call.changed(before) == [[]]


@pytest.mark.parametrize("kernel", KERNELS)
def test_three_models_of_different_shapes_in_one_launch(kernel):
    """Each model of a group passes its own gate and keeps its guards; tiny: M = 7 runs in the MR = 32 instantiation."""
    mcs = [R.named_model_case(n) for n in R.MODEL_GROUP_CASES[kernel]]
    call = _call(kernel, mcs, R.STEP_GRADIENTS, adam_seed=3, steps=7)
    for i, mc in enumerate(mcs):
        _clean(call, i)
        _gate(mc, call.res[i], "gradients", "%s group model %d (%s)" % (kernel, i, R.MODEL_GROUP_CASES[kernel][i]))
        _upper_zero(mc, call.res[i])


# Adam as the kernels state it (torch.optim.Adam): m' = b1 m + (1 - b1) g; v' = b2 v + (1 - b2) g g; p' = p - (lr / bc1) m' /
# (sqrt(v') / sqrt(bc2) + eps), bc1 = 1 - b1^t, bc2 = 1 - b2^t, t = steps_done + 1.  Roundings per element, each at most one
# spacing of the magnitude it rounds:
#   m'  two products, the 1 - b1, one sum whose terms may cancel: 4 spacings of |b1 m| + |(1 - b1) g|;
#   v'  three products, the 1 - b2, one sum of positive terms: 5 spacings of v';
#   d = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps), formed by the reference from the DEVICE's m' and v', so their errors do
#       not enter: bc = 1 - b^t is a pow (POW_ULP = 2: what device math libraries document for the double-precision pow)
#       whose error the subtraction amplifies by k = b^t / (1 - b^t) -- 0.75 for b1 and 124 for b2 at t = 8: this, not the
#       per-element arithmetic, is what the bound consists of -- plus the subtraction's own rounding: POW_ULP k + 1.
#       lr / bc1: one more, e1 = POW_ULP k1 + 2.  sqrt(bc2): half of bc2's plus its own, e2 = (POW_ULP k2 + 1) / 2 + 1.
#       Denominator (positive terms): sqrt(v') 1, the quotient 1, e2, the sum 1.  d: e1, the product with m' 1, the
#       denominator's 3 + e2, the quotient 1: e1 + e2 + 6 spacings of d;
#   p' = p - d: one spacing of p' and d's.
POW_ULP = 2
ADAM_ULP = {"m": 4, "v": 5}


def adam_step_spacings(t):
    b1, b2 = R.ADAM["beta1"], R.ADAM["beta2"]
    k1, k2 = b1 ** t / (1 - b1 ** t), b2 ** t / (1 - b2 ** t)
    return (POW_ULP * k1 + 2) + ((POW_ULP * k2 + 1) / 2 + 1) + 6


TRAINABLE = {"all": lambda L: [R.TRAIN_ALL] * L, "only_m": lambda L: [1 << 7] * L, "only_raw_noise_1": lambda L: [0, 1 << 9, 0][:L],
             "hyper_and_L_S_0": lambda L: [0x7F | 1 << 8] + [0] * (L - 1), "none": lambda L: [0] * L}


@pytest.mark.parametrize("steps", [0, 7])
@pytest.mark.parametrize("pattern", list(TRAINABLE))
@pytest.mark.parametrize("kernel", KERNELS)
def test_update_is_adam_on_the_device_gradient(kernel, pattern, steps):
    """GRADIENTS, then UPDATE from the same state (random non-zero adam_m / adam_v: from zero state the first step is -lr sign(g)
    and hides any gradient error): torch.optim.Adam's formula in longdouble on the device's OWN gradient gives parameters,
    adam_m and adam_v within the spacings derived above per element; steps_done advances by one; a tensor whose trainable bit is cleared is
    bitwise unchanged together with its Adam state."""
    mc = R.named_model_case(R.MODEL_UPDATE_CASES[kernel])
    bits = TRAINABLE[pattern](mc["L"])
    call = R.OneLaunch([mc], kernel == "coop", adam_seed=11, steps=steps, trainable=[bits])
    before = call.snapshot()
    call.launch(R.STEP_GRADIENTS)
    _clean(call)
    g = R.ld(call.res[0]["grad"])
    p0, m0, v0 = R.ld(call.params(0)), R.ld(before[0]["adam_m"].cpu().numpy()), R.ld(before[0]["adam_v"].cpu().numpy())
    assert call.changed(before) == [[]]
    call.launch(R.STEP_UPDATE)
    _clean(call)
    assert np.array_equal(call.res[0]["grad"], np.asarray(g, np.float64))           # the same gradient, to the bit
    p1, m1, v1 = call.params(0), call.state[0]["adam_m"].cpu().numpy(), call.state[0]["adam_v"].cpu().numpy()
    assert int(call.state[0]["steps_done"][0]) == steps + 1
    a, t = R.ADAM, steps + 1
    b1, b2 = R.ld(a["beta1"]), R.ld(a["beta2"])
    mr, vr = b1 * m0 + (1 - b1) * g, b2 * v0 + (1 - b2) * g * g
    dr = (R.ld(a["lr"]) / (1 - b1 ** t)) * R.ld(m1) / (np.sqrt(R.ld(v1)) / np.sqrt(1 - b2 ** t) + R.ld(a["eps"]))
    on = np.zeros(len(g), bool)
    for (name, lo, hi) in R.model_layout(mc):
        if name == "g_noise":
            on[lo:hi] = [bool(bits[l] >> 9 & 1) for l in range(mc["L"])]
        elif name.startswith("g_m"):
            on[lo:hi] = bool(bits[int(name[3:])] >> 7 & 1)
        elif name.startswith("g_LS"):
            on[lo:hi] = bool(bits[int(name[4:])] >> 8 & 1)
        else:                                                                        # the packed hyper-parameters: bit s per tensor
            l, d, o = int(name[5:]), mc["d"], lo
            for s, n in enumerate([1, d] if l == 0 else [1, 1, 1, 1, 1, d, d]):
                on[o:o + n] = bool(bits[l] >> s & 1)
                o += n
    ulp = lambda x: np.spacing(np.abs(np.asarray(x, np.float64)))
    off = ~on
    assert np.array_equal(p1[off], np.asarray(p0, np.float64)[off]) and np.array_equal(m1[off], np.asarray(m0, np.float64)[off])
    assert np.array_equal(v1[off], np.asarray(v0, np.float64)[off])
    if on.any():
        em = np.abs(R.ld(m1) - mr)[on] / ulp(np.abs(b1 * m0) + np.abs((1 - b1) * g))[on]
        ev = np.abs(R.ld(v1) - vr)[on] / ulp(vr)[on]
        ep = np.abs(R.ld(p1) - (p0 - dr))[on] / (ulp(p0 - dr)[on] + adam_step_spacings(t) * ulp(dr)[on])
        print("%s UPDATE %s steps_done %d: adam_m %.2f, adam_v %.2f spacings, parameters %.3f of the bound (%.1f spacings of the step)" % (kernel, pattern, steps, em.max(), ev.max(), ep.max(), adam_step_spacings(t)))
        assert em.max() <= ADAM_ULP["m"] and ev.max() <= ADAM_ULP["v"] and ep.max() <= 1
    changed = set(call.changed(before)[0])
    assert changed <= {"adam_m", "adam_v", "steps_done"} | {k for k in call.state[0] if k[:3] in ("raw", "m0", "m1", "m2", "L_S")}, changed


def _refusals(kernel):
    G, I = R.STEP_GRADIENTS, R.STEP_INPUT_GRADIENTS
    set_ = lambda k, v: (lambda recs: setattr(recs[0], k, v))

    def rows_up(recs):
        recs[0].rows[1] = recs[0].rows[0] + 1
    out = [("M_too_large", "M7_L2_d2_S3", G, 0, set_("M", 129 if kernel == "coop" else 33)), ("d9", "M7_L2_d2_S3", G, 0, set_("d", 9)),
           ("L4", "M7_L2_d2_S3", G, 0, set_("L", 4)), ("rows_not_descending", "M7_L2_d2_S3", G, 0, rows_up),
           ("input_gradients_without_grad", "M16_L2_d8_S3", I, 0, set_("grad", None))]
    if kernel == "coop":
        def no_seeds(recs):
            recs[0].seed_gmean = recs[0].seed_gvar = None
        out += [("input_gradients_without_seeds", "M16_L2_d8_S3", I, 0, no_seeds), ("chain_valid_on_gradients", "M7_L2_d2_S3", G | R.STEP_CHAIN_VALID, 0, None),
                ("chain_valid_on_update", "M7_L2_d2_S3", R.STEP_UPDATE | R.STEP_CHAIN_VALID, 0, None), ("wgs_65", "M7_L2_d2_S3", G, 65, None)]
    return out


@pytest.mark.parametrize("kernel,what", [(k, r[0]) for k in KERNELS for r in _refusals(k)])
def test_refused_arguments_write_nothing(kernel, what):
    _, name, mode, wgs, over = next(r for r in _refusals(kernel) if r[0] == what)
    call = R.OneLaunch([R.named_model_case(name)], kernel == "coop", adam_seed=3, steps=7, over=over)
    before = call.snapshot()
    call.launch(mode, wgs)
    assert call.rc == R.BAD_ARG
    assert call.written[0] == [] and call.changed(before) == [[]] and call.status == 0
    if kernel == "coop":
        assert not call.sync.any()
