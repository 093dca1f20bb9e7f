"""mobocmf_rff_eval, mobocmf_rff_eval_chains (csrc/rff.hip), mobocmf_rff_chains_value_grad and mobocmf_rff_refine (csrc/rff_opt.hip)
through the C ABI, componentwise against the longdouble restatement ON THE GIVEN DRAWS (tests/rff_reference.py: the gate and
where its constants come from; tests/test_rff_reference_cpu.py: the proof on the CPU).

The cases are the smallest on each side of a switch in the kernels -- feature counts around an LDS chunk, a wavefront and the
eight or four wavefronts of a refinement; point counts around a workgroup; every DB instantiation from both ends; chains of
different depth and F in one launch -- and every launch is repeated (the same bits) into NaN-prefilled outputs with guard
words behind them."""
import numpy as np
import pytest

from tests import rff_reference as F

pytestmark = pytest.mark.gpu

# what each case is named for, restated from the kernels' geometry (rff_geometry)
EVAL_SIDES = {
    "d1_F1_n1_L1": dict(DB=2, dead=1, chunks=[[1]], last_chunk=[[1]], wgs=1, last_rows=1),
    "d2_F63_n255_L2": dict(DB=2, dead=0, chunks=[[1, 1]], last_chunk=[[63, 63]], wgs=1, last_rows=255),
    "d3_F64_n256_L3": dict(DB=8, dead=5, chunks=[[1, 1, 1]], last_chunk=[[64] * 3], wgs=1, last_rows=256),
    "d8_F65_n257_L2": dict(DB=8, dead=0, chunks=[[2, 2]], last_chunk=[[1, 1]], wgs=2, last_rows=1),
    "d9_F129_n257_L1": dict(DB=32, dead=23, chunks=[[3]], last_chunk=[[1]], wgs=2, last_rows=1),
    "d32_F64_n1_L3": dict(DB=32, dead=0, chunks=[[1, 1, 1]], wgs=1, last_rows=1),
    "d32_F65_n256_L2": dict(DB=32, dead=0, chunks=[[2, 2]], last_chunk=[[1, 1]], wgs=1, last_rows=256),
    "d2_F129_n257_L3": dict(DB=2, chunks=[[3, 3, 3]], last_chunk=[[1, 1, 1]], wgs=2, last_rows=1),
    "mixed_d3_K3_n257": dict(DB=8, chunks=[[2], [1, 1, 3], [1, 2]], last_chunk=[[1], [64, 1, 1], [63, 1]], wgs=2, last_rows=1),
    "short_d2_F65_n257_L2": dict(DB=2, chunks=[[2, 2]], wgs=2),
    "cancel_d3_F65_n5_L1": dict(DB=8, chunks=[[2]], last_chunk=[[1]], wgs=1, last_rows=5),
}
VG_SIDES = {
    "d1_F1_n1_L1": dict(DB=2, dead=1, vg_wgs=1, vg_last_points=1, vg_idle_lanes=[[63]]),
    "d2_F1_n5_L2": dict(DB=2, dead=0, vg_wgs=2, vg_last_points=1, vg_idle_lanes=[[63, 63]]),
    "d2_F63_n3_L2": dict(DB=2, dead=0, vg_wgs=1, vg_last_points=3, vg_idle_lanes=[[1, 1]]),
    "d3_F64_n4_L2": dict(DB=8, dead=5, vg_wgs=1, vg_last_points=4, vg_idle_lanes=[[0, 0]]),
    "d8_F65_n5_L2": dict(DB=8, dead=0, vg_wgs=2, vg_last_points=1, vg_idle_lanes=[[0, 0]]),
    "d9_F65_n5_L3": dict(DB=32, dead=23, vg_wgs=2, vg_last_points=1, vg_idle_lanes=[[0, 0, 0]]),
    "d32_F63_n3_L2": dict(DB=32, dead=0, vg_wgs=1, vg_last_points=3, vg_idle_lanes=[[1, 1]]),
    "mixed_d3_K3_n5": dict(DB=8, vg_wgs=2, vg_last_points=1, vg_idle_lanes=[[0], [0, 63, 0], [1, 0]]),
    "short_d2_F65_n5_L2": dict(DB=2, vg_wgs=2),
    "cancel_d3_F65_n5_L1": dict(DB=8, vg_wgs=2, vg_last_points=1),
}
REFINE_SIDES = {
    "d1_F1_L1_C0": dict(DB=2, dead=1, NW=8, per_thread=[[1]], idle_waves=[[7]]),
    "d2_F511_L1_C1": dict(DB=2, dead=0, NW=8, per_thread=[[1], [1]], idle_waves=[[0], [0]]),
    "d8_F512_L3_C2": dict(DB=8, dead=0, NW=8, per_thread=[[1, 1, 1]] * 3, idle_waves=[[0, 0, 0]] * 3),
    "d3_F513_L3_C32": dict(DB=8, dead=5, NW=8, per_thread=[[2, 1, 2], [1, 2], [2]], idle_waves=[[0, 7, 0], [6, 0], [0]]),
    "d9_F255_L1_C1": dict(DB=32, dead=23, NW=4, per_thread=[[1], [1]], idle_waves=[[0], [0]]),
    "d32_F256_L3_C2": dict(DB=32, dead=0, NW=4, per_thread=[[1, 1, 1]] * 3, idle_waves=[[0, 0, 0]] * 3),
    "d9_F257_L3_C32": dict(DB=32, dead=23, NW=4, per_thread=[[2, 2, 2], [2], [1, 2]], idle_waves=[[0, 0, 0], [0], [3, 0]]),
    "d8_F512_L1_C0_clamped": dict(DB=8, NW=8, per_thread=[[1]], idle_waves=[[0]]),
}
_bits = lambda a: np.ascontiguousarray(a).view(np.int64)
_same = lambda a, b, names: all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in names)


def test_the_cases_sit_on_the_sides_they_are_named_for():
    for sides, cases, get in ((EVAL_SIDES, F.EVAL_CASES, F.eval_case), (VG_SIDES, F.VG_CASES, F.vg_case),
                              (REFINE_SIDES, F.REFINE_CASES, F.refine_case)):
        assert set(sides) == set(cases)
        for name, side in sides.items():
            g = F.rff_geometry(get(name))
            assert {k: g[k] for k in side} == side, (name, g)
    assert sorted(kw["C"] for kw in F.REFINE_CASES.values()) == [0, 0, 1, 1, 2, 2, F.MAX_CON, F.MAX_CON]
    assert {c[0] for c in F.EVAL1_CASES.values()} <= set(F.EVAL_CASES)
    assert sorted(F.eval_case(c)["chains"][k][l] for c, k, l in F.EVAL1_CASES.values()) == [1, 63, 64, 65, 129]


def _gated(label, got, ref, S, names):
    bad, worst, report = F.rff_gate(got, ref, S, names)
    print("%s: %s" % (label, report))
    assert bad == [], (label, bad, report)


@pytest.mark.parametrize("name", list(F.EVAL_CASES))
def test_eval_chains_on_the_given_draws(name):
    """One launch of every chain of the case inside the 'value' gate; the repeat and every chain's own launch give the same bits."""
    c = F.eval_case(name)
    call = F.RffLaunch(c)
    first = call.eval_chains()
    assert first["rc"] == 0 and first["guards"]
    _gated("eval_chains " + name, first, F.rff_chain_ref(c), F.rff_chain_ref(c, shadow=True), ("value",))
    again = call.eval_chains()
    assert again["rc"] == 0 and again["guards"] and _same(first, again, ("value",))
    if c["K"] > 1:
        for k in range(c["K"]):
            one = F.RffLaunch(c, [k]).eval_chains()
            assert one["rc"] == 0 and one["guards"] and np.array_equal(_bits(one["value"][0]), _bits(first["value"][k])), (name, k)


@pytest.mark.parametrize("name", list(F.EVAL1_CASES))
def test_eval_kind_1_on_a_given_fprev(name):
    c, k, l, fp = F.eval1_case(name)
    call = F.RffLaunch(c)
    first = call.eval_layer1(k, l, fp)
    assert first["rc"] == 0 and first["guards"]
    _gated("rff_eval kind 1 " + name, first, F.rff_layer1_ref(c, k, l, fp), F.rff_layer1_ref(c, k, l, fp, shadow=True), ("value",))
    again = call.eval_layer1(k, l, fp)
    assert again["rc"] == 0 and again["guards"] and _same(first, again, ("value",))


@pytest.mark.parametrize("name", list(F.VG_CASES))
def test_value_grad_on_the_given_draws(name):
    """Values and gradients inside their gates against the longdouble statement (not against another kernel); the repeat and
    every chain's own launch give the same bits."""
    c = F.vg_case(name)
    call = F.RffLaunch(c)
    first = call.value_grad()
    assert first["rc"] == 0 and first["guards"]
    _gated("value_grad " + name, first, F.rff_chain_ref(c), F.rff_chain_ref(c, shadow=True), F.RFF_GROUPS)
    again = call.value_grad()
    assert again["rc"] == 0 and again["guards"] and _same(first, again, F.RFF_GROUPS)
    if c["K"] > 1:
        for k in range(c["K"]):
            one = F.RffLaunch(c, [k]).value_grad()
            assert one["rc"] == 0 and one["guards"], (name, k)
            assert all(np.array_equal(_bits(one[g][0]), _bits(first[g][k])) for g in F.RFF_GROUPS), (name, k)


@pytest.mark.parametrize("name", list(F.REFINE_CASES))
def test_refine_one_step_on_the_given_draws(name):
    """outer = inner = 1, backtracks = restore = 0: xs inside the model's bound (exactly 0.0 on the clamped component), fs and
    slack_min inside the 'value' gate of the reference at the written xs, NaN fs where no point is feasible; the repeat and
    every start's own launch give the same bits."""
    c = F.refine_case(name)
    call = F.RffLaunch(c)
    first = call.refine_step()
    assert first["rc"] == 0 and first["guards"]
    bad, worst, report = F.rff_refine_gate(c, first)
    print("refine step %s: %s" % (name, report))
    assert bad == [], (name, bad, report)
    model = F.rff_refine_step_ref(c)
    for p, m in enumerate(model):
        assert np.isnan(first["fs"][p]).all() != m["feasible"] and np.isfinite(first["xs"][p]).all()
        assert first["status"][p] == (0 if m["feasible"] else 2) and first["start_best"][p] == (np.argmin(first["fs"][p]) if m["feasible"] else -1)
    if c.get("clamped"):
        p, r, k = c["clamped"]
        assert first["xs"][p, r, k] == 0.0 and not np.signbit(first["xs"][p, r, k])
    names = ("xs", "fs", "slack_min", "x_best", "f_best")
    again = call.refine_step()
    assert again["rc"] == 0 and again["guards"] and _same(first, again, names)
    for p in range(c["P"]):
        for r in range(c["R"]):
            one = call.refine_step(only=(p, r))
            assert one["rc"] == 0 and one["guards"], (name, p, r)
            assert all(np.array_equal(_bits(one[k][0, 0]), _bits(first[k][p, r])) for k in ("xs", "fs", "slack_min")), (name, p, r)
