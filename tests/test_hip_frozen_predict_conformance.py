"""mobocmf_frozen_predict and mobocmf_frozen_predict_split (csrc/frozen_predict.hip) through the C ABI, componentwise against the
longdouble restatement ON THE CHAIN STATE THE KERNEL READS (tests/frozen_predict_reference.py: the gate and where its
constants come from; tests/test_frozen_predict_reference_cpu.py: the proof on the CPU).

The chains come from mobocmf_layers_chain_forward (branch = 1) into NaN-prefilled blocks and are read back: the kernels read
pad rows and columns M .. Mr-1 of them, so a pad word the chain forward leaves unwritten shows as a NaN moment.  The cases are
the smallest on each side of a switch in the kernel -- sizes the predict groups (128 < M, one M per group) never run."""
import numpy as np
import pytest

from tests import frozen_predict_reference as F
from tests import kernel_reference as R

pytestmark = pytest.mark.gpu

# what each case is named for, restated from the kernel's geometry (frozen_geometry)
PANEL_SIDES = {
    "M1_L1_d1_T1": dict(rows=16, wgs=1, last_rows=1, tiles=1, rounds=1, blocks=1, dead=15),
    "M16_L2_d8_S2_T9": dict(rows=8, wgs=2, last_rows=1, tiles=1, blocks=1, dead=0),
    "M17_L2_d3_S3_T6": dict(rows=5, wgs=2, tiles=2, blocks=1, dead=1),
    "M200_L1_d4_T33": dict(rows=16, wgs=3, last_rows=1, tiles=13, rounds=2),
    "M129_L2_d2_S5_T7_uniform": dict(tiles=9, rounds=2, last_round=1, rows=3),
    "M130_L3_d2_S17_T3": dict(rows=1, wgs=3, blocks=2, dead=15, tiles=9),
    "M257_L2_d8_S16_T2": dict(rows=1, tiles=17, rounds=3, last_round=1, blocks=1, dead=0),
    "M512_L2_d8_S48_T2": dict(rows=1, blocks=3, dead=0, tiles=32, rounds=4, lds=2 * 64 * 1024 + 512 * 8),
    "floor_M130_L1_d8_T3": dict(rows=16, wgs=1, tiles=9),
}
SPLIT_SIDES = {
    "M16_L1_d2_T9": dict(rows=8, parts=1, wgs=2),
    "M65_L3_d8_S8_T2": dict(rows=1, parts=1, last_part=8, wgs=2),
    "M129_L2_d2_S11_T3_uniform": dict(parts=2, last_part=3, wgs=6, tiles=9),
    "M1024_L2_d8_S9_T2": dict(parts=2, last_part=1, wgs=4, tiles=64, lds=136 * 1024),
    "floor_M130_L1_d8_T3": dict(rows=8, parts=1, wgs=1),
    "floor_M130_L2_d8_S9_T3": dict(parts=2, last_part=1, wgs=6),
}
_bits = lambda a: np.ascontiguousarray(a).view(np.int64)


def test_the_cases_sit_on_the_sides_they_are_named_for():
    for sides, cases, split in ((PANEL_SIDES, F.FROZEN_PANEL_CASES, False), (SPLIT_SIDES, F.FROZEN_SPLIT_CASES, True)):
        assert set(sides) == set(cases)
        for name, side in sides.items():
            g = F.frozen_geometry(F.frozen_case(cases[name]), split)
            assert {k: g[k] for k in side} == side, (name, g)
    g = [F.frozen_geometry(mc, False) for mc in F.frozen_group_cases()]
    assert len({(x["tiles"], x["rows"]) for x in g}) == 3 and max(x["tiles"] for x in g) == g[2]["tiles"]      # LDS is sized by the last


def _chains_are_sound(call):
    """On the host, before anything is launched on them: L^-T and U^T are the transposes of L^-1 and U bit for bit, L^-1 and U
    lower triangular."""
    for chains in call.chains:
        for c in chains:
            assert np.array_equal(_bits(c["LinvT"]), _bits(c["Linv"].T)) and np.array_equal(_bits(c["UT"]), _bits(c["U"].T))
            assert not np.triu(c["Linv"], 1).any() and not np.triu(c["U"], 1).any()
            assert np.isfinite(c["Linv"]).all() and np.isfinite(c["U"]).all() and np.isfinite(c["a"]).all()


def _gate(call, i, what, label):
    mc, chains = call.mcs[i], call.chains[i]
    names = F.FROZEN_NAMES[what]
    bad, worst, report = F.frozen_gate(call.res[i], F.frozen_predict_ref(mc, chains), F.frozen_predict_ref(mc, chains, shadow=True), names)
    print("%s%s %s: %s" % (label, " model %d (M = %d)" % (i, mc["M"]) if call.n > 1 else "", what, report))
    assert bad == [], (label, what, bad, report)


def _conformance(mcs, split, label):
    """FORWARD: the moments inside the gate, nothing else written.  Everything poisoned; INPUT_GRADIENTS: the same moments
    bit for bit, g_x inside the gate, exact zeros on the rows without seeds.  Poisoned again: every bit repeats.  The guards
    behind every output and behind `work` are still NaN."""
    call = F.FrozenLaunch(mcs, split)
    _chains_are_sound(call)
    call.run(F.FORWARD)
    assert call.rc == 0 and all(call.guards) and all(call.grad_untouched)
    for i in range(call.n):
        _gate(call, i, "forward", label)
    fwd = [dict(r) for r in call.res]
    call.run(F.INPUT_GRADIENTS)
    assert call.rc == 0 and all(call.guards)
    first = [dict(r) for r in call.res]
    for i, mc in enumerate(call.mcs):
        assert all(np.array_equal(_bits(fwd[i][k]), _bits(first[i][k])) for k in F.FROZEN_NAMES["forward"]), label
        _gate(call, i, "input", label)
        off = np.arange(mc["rows"][0]) % 3 == 1
        assert (first[i]["g_x"][off] == 0).all() and first[i]["g_x"][~off].any(axis=1).all(), label
    call.run(F.INPUT_GRADIENTS)
    assert call.rc == 0 and all(call.guards)
    for a, b in zip(first, call.res):
        assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in F.FROZEN_NAMES["input"]), label
    return call, first


@pytest.mark.parametrize("name", list(F.FROZEN_PANEL_CASES))
def test_panel_form_on_the_given_chain(name):
    mc = F.frozen_case(F.FROZEN_PANEL_CASES[name])
    call, res = _conformance([mc], False, "panel %s" % name)
    if name.startswith("floor"):
        assert F.floored_columns(mc, call.chains[0])[0].tolist() == [mc["rows"][0] - 1] and res[0]["top_var"][-1] == 1e-10


@pytest.mark.parametrize("name", list(F.FROZEN_SPLIT_CASES))
def test_split_form_on_the_given_chain(name):
    mc = F.frozen_case(F.FROZEN_SPLIT_CASES[name])
    call, _ = _conformance([mc], True, "split %s" % name)
    if name.startswith("floor"):
        assert F.floored_columns(mc, call.chains[0])[0].tolist() == [mc["rows"][0] - 1]
        assert mc["L"] > 1 or call.res[0]["top_var"][-1] == 1e-10


@pytest.mark.parametrize("split", [False, True], ids=["panel", "split"])
def test_models_of_different_size_in_one_launch(split):
    """(M, L, S) = (17, 2, 3), (129, 1, -), (257, 3, 2) at d = 2, T = 6 in one call: the LDS is sized by the largest M while
    each workgroup offsets its panels by its own Mr.  Every model passes its gate and equals its own single-model launch bit
    for bit (the chain forward is deterministic: the single launch forms the same chain again)."""
    mcs = F.frozen_group_cases()
    _, together = _conformance(mcs, split, "group (%s)" % ("split" if split else "panel"))
    for i, mc in enumerate(mcs):
        alone = F.FrozenLaunch([mc], split).run(F.INPUT_GRADIENTS)
        assert alone.rc == 0 and all(alone.guards)
        assert all(np.array_equal(_bits(together[i][k]), _bits(alone.res[0][k])) for k in F.FROZEN_NAMES["input"]), (i, mc["M"])
