"""chain_backward of csrc/api.hip forms dK_mm = sym(L^-T Wn L^-1) directly (backward) -- against the longdouble
reference of tests/kernel_reference.py, which states the Cholesky backward (Phi(L^T dL)) and so derives the same gradient
another way.  The gate is the layer bound with its own constants: |got - ref| <= LAYER_C[group] u S, exact zeros where S = 0.
Here: z-batched chains whose clamped columns make Hc differ from H, at the sizes and tunings that take the M x M products
through the small-operand, the mid-size and the tiled family; layers that only differentiate the KL next to layers with a
panel; the eval branch, where Hc IS H; and the chain backward twice over the same chain block."""
import numpy as np
import pytest
import torch

from tests import kernel_reference as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason="numpy.longdouble is no wider than float64 here")]

# (kind 0, kind 1) of equal M with clamped columns (keys of R.LAYER_CASES: tests/test_layer_reference_cpu.py proves the
# conditioning and the margins on them).  Mp = 256: the small-operand kernel, or -- R.TILED -- the tiled family; Mp = 384:
# the mid-size kernel (four wavefronts per workgroup by default, eight under mid_gemm_waves = 8), or the tiled family.
CLAMPED_PAIRS = {129: ((0, 2, 129, 12, 1, 0, 4, False, 0, 0), (1, 2, 129, 4, 3, 0, 2, False, 0, 0)),
                 257: ((0, 9, 257, 300, 1, 0, 20, False, 0, 0), (1, 9, 257, 100, 3, 0, 10, False, 0, 0))}
KL_PAIRS = {8: ((0, 2, 8, 12, 1, 0, 0, False, 0, 1), (1, 2, 8, 4, 3, 0, 0, False, 0, 1)),
            129: ((0, 2, 129, 300, 1, 0, 0, False, 0, 1), (1, 2, 129, 300, 1, 0, 0, False, 0, 1))}
EVAL_CASES = [(0, 9, 127, 12, 1, 0, 0, False, 1, 0), (1, 9, 127, 12, 1, 0, 0, False, 1, 0),
              (0, 2, 257, 129, 1, 0, 0, True, 1, 1), (1, 2, 257, 129, 1, 0, 0, True, 1, 1)]
TUNINGS = [{}, R.TILED, dict(mid_gemm_waves=8)]
GRADS = ("g_m", "g_LS", "g_hyp", "g_zf")


def _tid(t):
    return "_".join("%s%d" % kv for kv in t.items()) or "default"


def _id(k):
    return "k%d_d%d_M%d_nb%d_x%d_s%d_c%d_f%d_b%d_dx%d" % tuple(int(v) for v in k)


def _gate(got, names, what, ref, S):
    bad, worst, report = R.layer_gate(got, ref, S, names)
    print("%s: %s" % (what, report))
    assert not bad, "%s: (output, worst err / (u S), non-zeros where S = 0) %r against C_g %r" % (what, bad, R.LAYER_C)


def _clean(r, what):
    assert r.rc == 0, (what, r.rc)
    assert r.untouched, what + ": a guard double behind an output was written"


def _chain_and_panels(cs, panel, tuning=None):
    """The z-batched chain forward of ``cs`` and, for the layers with panel[z], the PANEL forward and backward (which leave H,
    Hc and da in the layer's chain block).  Returns the chain call and the panel backward's LayerCall per layer (or None)."""
    ch = R.chain_forward_direct(cs, R.make_tuning(**tuning) if tuning else None)
    assert ch.rc == 0 and ch.info == [0] * len(cs) and ch.untouched
    shares = [None] * len(cs)
    for z, c in enumerate(cs):
        if panel[z]:
            pf = R.panel_forward_direct(ch, z, c)
            _clean(pf, "panel forward %d" % z)
            shares[z] = R.panel_backward_direct(pf)
            _clean(shares[z], "panel backward %d" % z)
    return ch, shares


@pytest.mark.parametrize("tuning", TUNINGS, ids=_tid)
@pytest.mark.parametrize("mode", (1, 2, 6), ids=("shares_apart", "accumulated", "zf_folded_into_g_m"))
@pytest.mark.parametrize("M", sorted(CLAMPED_PAIRS))
def test_two_clamped_layers_in_one_chain(M, mode, tuning):
    """had_panel = 1 (the two shares of g_hyp / g_zf in buffers of their own, added here), 2 (accumulated by the chain
    backward), 2 | 4 (the whole g_zf of layer 1 added to g_m of layer 0)."""
    cs = [R.layer_case(*k) for k in CLAMPED_PAIRS[M]]
    for c in cs:
        ref = R.layer_ref(c)
        assert (ref["knn"] - ref["q"] <= 0).any() and (ref["knn"] - ref["q"] > 0).any(), "the case does not make Hc differ from H"
    ch, shares = _chain_and_panels(cs, [True, True], tuning)
    had = [mode if (z or mode != 6) else 2 for z in range(2)]
    panel = [{k: v.copy() for k, v in s.out.items()} for s in shares]
    outs = R.chain_backward_direct(ch, [c["g_kl"] for c in cs], had, shares if mode >= 2 else None)
    for z, (c, o) in enumerate(zip(cs, outs)):
        _clean(o, "chain backward %d" % z)
        got = dict(o.out)
        ref, S = dict(R.layer_ref(c)), dict(R.layer_ref(c, shadow=True))
        names = [n for n in GRADS if n in got and not (n == "g_zf" and mode == 6)]
        if mode == 1:
            got["g_hyp"] = got["g_hyp"] + panel[z]["g_hyp"]
            if c["kind"] == 1:
                got["g_zf"] = got["g_zf"] + panel[z]["g_zf"]
        if mode == 6:
            if z == 1:
                assert np.array_equal(o.out["g_zf"], panel[z]["g_zf"])      # g_zf is not written: it still holds the PANEL share
            else:                                                          # g_m[0] also carries the whole g_zf of layer 1
                ref["g_m"] = ref["g_m"] + R.layer_ref(cs[1])["g_zf"]
                S["g_m"] = S["g_m"] + R.layer_ref(cs[1], shadow=True)["g_zf"]
        _gate(got, names, "M %d layer %d had_panel %d %s" % (M, z, had[z], _tid(tuning)), ref, S)


@pytest.mark.parametrize("g_kl", (1.0, 1e-4))
@pytest.mark.parametrize("zero_layer", (1, 0), ids=("kind1_kl_only", "kind0_kl_only"))
@pytest.mark.parametrize("M", sorted(KL_PAIRS))
def test_kl_only_layer_beside_a_layer_with_a_panel(M, zero_layer, g_kl):
    """had_panel = 0 for one layer of the batch (H, Hc, da cleared: only the KL is differentiated), 1 for the other."""
    base = [R.layer_case(*k) for k in KL_PAIRS[M]]
    cs = [R.with_upstream(c, None, None, g_kl, tag="kl_only_%g" % g_kl) if z == zero_layer else
          R.with_upstream(c, c["g_mean"], c["g_var"], g_kl, tag="g_kl_%g" % g_kl) for z, c in enumerate(base)]
    ch, shares = _chain_and_panels(cs, [z != zero_layer for z in range(2)])
    outs = R.chain_backward_direct(ch, [g_kl, g_kl], [0 if z == zero_layer else 1 for z in range(2)])
    for z, (c, o) in enumerate(zip(cs, outs)):
        _clean(o, "chain backward %d" % z)
        got = dict(o.out)
        if z != zero_layer:
            got["g_hyp"] = got["g_hyp"] + shares[z].out["g_hyp"]
            if c["kind"] == 1:
                got["g_zf"] = got["g_zf"] + shares[z].out["g_zf"]
        _gate(got, [n for n in GRADS if n in got], "M %d layer %d %s g_kl %g" % (M, z, "KL only" if z == zero_layer else "with panel", g_kl),
              R.layer_ref(c), R.layer_ref(c, shadow=True))


@pytest.mark.parametrize("key", EVAL_CASES, ids=_id)
def test_eval_branch_where_hc_is_h(key):
    """branch = 1 through mobocmf_layer_backward: one layer, no clamp -- the chain backward reads H where it reads Hc."""
    c = R.layer_case(*key)
    fw = R.layer_forward_direct(c)
    _clean(fw, "forward")
    assert fw.info == 0
    bw = R.layer_backward_direct(fw)
    _clean(bw, "backward")
    _gate(dict(fw.out, **bw.out), R.layer_names(c), _id(key), R.layer_ref(c), R.layer_ref(c, shadow=True))


@pytest.mark.parametrize("M", sorted(CLAMPED_PAIRS))
def test_twice_over_one_chain_block_is_bitwise_equal(M):
    """The chain backward reads H, Hc and da of the chain block and the chain state, and modifies none of them: a second call over the
    same block and the same panel shares returns the same bits."""
    cs = [R.layer_case(*k) for k in CLAMPED_PAIRS[M]]
    ch, _ = _chain_and_panels(cs, [True, True])
    state = [R.chain_block(ch, z, state_only=True).clone() for z in range(2)]
    first = R.chain_backward_direct(ch, [c["g_kl"] for c in cs], [1, 1])
    second = R.chain_backward_direct(ch, [c["g_kl"] for c in cs], [1, 1])
    for z, (a, b) in enumerate(zip(first, second)):
        _clean(a, "first call, layer %d" % z)
        _clean(b, "second call, layer %d" % z)
        assert set(a.out) == set(b.out) and len(a.out) == (4 if cs[z]["kind"] == 1 else 3)
        for k in a.out:
            assert np.isfinite(a.out[k]).all(), (z, k)
            assert a.out[k].tobytes() == b.out[k].tobytes(), (z, k)
        assert torch.equal(R.chain_block(ch, z, state_only=True), state[z]), z
