"""The variational layer -- chain_forward / panel_forward / panel_backward / chain_backward of csrc/api.hip with the kernels
of elementwise.hip that join the products, the Gram kernels and the factorisation chain -- against the longdouble reference
of tests/kernel_reference.py, componentwise: |got - ref| <= C_g u S with the magnitude shadow S, exact zeros where S = 0
("The layer bound").  tests/test_layer_reference_cpu.py proves the conditions on these inputs and the constants.
Every call goes through the C ABI directly: NaN-filled outputs and workspaces, guard doubles behind every output, info = 0."""
import numpy as np
import pytest
import torch

from tests import kernel_reference as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason="numpy.longdouble is no wider than float64 here")]

GRADS = ("g_m", "g_LS", "g_hyp", "g_x", "g_f", "g_zf")


def _id(k):
    return "k%d_d%d_M%d_nb%d_x%d_s%d_c%d_f%d_b%d_dx%d" % tuple(int(v) for v in k)


def _gate(c, got, names, what, ref=None, S=None):
    ref = R.layer_ref(c) if ref is None else ref
    S = R.layer_ref(c, shadow=True) if S is None else S
    bad, worst, report = R.layer_gate(got, ref, S, names)
    print("%s: %s" % (what, report))
    assert not bad, "%s: (output, worst err / (u S), non-zeros where S = 0) %r against C_g %r" % (what, bad, R.LAYER_C)
    return worst


def _clean(r, what):
    assert r.rc == 0, (what, r.rc)
    assert r.untouched, what + ": a guard double behind an output was written"


def _whole(c, tune=None, up=None):
    fw = R.layer_forward_direct(c, tune)
    _clean(fw, "forward")
    assert fw.info == 0
    bw = R.layer_backward_direct(fw, up)
    _clean(bw, "backward")
    return fw, bw


def _all_nan(t):
    return bool(torch.isnan(t.view(torch.float64)).all())


@pytest.mark.parametrize("key", R.LAYER_CASES, ids=_id)
def test_whole_call_is_within_the_layer_bound(key):
    c = R.layer_case(*key)
    fw, bw = _whole(c)
    _gate(c, dict(fw.out, **bw.out), R.layer_names(c), _id(key))


@pytest.mark.parametrize("key", R.LAYER_UPSTREAM_CASES, ids=_id)
def test_each_upstream_gradient_alone(key):
    """One backward each over one forward for g_mean alone, g_var alone, g_kl alone, all three, and all three with g_kl = 1e-4
    (the absent ones as exact zeros: the entry points take no NULL): moments_bwd_prep and the chain backward see each share
    by itself, and a KL share three orders below the others is still held componentwise."""
    c = R.layer_case(*key)
    fw = R.layer_forward_direct(c)
    _clean(fw, "forward")
    names = [n for n in R.layer_names(c) if n in GRADS]
    ups = {"mean": R.with_upstream(c, c["g_mean"], None, 0.0, tag="mean"), "var": R.with_upstream(c, None, c["g_var"], 0.0, tag="var"),
           "kl": R.with_upstream(c, None, None, c["g_kl"], tag="kl"), "all": c,
           "kl_small": R.with_upstream(c, c["g_mean"], c["g_var"], 1e-4, tag="kl_small")}
    for tag, cu in ups.items():
        bw = R.layer_backward_direct(fw, cu)
        _clean(bw, tag)
        _gate(cu, bw.out, names, "%s upstream %s" % (_id(key), tag))


@pytest.mark.parametrize("sparse", (1, 0))
@pytest.mark.parametrize("pattern", sorted(R.LAYER_ACTIVITY))
@pytest.mark.parametrize("key", R.LAYER_ACTIVITY_CASES, ids=_id)
def test_inactive_column_blocks(key, pattern, sparse):
    """N' = 640 with whole 128-blocks of exactly zero upstream gradients, skipped (sparse_backward = 1) or multiplied through
    (0): both within the gate, and the outputs of the inactive columns exactly zero."""
    c, mask = R.activity_case(R.layer_case(*key), pattern)
    fw, bw = _whole(c, R.make_tuning(sparse_backward=sparse))
    names = [n for n in R.layer_names(c) if n in GRADS]
    _gate(c, bw.out, names, "%s %s sparse_backward=%d" % (_id(key), pattern, sparse))
    rows = mask.reshape(c["nbase"], c["xdiv"]).any(1)
    assert not bw.out["g_x"][~rows].any()
    if c["kind"] == 1:
        assert not bw.out["g_f"][~mask].any()


TUNINGS = [dict(potrf_cols=0), dict(potrf_cols=1), dict(potrf_cols=4), R.TILED, dict(mid_gemm_waves=4), dict(mid_gemm_waves=8),
           dict(tile_rows=64), dict(tile_rows=128), dict(pair_mode=1), dict(pair_mode=2)]


@pytest.mark.parametrize("tuning", TUNINGS, ids=lambda t: "_".join("%s%d" % kv for kv in t.items()))
@pytest.mark.parametrize("key", R.LAYER_TUNING_CASES, ids=_id)
def test_tunings_stay_within_the_layer_bound(key, tuning):
    """M = 257 and 400 under every factorisation form, product family, tile height and pairing the layer can be given, the
    sizes queried with the same tuning."""
    c = R.layer_case(*key)
    fw, bw = _whole(c, R.make_tuning(**tuning))
    _gate(c, dict(fw.out, **bw.out), R.layer_names(c), "%s %r" % (_id(key), tuning))


@pytest.mark.parametrize("mode", (0, 1, 2, 6), ids=("kl_only", "shares_apart", "accumulated", "zf_folded_into_g_m"))
def test_split_calls_three_layers(mode):
    """Three layers of M = 129 (kind 0, 1, 1) through one z-batched chain forward, a PANEL call per layer and one chain
    backward; had_panel = 0 (only the KL differentiated), 1 (the two shares of g_hyp / g_zf in buffers of their own, added here),
    2 (accumulated by the chain backward), 2 | 4 (the whole g_zf of layers 1 and 2 added to g_m of the layer below)."""
    cs = [R.layer_case(*k) for k in R.LAYER_SPLIT_CASES]
    if mode == 0:
        cs = [R.with_upstream(c, None, None, c["g_kl"], tag="kl") for c in cs]
    ch = R.chain_forward_direct(cs)
    assert ch.rc == 0 and ch.info == [0, 0, 0] and ch.untouched
    shares = [None] * 3
    for z, c in enumerate(cs):
        _gate(c, {"kl": ch.kl[z]}, ("kl",), "layer %d chain forward" % z)
        if mode:
            pf = R.panel_forward_direct(ch, z, c)
            _clean(pf, "panel forward")
            _gate(c, pf.out, ("mean", "var"), "layer %d panel forward" % z)
            shares[z] = R.panel_backward_direct(pf)
            _clean(shares[z], "panel backward")
            _gate(c, shares[z].out, [n for n in ("g_x", "g_f") if n in shares[z].out], "layer %d panel backward" % z)
    had = [mode if (z or mode != 6) else 2 for z in range(3)]
    panel = [None if s is None else {k: v.copy() for k, v in s.out.items()} for s in shares]
    outs = R.chain_backward_direct(ch, [c["g_kl"] for c in cs], had, shares if mode >= 2 else None)
    for z, (c, o) in enumerate(zip(cs, outs)):
        assert o.rc == 0 and o.untouched, z
        got = dict(o.out)
        ref, S = dict(R.layer_ref(c)), dict(R.layer_ref(c, shadow=True))
        names = ["g_LS", "g_hyp", "g_m"] + (["g_zf"] if c["kind"] == 1 and mode != 6 else [])
        if mode == 1:
            got["g_hyp"] = got["g_hyp"] + panel[z]["g_hyp"]
            if c["kind"] == 1:
                got["g_zf"] = got["g_zf"] + panel[z]["g_zf"]
        if mode == 6:
            if z >= 1:
                assert np.array_equal(o.out["g_zf"], panel[z]["g_zf"])      # g_zf is not written: it still holds the PANEL share
            if z + 1 < 3:                                        # g_m[z] also carries the whole g_zf of the layer above
                up = cs[z + 1]
                ref["g_m"] = ref["g_m"] + R.layer_ref(up)["g_zf"]
                S["g_m"] = S["g_m"] + R.layer_ref(up, shadow=True)["g_zf"]
        _gate(c, got, names, "layer %d chain backward, had_panel %d" % (z, had[z]), ref=ref, S=S)


def test_split_calls_one_small_layer():
    c = R.layer_case(*R.LAYER_SPLIT_ONE)
    ch = R.chain_forward_direct([c])
    assert ch.rc == 0 and ch.info == [0] and ch.untouched
    pf = R.panel_forward_direct(ch, 0, c)
    _clean(pf, "panel forward")
    pb = R.panel_backward_direct(pf)
    _clean(pb, "panel backward")
    o = R.chain_backward_direct(ch, [c["g_kl"]], [2], [pb])[0]
    _clean(o, "chain backward")
    _gate(c, dict(pf.out, kl=ch.kl[0], g_x=pb.out["g_x"], g_f=pb.out["g_f"], **o.out), R.layer_names(c), "n = 1, M = 8")


@pytest.mark.parametrize("key", R.LAYER_SPLIT_CASES[:2], ids=_id)
def test_constant_parameters_on_the_state_alone(key):
    """params_const = 1: the PANEL calls get the chain STATE alone (a copy of its bytes, nothing behind it), yield g_f / g_x
    within the gate and leave those bytes as they were; the whole-call entry points refuse the flag."""
    c = R.layer_case(*key)
    ch = R.chain_forward_direct([c])
    assert ch.rc == 0 and ch.info == [0]
    state = R.chain_block(ch, 0, state_only=True).clone()
    before = state.clone()
    pf = R.panel_forward_direct(ch, 0, c, params_const=1, block=state)
    _clean(pf, "panel forward")
    pb = R.panel_backward_direct(pf)
    _clean(pb, "panel backward")
    assert torch.equal(state, before)
    _gate(c, dict(pf.out, **pb.out), ["mean", "var", "g_x"] + (["g_f"] if c["kind"] == 1 else []), _id(key) + " params_const")
    fw = R.layer_forward_direct(c, desc=R.layer_desc(c, params_const=1))
    assert fw.rc == R.BAD_ARG and all(np.isnan(v).all() for v in fw.out.values()) and _all_nan(fw.saved)
    fw = R.layer_forward_direct(c)
    fw.desc.params_const = 1
    bw = R.layer_backward_direct(fw)
    assert bw.rc == R.BAD_ARG and all(np.isnan(v).all() for v in bw.out.values())


def test_refused_arguments_write_nothing():
    c = R.layer_case(*R.LAYER_CASES[17])                        # kind 1, M = 8, N' = 12, xdiv = 3
    good = R.layer_desc(c)
    for what, over in (("Np % xdiv != 0", dict(Np=13)), ("d = 0", dict(d=0)), ("d = 33", dict(d=33))):
        fw = R.layer_forward_direct(c, desc=R.layer_desc(c, **over), size_desc=good)
        assert fw.size_rc == R.BAD_ARG and fw.rc == R.BAD_ARG, what
        assert all(np.isnan(v).all() for v in fw.out.values()) and _all_nan(fw.saved) and fw.info == -77, what
    fw = R.layer_forward_direct(c, saved_short=1)
    assert fw.rc == R.WORKSPACE_TOO_SMALL and all(np.isnan(v).all() for v in fw.out.values()) and _all_nan(fw.saved) and fw.info == -77
    fw = R.layer_forward_direct(c)
    _clean(fw, "forward")
    for null in ("g_mean", "g_var"):                            # the absent upstream gradient is a vector of zeros, never NULL
        bw = R.layer_backward_direct(fw, null=(null,))
        assert bw.rc == R.BAD_ARG and all(np.isnan(v).all() for v in bw.out.values()), null
    cs = [R.layer_case(*R.LAYER_SPLIT_CASES[1]), c]             # M = 129 and M = 8 in one chain call
    ch = R.chain_forward_direct(cs)
    assert ch.rc == R.BAD_ARG and _all_nan(ch.blocks) and ch.info == [-77, -77] and all(np.isnan(k) for k in ch.kl)
