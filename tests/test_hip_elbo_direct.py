"""The fused ELBO (mobocmf_elbo_forward / _backward, F.elbo_fused) against an extended-precision restatement of
variational_elbo_mf.py:24-51 (tests/kernel_reference.py: elbo_hp).

Sizes sit on both sides of the one-block path (every layer <= 4096 entries: one launch of one workgroup; beyond it a
reduction launch over ceil(n / 1024) workgroups plus a one-block tail).  Covered: L in {1, 3, 8} with absent layers, div in
{1, 3, 8}, rows[l] in {B, a prefix, 0}, the Interval noise and hi <= lo (raw is tau), a fidelity level no row has, n_kl in
{0, 8}, scale in {0, 0.37}, upstream gradients on elbo only, on scaled_kl only, on both.

Bounds: the three scalars and g_raw_noise within (n + 16) 2^-53 sum|terms| (n summed entries: any summation order, plus the
few operations of tau, log tau and the tail); g_mean / g_var within 8 2^-53 |ref| per element, exactly 0 on masked rows, and
NOT WRITTEN beyond a layer's prefix (the buffers are NaN-filled).
"""
import numpy as np
import pytest
import torch

from tests import kernel_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE_BLOCK_ENTRIES = 4096             # elementwise.hip: elbo_blocks() <= 4 blocks of 1024 entries -> the one-block kernels


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float64))).to(DEV)


DEAD_LEVEL = {3: 0, 8: 7}            # the fidelity level no row has (a layer that holds all B rows)


def _problem(L, B, seed):
    """Layer l: div = (1, 3, 8)[l % 3] (L = 1: 8), rows = (B, a prefix, 0)[(l + l // 3) % 3] -- so div 8 meets rows 0 (layer 2)
    and rows B (layer 5); layers 3 and 6 of an 8-layer problem are absent.  The level no row has is a layer that holds all B
    rows (level 0 at L = 3, level 7 at L = 8), never the prefix layer: the prefix (layer 1) ends in the MIDDLE of its own
    level's rows, so it carries live terms and a cut that matters.  Interval noise and raw = tau (hi <= lo) both meet live
    layers: L = 3 Interval on the prefix layer; L = 8 Interval on even layers (0 live), raw = tau on odd ones (1, 5 live)."""
    rng = np.random.default_rng(seed)
    dead = DEAD_LEVEL.get(L)
    levels = [l for l in range(L) if l != dead]
    fid = np.sort(rng.choice(levels, B))[::-1].astype(np.float64).copy()      # descending fidelity, as the steps order a batch
    prefix = int((fid > 1).sum() + (fid == 1).sum() // 2 + 1)                  # all rows above level 1, half of level 1's own
    y = rng.standard_normal(B)
    layers = []
    for l in range(L):
        if L == 8 and l in (3, 6):
            layers.append(None)
            continue
        div = 8 if L == 1 else (1, 3, 8)[l % 3]
        rows = B if L == 1 else (B, prefix, 0)[(l + l // 3) % 3]
        interval = (l == 1) if L == 3 else (l % 2 == 0)
        lo, hi = ((1e-4, 2.0) if interval else (0.0, 0.0))
        raw = float(rng.standard_normal()) if hi > lo else 0.2 + float(rng.random())
        layers.append(dict(mean=rng.standard_normal(B * div), var=rng.random(B * div) + 1e-3, raw=raw, lo=lo, hi=hi, div=div,
                           rows=rows))
    return layers, y, fid


def _to_dev(layers):
    return [None if lay is None else dict(lay, mean=dev(lay["mean"]), var=dev(lay["var"]), raw=dev([lay["raw"]])) for lay in layers]


def _scalar_ok(got, ref, absref, n, what):
    err = abs(R.ld(got) - ref)
    bound = (n + 16) * R.ld(R.U) * absref
    assert err <= bound, f"{what}: |err| = {float(err):.3e} > (n + 16) u sum|terms| = {float(bound):.3e} (n = {n})"


CASES = [
    # B chosen so that the widest layer (div 8) holds exactly 4096 entries, or just more
    ("inside", 1, 512, 0, 0.37, "elbo"), ("beyond", 1, 513, 8, 0.37, "both"),
    ("inside", 3, 512, 8, 0.37, "both"), ("beyond", 3, 513, 0, 0.37, "elbo"), ("beyond", 3, 513, 8, 0.0, "skl"),
    ("inside", 8, 512, 8, 0.0, "both"), ("beyond", 8, 513, 8, 0.37, "skl"), ("inside", 8, 512, 0, 0.37, "elbo"),
    ("inside", 3, 512, 8, 0.37, "skl"), ("beyond", 8, 520, 8, 0.37, "both"),
]


@pytest.mark.parametrize("side,L,B,n_kl,scale,upstream", CASES,
                         ids=[f"{s}-L{L}-B{B}-kl{k}-scale{sc}-{u}" for s, L, B, k, sc, u in CASES])
def test_fused_elbo_against_extended_precision(side, L, B, n_kl, scale, upstream):
    layers, y, fid = _problem(L, B, seed=L * 1000 + B)
    widest = max(B * lay["div"] for lay in layers if lay is not None)
    assert (widest <= ONE_BLOCK_ENTRIES) == (side == "inside") and abs(widest - ONE_BLOCK_ENTRIES) <= 64
    rng = np.random.default_rng(5)
    kls = list(rng.random(n_kl) * 3.0)
    g_elbo = None if upstream == "skl" else -1.0 + 0.25 * float(rng.random())
    g_skl = None if upstream == "elbo" else 0.5 + float(rng.random())
    ref = R.elbo_hp(layers, y, fid, kls, scale, g_elbo, g_skl)
    dl, yd, fd = _to_dev(layers), dev(y), dev(fid)
    kd = [dev([k]) for k in kls]

    out = R.elbo_forward(dl, yd, fd, kd, scale).cpu().numpy()
    for i, name in enumerate(("elbo", "scaled_kl", "loss")):
        _scalar_ok(out[i], ref["out3"][i], ref["abs3"][i], ref["n_terms"], name)
    assert out[2] == -out[0]

    ge = None if g_elbo is None else dev([g_elbo])
    gs = None if g_skl is None else dev([g_skl])
    gm, gv, gr, gkl = R.elbo_backward(dl, yd, fd, scale, ge, gs)
    _scalar_ok(float(gkl[0]), ref["g_kl"], ref["g_kl_abs"], 0, "g_kl")
    for l, lay in enumerate(layers):
        if lay is None:
            continue
        nn = lay["rows"] * lay["div"]
        for name, got, want in (("g_mean", gm[l], ref["g_mean"][l]), ("g_var", gv[l], ref["g_var"][l])):
            got = got.cpu().numpy()
            assert np.isnan(got[nn:]).all(), f"{name}[{l}]: rows beyond the prefix of {lay['rows']} were written"
            w = want[:nn]
            assert not got[:nn][w == 0].any(), f"{name}[{l}]: masked rows must be exactly zero"
            err = np.abs(R.ld(got[:nn]) - w)
            assert bool(np.all(err <= 8 * R.ld(R.U) * np.abs(w))), \
                f"{name}[{l}]: worst |err| / (u |ref|) = {float(np.max(err / np.maximum(R.ld(R.U) * np.abs(w), R.ld(1e-300)))):.2f} > 8"
        _scalar_ok(float(gr[l][0]), ref["g_raw"][l], ref["g_raw_abs"][l], ref["n_raw"][l], f"g_raw_noise[{l}]")
    # a fidelity level no row has, a layer with no rows: their data terms are exactly zero
    if L >= 3:
        dead = DEAD_LEVEL[L]
        assert ref["n_raw"][dead] == 0 and layers[dead]["rows"] == B and float(gr[dead][0]) == 0.0
        assert layers[2]["rows"] == 0 and float(gr[2][0]) == 0.0
        # the prefix layer is live, and its prefix cuts through its own level's rows
        assert 0 < layers[1]["rows"] < B and 0 < ref["n_raw"][1] < int((fid == 1).sum()) * layers[1]["div"]


@pytest.mark.parametrize("L,B", [(3, 512), (1, 513)], ids=["one_block_with_an_empty_layer", "blocks_and_tail"])
def test_elbo_fused_autograd_wrapper(L, B):
    """F.elbo_fused (the autograd wrapper the models use; prefix layers hold rows * div entries, a layer of no rows has no
    storage and must still get a zero noise gradient) against the same reference."""
    from mobocmf_amd import functional as F
    layers, y, fid = _problem(L, B, seed=77)
    kls = [0.4, 1.1, 2.2]
    ref = R.elbo_hp(layers, y, fid, kls, 0.37, 1.0, 0.3)
    assert L == 1 or (0 < layers[1]["rows"] < B and ref["n_raw"][1] > 0)      # a live prefix layer of rows * div entries
    req = lambda t: t.requires_grad_(True)
    spec, leaves = [], []
    for lay in layers:
        nn = lay["rows"] * lay["div"]
        m, v, r = req(dev(lay["mean"][:nn])), req(dev(lay["var"][:nn])), req(dev([lay["raw"]]))
        leaves.append((m, v, r))
        spec.append((m, v, r, lay["div"], lay["lo"], lay["hi"], lay["rows"]))
    kd = [torch.tensor(k, dtype=torch.float64, device=DEV, requires_grad=True) for k in kls]
    elbo, skl, neg = F.elbo_fused(spec, dev(y), dev(fid), kd, 0.37)
    _scalar_ok(float(elbo), ref["out3"][0], ref["abs3"][0], ref["n_terms"], "elbo")
    _scalar_ok(float(skl), ref["out3"][1], ref["abs3"][1], ref["n_terms"], "scaled_kl")
    assert float(neg) == -float(elbo)
    (elbo + 0.3 * skl).backward()
    for l, (lay, (m, v, r)) in enumerate(zip(layers, leaves)):
        nn = lay["rows"] * lay["div"]
        for name, got, want in (("g_mean", m.grad, ref["g_mean"][l][:nn]), ("g_var", v.grad, ref["g_var"][l][:nn])):
            err = np.abs(R.ld(got.cpu().numpy()) - want)
            assert bool(np.all(err <= 8 * R.ld(R.U) * np.abs(want))), f"{name}[{l}]"
        _scalar_ok(float(r.grad[0]), ref["g_raw"][l], ref["g_raw_abs"][l], ref["n_raw"][l], f"g_raw_noise[{l}]")
    for k in kd:
        _scalar_ok(float(k.grad), ref["g_kl"], ref["g_kl_abs"], 0, "g_kl")
