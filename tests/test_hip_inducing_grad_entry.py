"""The `_z` variants of the backward halves (mobocmf_layer_backward_z, mobocmf_layer_panel_backward_z,
mobocmf_layers_chain_backward_z) through ctypes on kernel_reference.layer_case problems: every output other than g_Zx is
bitwise the plain call's; the whole call's g_Zx is the PANEL share plus the CHAIN share of the split calls (two float64
vectors added in another order: 1e-12 of the max-norm); g_Zx against autograd over the float64 layer oracle; an activity
pattern that leaves column blocks of dK unwritten (and poisoned: every workspace is NaN before a call); refusals."""
import ctypes

import numpy as np
import pytest
import torch

from tests import kernel_reference as R

pytestmark = pytest.mark.gpu
CASES = [(kind, 2, M, 40 if xdiv == 8 else 300, xdiv, 0, 0, False, 0, 1) for kind in (0, 1) for M in (33, 65) for xdiv in (1, 8)
         if not (kind == 0 and xdiv == 8)] + [(0, 2, 33, 300, 1, 1, 0, False, 0, 0), (0, 2, 65, 300, 1, 1, 0, False, 0, 0)]


def _zbytes(desc):
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert R.lib().mobocmf_inducing_grad_workspace_bytes(ctypes.byref(desc), ctypes.byref(a), ctypes.byref(b)) == 0
    assert a.value % 256 == 0 and b.value % 256 == 0 and a.value > 0 and b.value > 0
    return a.value, b.value


def _zws(nbytes):
    return torch.full((nbytes // 8 + R.GUARD,), R.NAN, dtype=torch.float64, device="cuda")


def _guard_ok(ws, nbytes):
    return bool(torch.isnan(ws[nbytes // 8:]).all())


def layer_backward_z(fw, c, zws_bytes=None, zws=None):
    r = R.LayerCall()
    lens = R._grad_lens(c, ("g_hyp", "g_m", "g_LS", "g_x", "g_f", "g_zf"))
    lens["g_Zx"] = c["M"] * c["d"]
    bufs = {k: R._out(n) for k, n in lens.items()}
    scratch = R._nan_bytes(fw.cb)
    up = {k: R._dev(c[k]) for k in ("g_mean", "g_var")}
    gkl = R._dev(np.array([c["g_kl"]]))
    pb, cbz = _zbytes(fw.desc)
    need = pb + cbz
    ws = _zws(need) if zws is None else zws
    i, p = fw.inp, R._p
    r.rc = R.lib().mobocmf_layer_backward_z(ctypes.byref(fw.desc), p(i["x"]), p(i["f"]), p(i["Zx"]), p(i["zf"]), p(i["hyp"]), p(i["m"]),
                                            p(i["L_S"]), p(up["g_mean"]), p(up["g_var"]), p(gkl), p(bufs.get("g_f")), p(bufs.get("g_zf")),
                                            p(bufs["g_hyp"]), p(bufs["g_m"]), p(bufs["g_LS"]), p(bufs.get("g_x")), p(bufs["g_Zx"]),
                                            p(fw.saved), fw.sb, p(scratch), fw.cb, p(ws), need if zws_bytes is None else zws_bytes,
                                            R._stream())
    R._collect(r, bufs, lens)
    r.untouched = r.untouched and _guard_ok(ws, need)
    r.ws = ws
    return r


def panel_backward_z(pf, c, zws_bytes=None):
    r = R.LayerCall()
    lens = R._grad_lens(c, ("g_hyp", "g_x", "g_f", "g_zf"))
    lens["g_Zx"] = c["M"] * c["d"]
    bufs = {k: R._out(n) for k, n in lens.items()}
    scratch = R._nan_bytes(pf.cb)
    gm, gv = R._dev(c["g_mean"]), R._dev(c["g_var"])
    need = _zbytes(pf.desc)[0]
    ws = _zws(need)
    i, p = pf.inp, R._p
    r.rc = R.lib().mobocmf_layer_panel_backward_z(ctypes.byref(pf.desc), p(pf.x), p(pf.f), p(i["Zx"]), p(i["zf"]), p(i["hyp"]), p(gm), p(gv),
                                                  p(bufs.get("g_f")), p(bufs.get("g_zf")), p(bufs["g_hyp"]), p(bufs.get("g_x")),
                                                  p(bufs["g_Zx"]), p(pf.block), pf.block.numel(), p(pf.saved), pf.sb, p(scratch), pf.cb,
                                                  p(ws), need if zws_bytes is None else zws_bytes, R._stream())
    R._collect(r, bufs, lens)
    r.untouched = r.untouched and _guard_ok(ws, need)
    return r


def chain_backward_z(ch, g_kl, had_panel, shares, zws_bytes=None):
    n = len(ch.cs)
    lens, bufs = [], []
    for z, c in enumerate(ch.cs):
        l = R._grad_lens(c, ("g_hyp", "g_m", "g_LS", "g_zf"))
        l["g_Zx"] = c["M"] * c["d"]
        b = {k: R._out(m) for k, m in l.items()}
        b["g_hyp"] = shares[z].bufs["g_hyp"]
        if "g_zf" in b:
            b["g_zf"] = shares[z].bufs["g_zf"]
        lens.append(l)
        bufs.append(b)
    gk = [R._dev(np.array([g])) for g in g_kl]
    T = lambda k: R._tab([i[k] for i in ch.inp])
    B = lambda k: R._tab([b.get(k) for b in bufs])
    need = sum(_zbytes(d)[1] for d in ch.descs)
    ws = _zws(need)
    rc = R.lib().mobocmf_layers_chain_backward_z(n, R._desc_table(ch.descs), T("Zx"), T("zf"), T("hyp"), R._tab(gk),
                                                 (ctypes.c_int32 * n)(*had_panel), B("g_zf"), B("g_hyp"), B("g_m"), B("g_LS"), B("g_Zx"),
                                                 R._p(ch.blocks), ch.stride, ch.blocks.numel(), R._p(ws),
                                                 need if zws_bytes is None else zws_bytes, R._stream())
    outs = []
    for z in range(n):
        r = R.LayerCall()
        r.rc = rc
        R._collect(r, bufs[z], lens[z])
        r.untouched = r.untouched and _guard_ok(ws, need)
        outs.append(r)
    return outs


def _bits_equal(a, b, names):
    for k in names:
        x, y = np.ascontiguousarray(a.out[k]).reshape(-1), np.ascontiguousarray(b.out[k]).reshape(-1)
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), k


def _oracle_gZx(c):
    """dL/dZ_x by autograd over the float64 oracle: L = g_mean . mean + g_var . var + g_kl kl."""
    from oracle import mfdgp_oracle as O
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    Zx = t(c["Zx"]).clone().requires_grad_(True)
    hyp = {k: t(v) for k, v in R.hyp_dict(c["kind"], c["hyp"], c["d"]).items()}
    x = t(c["x"]).repeat_interleave(c["xdiv"], 0)
    Xt = x if c["kind"] == 0 else torch.cat([x, t(c["f"])[:, None]], 1)
    Zt = Zx if c["kind"] == 0 else torch.cat([Zx, t(c["zf"])[:, None]], 1)
    mean, var, _ = O.layer_moments(hyp, Xt, Zt, t(c["m"]), t(c["L_S"]), jitter=c["jitter"], training=c["branch"] == 0, shortcut=False)
    kl = O.kl_layer(hyp, Zt, t(c["m"]), t(c["L_S"]), c["jitter"])
    ((t(c["g_mean"]) * mean).sum() + (t(c["g_var"]) * var).sum() + c["g_kl"] * kl).backward()
    return Zx.grad.numpy()


def _whole_and_split(c):
    fw = R.layer_forward_direct(c)
    assert fw.rc == 0 and fw.info == 0
    plain = R.layer_backward_direct(fw, c)
    fw2 = R.layer_forward_direct(c)
    zc = layer_backward_z(fw2, c)
    assert plain.rc == 0 and zc.rc == 0 and zc.untouched
    _bits_equal(plain, zc, plain.out)
    gz = zc.out["g_Zx"].reshape(c["M"], c["d"])
    assert np.isfinite(gz).all()
    # the split calls: plain against `_z`, and the two shares
    ch = R.chain_forward_direct([c])
    pf = R.panel_forward_direct(ch, 0, c)
    pb = R.panel_backward_direct(pf, c)
    ch2 = R.chain_forward_direct([c])
    pf2 = R.panel_forward_direct(ch2, 0, c)
    pbz = panel_backward_z(pf2, c)
    assert pb.rc == 0 and pbz.rc == 0 and pbz.untouched
    _bits_equal(pb, pbz, pb.out)
    panel_share = pbz.out["g_Zx"].copy()
    cb = R.chain_backward_direct(ch, [c["g_kl"]], [2], [pb])[0]
    cbz = chain_backward_z(ch2, [c["g_kl"]], [2], [pbz])[0]
    assert cb.rc == 0 and cbz.rc == 0 and cbz.untouched
    _bits_equal(cb, cbz, cb.out)
    both = (panel_share + cbz.out["g_Zx"]).reshape(c["M"], c["d"])
    assert np.max(np.abs(gz - both)) <= 1e-12 * np.max(np.abs(gz)), np.max(np.abs(gz - both)) / np.max(np.abs(gz))
    return gz


@pytest.mark.parametrize("key", CASES, ids=[f"kind{k[0]}-M{k[2]}-xdiv{k[4]}-dx{k[9]}" for k in CASES])
def test_z_variants_keep_every_other_output_and_add_up(key):
    c = R.layer_case(*key)
    gz = _whole_and_split(c)
    ref = _oracle_gZx(c)
    # cond(K_mm) <= 1e3 on these problems (kernel_reference.layer_case): the oracle and the device agree far below 1e-8
    err = np.max(np.abs(gz - ref)) / np.max(np.abs(ref))
    print(f"{key}: |g_Zx - oracle| / max|oracle| = {err:.2e}")
    assert err < 1e-8, err


@pytest.mark.parametrize("pattern", list(R.LAYER_ACTIVITY))
@pytest.mark.parametrize("key", [(0, 2, 65, 640, 1, 0, 0, False, 0, 1), (1, 2, 33, 80, 8, 0, 0, False, 0, 1)], ids=["kind0", "kind1"])
def test_z_variants_with_unwritten_column_blocks(key, pattern):
    """Whole 128-column blocks of exactly zero upstream gradients: those blocks of dK are never written (the scratch is NaN
    before every call) and the row-side backward must not read them."""
    c, _ = R.activity_case(R.layer_case(*key), pattern)
    gz = _whole_and_split(c)
    ref = _oracle_gZx(c)
    err = np.max(np.abs(gz - ref)) / np.max(np.abs(ref))
    print(f"{key} {pattern}: |g_Zx - oracle| / max|oracle| = {err:.2e}")
    assert err < 1e-8, err


def test_z_variants_refuse_before_any_launch():
    c = R.layer_case(1, 2, 33, 40, 8)
    fw = R.layer_forward_direct(c)
    pb, cb = _zbytes(fw.desc)
    r = layer_backward_z(fw, c, zws_bytes=pb + cb - 8)
    assert r.rc == R.WORKSPACE_TOO_SMALL and all(np.isnan(v).all() for v in r.out.values()) and bool(torch.isnan(r.ws).all())
    ch = R.chain_forward_direct([c])
    pf = R.panel_forward_direct(ch, 0, c)
    r = panel_backward_z(pf, c, zws_bytes=pb - 8)
    assert r.rc == R.WORKSPACE_TOO_SMALL and all(np.isnan(v).all() for v in r.out.values())
    # constant parameters: no chain backward follows, no inducing-input gradient either
    pfc = R.panel_forward_direct(ch, 0, c, params_const=1, block=R.chain_block(ch, 0, state_only=True).clone())
    assert pfc.rc == 0
    r = panel_backward_z(pfc, c)
    assert r.rc == R.BAD_ARG and all(np.isnan(v).all() for v in r.out.values())
    ok = R.panel_backward_direct(pf, c)
    r = chain_backward_z(ch, [c["g_kl"]], [2], [ok], zws_bytes=cb - 8)[0]
    assert r.rc == R.WORKSPACE_TOO_SMALL and np.isnan(r.out["g_m"]).all() and np.isnan(r.out["g_Zx"]).all()
    # a workspace inside the call's own scratch is refused
    fw = R.layer_forward_direct(c)
    lens = R._grad_lens(c, ("g_hyp", "g_m", "g_LS", "g_x", "g_f", "g_zf"))
    bufs = {k: R._out(n) for k, n in lens.items()}
    gz = R._out(c["M"] * c["d"])
    scratch = R._nan_bytes(fw.cb)
    i, p = fw.inp, R._p
    rc = R.lib().mobocmf_layer_backward_z(ctypes.byref(fw.desc), p(i["x"]), p(i["f"]), p(i["Zx"]), p(i["zf"]), p(i["hyp"]), p(i["m"]),
                                          p(i["L_S"]), p(R._dev(c["g_mean"])), p(R._dev(c["g_var"])), p(R._dev(np.array([0.37]))),
                                          p(bufs.get("g_f")), p(bufs.get("g_zf")), p(bufs["g_hyp"]), p(bufs["g_m"]), p(bufs["g_LS"]),
                                          p(bufs.get("g_x")), p(gz), p(fw.saved), fw.sb, p(scratch), fw.cb, p(scratch), pb + cb,
                                          R._stream())
    assert rc == R.BAD_ARG and bool(torch.isnan(gz).all())
