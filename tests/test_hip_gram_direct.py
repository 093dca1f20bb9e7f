"""The Gram kernels directly: every forward instantiation (kind x d-bucket x replica path) through
mobocmf_gram_forward_rep against an extended-precision reference with a componentwise bound; every backward instantiation
(kind x d-bucket x d/dx x replica path), its column-activity path, its three launch geometries and the three forms of its
reduction through mobocmf_gram_backward against an extended-precision reference with a bound on the sum of the addends'
magnitudes (kernel_reference.py, "Gram backward"); and the backward once more through the layer against its oracle.

Forward bound per element: c (2 + |arg|) 2^-53 |term|, summed over the terms of kind 1, with arg the exponent's magnitude
(lengthscales down to 0.05: |arg| reaches the thousands and float64 underflows) and c = kernel_reference.GRAM_C, four times
the worst ratio measured for the float64 CPU restatement (tests/test_kernel_reference_cpu.py).  Elements whose reference is
below 1e-290 must agree to 1e-300 absolutely.
"""
import numpy as np
import pytest
import torch

from tests import kernel_reference as R
from tests.test_hip_layer import _close, _mk, _oracle, _pack

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV)


def _offset(a, off):
    """Device copy of the vector ``a`` starting ``off`` doubles into its allocation (off = 1: 8-byte aligned only)."""
    buf = torch.full((a.shape[0] + off + 1,), R.NAN, dtype=torch.float64, device=DEV)
    v = buf[off:off + a.shape[0]]
    v.copy_(torch.as_tensor(a))
    assert v.data_ptr() % 16 == (8 * off) % 16
    return v


@pytest.mark.parametrize("xdiv", R.GRAM_XDIV)
@pytest.mark.parametrize("d", R.GRAM_D)
@pytest.mark.parametrize("kind", [0, 1])
def test_gram_forward_componentwise(kind, d, xdiv):
    worst = 0.0
    for n1 in R.GRAM_N1:
        for nbase2 in R.GRAM_NBASE2:
            c = R.gram_case(kind, d, n1, nbase2, xdiv)
            K_ref, W, knn_ref = R.gram_hp(kind, c, xdiv)
            w, Mp = nbase2 * xdiv, (n1 + 31) // 32 * 32
            x1, f1, x2, hyp = dev(c["x1"]), dev(c["f1"]), dev(c["x2"]), dev(c["hyp"])
            for pad in (0, 2):
                for off in ((0, 1) if kind == 1 else (0,)):
                    what = f"kind={kind} d={d} xdiv={xdiv} n1={n1} nbase2={nbase2} ldk=w+{pad} f2 offset={off}"
                    f2 = _offset(c["f2"], off) if kind == 1 else None
                    K = R.Strided(Mp, w, pad)
                    knn = torch.full((w + 1,), R.NAN, dtype=torch.float64, device=DEV) if pad else None
                    R.gram_rep(kind, d, x1, f1, n1, x2, f2, nbase2, xdiv, hyp, K.view, K.ld, knn)
                    got = K.view.cpu().numpy()
                    bad, ratio = R.gram_violations(got[:n1], K_ref, W)
                    worst = max(worst, ratio)
                    assert bad == 0, what + f": {bad} elements outside the bound, worst ratio {ratio:.1f} > c = {R.GRAM_C}"
                    assert not got[n1:].any(), what + ": padding rows must be zero"
                    assert K.slack_untouched(), what + ": columns beyond the width were written"
                    if knn is not None:
                        kn = knn.cpu().numpy()
                        assert np.isnan(kn[w]), what
                        err = np.abs(R.ld(kn[:w]) - knn_ref)
                        assert bool(np.all(err <= 8 * R.U * np.abs(knn_ref))), what + ": knn"       # positive terms, five operations
    print(f"kind={kind} d={d} xdiv={xdiv}: worst ratio {worst:.2f} of c = {R.GRAM_C}")


def test_gram_functional_replicas_match_the_direct_call():
    from mobocmf_amd import functional as F
    c = R.gram_case(1, 3, 31, 127, 8)
    K, knn = F.gram(1, dev(c["x1"]), dev(c["f1"]), dev(c["x2"]), dev(c["f2"]), dev(c["hyp"]), xdiv=8, knn=True)
    Kd = R.Strided(32, 127 * 8)
    kd = torch.empty(127 * 8, dtype=torch.float64, device=DEV)
    R.gram_rep(1, 3, dev(c["x1"]), dev(c["f1"]), 31, dev(c["x2"]), dev(c["f2"]), 127, 8, dev(c["hyp"]), Kd.view, Kd.ld, kd)
    assert K.shape == (31, 127 * 8) and torch.equal(K, Kd.view[:31]) and torch.equal(knn, kd)
    K1 = F.gram(1, dev(c["x1"]), dev(c["f1"]), dev(c["x2"]), dev(c["f2"][::8].copy()), dev(c["hyp"]))
    assert K1.shape == (31, 127)
    from mobocmf_amd import _lib
    with pytest.raises(_lib.MobocmfError):
        F.gram(1, dev(c["x1"]), dev(c["f1"]), dev(c["x2"]), dev(c["f2"]), dev(c["hyp"]), xdiv=49)


# ----------------------------------------------------------------------------------------- backward, through the layer
_BWD = [(d, xdiv, dx, off) for d in (2, 9, 32) for xdiv in (8, 16) for dx in (True, False) for off in (False, True)
        if not (off and xdiv != 8)]


@pytest.mark.parametrize("d,xdiv,want_dx,offset_f", _BWD,
                         ids=[f"d{d}-xdiv{x}-{'dx' if dx else 'nodx'}-{'f_8_byte_aligned' if o else 'aligned_f'}" for d, x, dx, o in _BWD])
def test_layer_backward_replica_paths(d, xdiv, want_dx, offset_f):
    """kind 1 at M = 40, nbase = 150 (two column blocks of base rows) with the tolerances of tests/test_hip_layer.py.  An f
    that is only 8-byte aligned must take the general path of the Gram forward and backward: every consumer of f in the
    layer path either tests the alignment (gram.hip: vec_ok) or reads single doubles."""
    from mobocmf_amd import functional as F
    kind, M, nbase, branch = 1, 40, 150, 0
    x, f, Zx, zf, hyp, m, L_S = _mk(kind, d, M, nbase, xdiv, seed=300 + d + xdiv)
    if d == 2:
        # 40 inducing points in [0, 1]^2 under _mk's lengthscales of 0.8 .. 1.8 give a K_mm whose condition number is set by
        # the jitter (4e7 for this seed: cond x 2^-53 = 5e-9): neither the oracle nor the device can deliver the KL to the
        # 1e-10 of tests/test_hip_layer.py there.  A quarter of the lengthscale: cond ~ 1e4, as in that file's own cases.
        hyp["ls1"], hyp["ls2"] = hyp["ls1"] * 0.25, hyp["ls2"] * 0.25
    Np = nbase * xdiv
    rng = np.random.default_rng(7)
    w = [torch.tensor(rng.standard_normal(Np)), torch.tensor(rng.standard_normal(Np)), torch.tensor(0.37)]
    mean_o, var_o, kl_o = _oracle(kind, x, f, Zx, zf, hyp, m, L_S, xdiv, branch, w)
    g = lambda t, rg=True: t.detach().to(DEV).requires_grad_(rg)
    xg, Zg, zfg, mg, LSg = g(x, want_dx), g(Zx, False), g(zf), g(m), g(L_S)
    fg = (_offset(f.detach().numpy(), 1) if offset_f else f.detach().to(DEV)).requires_grad_(True)
    hg = _pack(kind, {k: v.detach() for k, v in hyp.items()}).to(DEV).requires_grad_(True)
    mean, var, kl = F.layer_forward(xg, fg, Zg, zfg, hg, mg, LSg, kind, xdiv=xdiv, branch=branch, want_dx=want_dx)
    _close(mean, mean_o, 1e-9, "mean")
    _close(var, var_o, 1e-8, "var")
    _close(kl, kl_o, 1e-10, "kl")
    ((w[0].to(DEV) * mean).sum() + (w[1].to(DEV) * var).sum() + w[2].to(DEV) * kl).backward()
    _close(mg.grad, m.grad, 1e-7, "g_m")
    _close(LSg.grad, torch.tril(L_S.grad), 1e-7, "g_LS")
    _close(hg.grad, _pack(kind, {k: v.grad for k, v in hyp.items()}), 1e-7, "g_hyp")
    _close(fg.grad, f.grad, 1e-7, "g_f")
    _close(zfg.grad, zf.grad, 1e-7, "g_zf")
    if want_dx:
        _close(xg.grad, x.grad, 1e-7, "g_x")
    else:
        assert xg.grad is None


# ------------------------------------------------------------------------------------ backward, direct (mobocmf_gram_backward)
# Bound per output component: 2^-53 (c W + D A), c = kernel_reference.GRAM_BWD_C, D = kernel_reference.gram_bwd_depth of the
# geometry the size query reports; components whose W is below 1e-290 must be within 1e-300 of the reference.
def _colact(active):
    return None if active is None else torch.tensor(list(active), dtype=torch.int32, device=DEV)


def _bwd_check(kind, d, n1, nbase2, xdiv, res, ref, want_dx, what):
    """All outputs of one call against ``ref``; returns (err / (2^-53 W), fraction of the bound), the worst of each."""
    want = {"hyp", "g_x2"} if kind == 0 else set(R.GRAM_BWD_OUTPUTS)
    want -= set() if want_dx else {"g_x2"}
    assert set(res.out) == want, what
    assert res.untouched, what + ": a write beyond an output's or the workspace's extent"
    D = R.gram_bwd_depth(kind, d, n1, nbase2, xdiv, res.geometry)
    bad, ratio, frac = R.gram_bwd_violations(res.out, {k: ref[k] for k in want}, D)
    print(f"{what}: worst err / (2^-53 W) {ratio:.2f}, {frac:.3f} of the bound (c = {R.GRAM_BWD_C}, D = {D})")
    assert bad == 0, what + f": {bad} components outside the bound, worst {frac:.3g} of it"
    return ratio, frac


def _G_store(n1, Np, G, pad=0, offset=0):
    """G inside a NaN store of round_up(n1, 32) rows: the rows >= n1 and the slack stay NaN (neither is read)."""
    S = R.Strided((n1 + 31) // 32 * 32, Np, pad, offset)
    S.view[:n1].copy_(dev(G))
    return S


@pytest.mark.parametrize("xdiv", R.GRAM_XDIV)
@pytest.mark.parametrize("d", R.GRAM_D)
@pytest.mark.parametrize("kind", [0, 1])
def test_gram_backward_componentwise(kind, d, xdiv):
    """Every instantiation: with and without d/dx, with and without gknn, 1 .. 3 workgroups of 128 base rows, 1 .. 5 of 8 rows
    of x1.  Kind 1 at xdiv 8 / 16 also the three ways off the vector path (f2 or G only 8-byte aligned, an odd ldk).  That the
    general instantiation ran there cannot be shown from outside: the geometry is the same, both instantiations add the same
    values in the same order (bitwise equal results), and the hardware serves a 16-byte load from an 8-byte aligned address --
    what is shown is that the values are right and nothing beyond the extents is touched."""
    worst = (0.0, 0.0)
    for n1 in R.GRAM_N1:
        for nbase2 in R.GRAM_BWD_NBASE2:
            c = R.gram_case(kind, d, n1, nbase2, xdiv)
            Np = nbase2 * xdiv
            G, gk = R.gram_bwd_inputs(n1, Np, seed=n1 + nbase2)
            ref0 = R.gram_bwd_hp(kind, c, xdiv, G)
            ref1 = R.gram_bwd_hp_with_knn(kind, c, ref0, gk)
            x1, f1, x2, hyp, gkd = dev(c["x1"]), dev(c["f1"]), dev(c["x2"]), dev(c["hyp"]), dev(gk)
            f2 = dev(c["f2"])
            variants = [(0, 0, 0, dx, kn) for dx in (True, False) for kn in (True, False)]
            if kind == 1 and xdiv in (8, 16):
                variants += [(1, 0, 0, True, True), (0, 1, 0, False, True), (0, 0, 1, True, False)]
            for f_off, g_off, pad, want_dx, with_knn in variants:
                what = (f"kind={kind} d={d} xdiv={xdiv} n1={n1} nbase2={nbase2} dx={want_dx} gknn={with_knn} "
                        f"f2 offset={f_off} G offset={g_off} ldk=w+{pad}")
                Gs = _G_store(n1, Np, G, pad, g_off)
                assert Gs.view.data_ptr() % 16 == 8 * g_off and Gs.ld == Np + pad
                fv = _offset(c["f2"], 1) if f_off else f2
                res = R.gram_bwd(kind, d, x1, f1, n1, x2, fv, nbase2, xdiv, hyp, Gs.view, Gs.ld, gkd if with_knn else None,
                                 None, want_dx)
                worst = tuple(map(max, worst, _bwd_check(kind, d, n1, nbase2, xdiv, res, ref1 if with_knn else ref0, want_dx, what)))
    print(f"backward kind={kind} d={d} xdiv={xdiv}: worst ratio {worst[0]:.2f} (c = {R.GRAM_BWD_C}), {worst[1]:.3f} of the bound")


# xdiv -> base rows giving a width that is / is not a multiple of 128.  8 and 16 divide 128 (a row's replicas share a block:
# the vector instantiations' all-or-nothing mask); 3 and 48 do not (replicas straddle block boundaries, per-replica mask)
_ACT_NBASE = {1: (384, 385), 3: (256, 257), 8: (160, 150), 16: (160, 150), 48: (40, 41)}
_ACT_PATTERNS = dict(R.ACTIVITY, scattered=lambda n: [1 if i % 3 == 1 or i == n - 1 else 0 for i in range(n)])


@pytest.mark.parametrize("pattern", list(_ACT_PATTERNS))
@pytest.mark.parametrize("kind,xdiv", [(0, 1), (0, 3), (1, 3), (1, 8), (1, 16), (1, 48)])
def test_gram_backward_column_activity(kind, xdiv, pattern):
    """Inactive 128-column blocks of G hold NaN and count as exact zeros; gknn is zero there, as a layer's is."""
    d, n1 = 3, 33
    worst = (0.0, 0.0)
    for nbase2 in _ACT_NBASE[xdiv]:
        Np = nbase2 * xdiv
        act = _ACT_PATTERNS[pattern]((Np + 127) // 128)
        mask = R.column_mask(act, Np)
        c = R.gram_case(kind, d, n1, nbase2, xdiv)
        G, gk = R.gram_bwd_inputs(n1, Np, seed=xdiv, active=act)
        ref = R.gram_bwd_hp(kind, c, xdiv, G, gk, act)
        Gn = np.where(mask[None, :], G, np.nan)
        assert np.isnan(Gn).sum() == n1 * int((~mask).sum()) and not gk[~mask].any()
        for want_dx in (True, False):
            what = f"kind={kind} xdiv={xdiv} nbase2={nbase2} Np={Np} {pattern} dx={want_dx}"
            Gs = _G_store(n1, Np, Gn)
            res = R.gram_bwd(kind, d, dev(c["x1"]), dev(c["f1"]), n1, dev(c["x2"]), dev(c["f2"]), nbase2, xdiv, dev(c["hyp"]),
                             Gs.view, Gs.ld, dev(gk), _colact(act), want_dx)
            worst = tuple(map(max, worst, _bwd_check(kind, d, n1, nbase2, xdiv, res, ref, want_dx, what)))
            if kind == 1:
                z = res.out["g_f2"][~mask]
                assert z.size == int((~mask).sum()) and not z.any() and not np.isnan(z).any(), what + ": g_f2 of an inactive block"
            if pattern == "none":
                assert all(not v.any() and not np.isnan(v).any() for v in res.out.values()), what + ": exact zeros everywhere"
    print(f"backward activity kind={kind} xdiv={xdiv} {pattern}: worst ratio {worst[0]:.2f}, {worst[1]:.3f} of the bound")


# (n1, nbase2) -> (rows per workgroup, reduction form of the hyp, g_f1, g_f2, g_x2 tasks; 0 serial, 1 wide, 2 four-way), at
# kind 0 / xdiv 1 and kind 1 / xdiv 8 alike (kind 0 has no g_f1 / g_f2).  gram_rows_per_block: 32 rows from grid x * Mp >= 32768,
# 16 from 16384, else 8.
_GEOMETRY = {
    (512, 8192): (32, (1, 1, 2, 2)),      # 64 x 16 workgroups
    (256, 8192): (16, (1, 1, 2, 2)),      # 64 x 16
    (512, 512): (8, (1, 0, 1, 1)),        # 4 x 64: 64 partials per column and <= 4096 columns -- the wide form for g_f2 / g_x2
    (33, 2048): (8, (1, 2, 0, 0)),        # 16 x 8
    (64, 384): (8, (2, 0, 0, 0)),         # 3 x 8
    (31, 129): (8, (0, 0, 0, 0)),         # 2 x 4
}


def test_gram_backward_geometry_cases_cover_every_rule():
    assert {g for g, _ in _GEOMETRY.values()} == {8, 16, 32}
    for task in range(4):
        assert {f[task] for _, f in _GEOMETRY.values()} == {0, 1, 2}, task


@pytest.mark.parametrize("kind,xdiv", [(0, 1), (1, 8)])
@pytest.mark.parametrize("n1,nbase2", list(_GEOMETRY))
def test_gram_backward_launch_geometry(n1, nbase2, kind, xdiv):
    """The three rows-per-workgroup values and the three reduction forms of every task, asserted from the geometry the size
    query reports.  The launch has the full grid; at most 8 column blocks are active (the first and the last among them), so
    the reference covers n1 x 1024 elements.  (512, 512) at kind 0 is the one dense case."""
    d = 2
    Np = nbase2 * xdiv
    nblk = (Np + 127) // 128
    gm, forms = _GEOMETRY[(n1, nbase2)]
    _, geo = R.gram_bwd_geometry(kind, d, n1, nbase2, xdiv, True)
    tasks = R.gram_bwd_tasks(kind, d, n1, nbase2, xdiv, geo)
    assert geo == ((nbase2 + 127) // 128, (n1 + 31) // 32 * 32 // gm, gm)
    got_forms = {k: R.sum_form(*pl) for k, pl in tasks.items()}
    want_forms = dict(zip(("hyp", "g_f1", "g_f2", "g_x2"), forms))
    assert got_forms == {k: want_forms[k] for k in tasks}, (geo, tasks)
    c = R.gram_case(kind, d, n1, nbase2, xdiv)
    what = f"kind={kind} xdiv={xdiv} n1={n1} nbase2={nbase2} geometry={geo}"
    Gd = torch.full((n1, Np), R.NAN, dtype=torch.float64, device=DEV)           # n1 is a multiple of 32 or the store is small
    if nblk <= 8 or Np % 128:
        act = None
        G, gk = R.gram_bwd_inputs(n1, Np, seed=5)
        ref = R.gram_bwd_hp(kind, c, xdiv, G, gk)
        Gd.copy_(dev(G))
    else:
        blocks = sorted({0, nblk - 1} | {(nblk * i) // 7 + (i % 2) for i in range(1, 7)})
        assert len(blocks) == 8 and blocks[-1] == nblk - 1
        act = [1 if b in blocks else 0 for b in range(nblk)]
        Gb, gkb = R.gram_bwd_inputs(n1, 128 * len(blocks), seed=5)
        ref = R.gram_bwd_hp_blocks(kind, c, xdiv, blocks, Gb, gkb)
        cols = torch.as_tensor(np.concatenate([np.arange(128 * b, 128 * b + 128) for b in blocks]), device=DEV)
        Gd[:, cols] = dev(Gb)
        gk = np.zeros(Np)
        gk[cols.cpu().numpy()] = gkb
    res = R.gram_bwd(kind, d, dev(c["x1"]), dev(c["f1"]), n1, dev(c["x2"]), dev(c["f2"]), nbase2, xdiv, dev(c["hyp"]), Gd, Np,
                     dev(gk), _colact(act), True)
    assert res.geometry == geo
    ratio, frac = _bwd_check(kind, d, n1, nbase2, xdiv, res, ref, True, what)
    if act is not None and kind == 1:
        assert not res.out["g_f2"][~R.column_mask(act, Np)].any(), what


def test_gram_backward_refuses_bad_arguments():
    from mobocmf_amd import _lib
    import ctypes
    kind, d, n1, nbase2, xdiv = 1, 3, 31, 127, 8
    c = R.gram_case(kind, d, n1, nbase2, xdiv)
    Np = nbase2 * xdiv
    G, gk = R.gram_bwd_inputs(n1, Np)
    a = dict(x1=dev(c["x1"]), f1=dev(c["f1"]), x2=dev(c["x2"]), f2=dev(c["f2"]), hyp=dev(c["hyp"]), G=dev(G))

    def call(ldk=Np, ws_bytes=None, **kw):
        v = dict(a, kind=kind, d=d, n1=n1, nbase2=nbase2, xdiv=xdiv)
        v.update(kw)
        return R.gram_bwd(v["kind"], v["d"], v["x1"], v["f1"], v["n1"], v["x2"], v["f2"], v["nbase2"], v["xdiv"], v["hyp"], v["G"],
                          ldk, dev(gk), None, True, ws_bytes=ws_bytes, check=False)

    nbytes, _ = R.gram_bwd_geometry(kind, d, n1, nbase2, xdiv, True)
    assert not isinstance(call(), int)
    assert call(ws_bytes=nbytes - 8) == _lib.WORKSPACE_TOO_SMALL and call(ws_bytes=0) == _lib.WORKSPACE_TOO_SMALL
    nodx, _ = R.gram_bwd_geometry(kind, d, n1, nbase2, xdiv, False)
    assert nodx < nbytes and call(ws_bytes=nodx) == _lib.WORKSPACE_TOO_SMALL           # the d/dx partials count
    assert call(ldk=Np - 1) == _lib.BAD_ARG
    for k in ("x1", "f1", "x2", "f2", "hyp", "G"):
        assert call(**{k: None}) == _lib.BAD_ARG, k
    lib, nb, geo = R.lib(), ctypes.c_size_t(), (ctypes.c_int32 * 3)()
    q = lambda kind=kind, d=d, n1=n1, nbase2=nbase2, xdiv=xdiv, out=ctypes.byref(nb): \
        lib.mobocmf_gram_backward_workspace_bytes(kind, d, n1, nbase2, xdiv, 1, out, geo)
    assert q() == _lib.OK and nb.value == nbytes and q(out=None) == _lib.BAD_ARG
    for kw in (dict(kind=2), dict(kind=-1), dict(d=0), dict(d=33), dict(n1=0), dict(nbase2=0), dict(xdiv=0), dict(xdiv=49)):
        assert q(**kw) == _lib.BAD_ARG, kw
        # the launch refuses the same shapes, every pointer given, before it looks at the workspace (of no bytes here)
        out = [torch.empty(n, dtype=torch.float64, device=DEV) for n in (64, n1, Np, nbase2 * d, 8)]
        rc = lib.mobocmf_gram_backward(kw.get("kind", kind), kw.get("d", d), R._p(a["x1"]), R._p(a["f1"]), kw.get("n1", n1),
                                       R._p(a["x2"]), R._p(a["f2"]), kw.get("nbase2", nbase2), kw.get("xdiv", xdiv), R._p(a["hyp"]),
                                       R._p(a["G"]), Np * 8, None, None, R._p(out[0]), R._p(out[1]), R._p(out[2]), R._p(out[3]),
                                       R._p(out[4]), 0, R._stream())
        assert rc == _lib.BAD_ARG, kw
    # kind 0 needs neither f nor the f gradients
    c0 = R.gram_case(0, d, n1, nbase2, 1)
    G0, _ = R.gram_bwd_inputs(n1, nbase2)
    r = R.gram_bwd(0, d, dev(c0["x1"]), None, n1, dev(c0["x2"]), None, nbase2, 1, dev(c0["hyp"]), dev(G0), nbase2, None, None, False)
    assert set(r.out) == {"hyp"} and r.untouched

