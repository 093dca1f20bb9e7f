"""The row-side Gram backward directly (mobocmf_gram_backward_rows, gram_rows.hip): every instantiation (kind x d-bucket), the
general and both fast-path replica widths, the row-group and chunk / activity-block edges, the K_mm mode, column activity with
poisoned inactive blocks, misaligned pointers, determinism, extents and refusals -- against the extended-precision reference
of tests/gram_rows_reference.py with the bound |got - ref| <= 2^-53 (c W + D A) per component: c = kernel_reference.GRAM_BWD_C,
D = gram_rows_depth of the geometry the size query reports; components whose W is below 1e-290 must be within 1e-300."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gram_rows_reference as Z
from tests import kernel_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV)


def _store(n1, Np, G, pad=0, offset=0):
    """G inside a NaN store of round_up(n1, 64) rows: rows >= n1 and the slack stay NaN (neither may be read)."""
    S = R.Strided((n1 + 63) // 64 * 64, Np, pad, offset)
    S.view[:n1].copy_(dev(G))
    return S


def _offset(a, off):
    buf = torch.full((a.shape[0] + off + 1,), R.NAN, dtype=torch.float64, device=DEV)
    v = buf[off:off + a.shape[0]]
    v.copy_(torch.as_tensor(a))
    return v


def _run(kind, d, n1, nbase2, xdiv, c, Gs, colact=None, symmetric=0, f2=None):
    return Z.gram_rows(kind, d, dev(c["x1"]), dev(c["f1"]), n1, dev(c["x2"]), dev(c["f2"]) if f2 is None else f2, nbase2, xdiv,
                       dev(c["hyp"]), Gs.view, Gs.ld, colact, symmetric)


def _check(res, ref, xdiv, n1, d, what):
    assert res.untouched, what + ": a write beyond g_x1's or the workspace's extent"
    D = Z.gram_rows_depth(res.geometry, xdiv, n1, d)
    bad, ratio, frac = R.gram_bwd_violations(res.out, ref, D)
    print(f"{what}: worst err / (2^-53 W) {ratio:.2f}, {frac:.3f} of the bound (c = {R.GRAM_BWD_C}, D = {D['g_x1']}, geometry {res.geometry})")
    assert bad == 0, what + f": {bad} components outside the bound, worst {frac:.3g} of it"
    return ratio, frac


@pytest.mark.parametrize("xdiv", Z.ROWS_XDIV)
@pytest.mark.parametrize("kind", [0, 1])
def test_gram_rows_componentwise(kind, xdiv):
    d = 3
    worst = (0.0, 0.0)
    for n1 in Z.ROWS_N1:
        for nbase2 in Z.ROWS_NBASE2:
            c = R.gram_case(kind, d, n1, nbase2, xdiv)
            Np = nbase2 * xdiv
            G, _ = R.gram_bwd_inputs(n1, Np, seed=n1 + nbase2)
            ref = Z.gram_rows_hp(kind, c, xdiv, G)
            res = _run(kind, d, n1, nbase2, xdiv, c, _store(n1, Np, G))
            worst = tuple(map(max, worst, _check(res, ref, xdiv, n1, d, f"kind={kind} xdiv={xdiv} n1={n1} nbase2={nbase2}")))
    print(f"rows kind={kind} xdiv={xdiv}: worst ratio {worst[0]:.2f} (c = {R.GRAM_BWD_C}), {worst[1]:.3f} of the bound")


@pytest.mark.parametrize("d", Z.ROWS_D)
@pytest.mark.parametrize("kind", [0, 1])
def test_gram_rows_every_width(kind, d):
    """d = 32: exponents leave float64's range and the "tiny" rule decides."""
    for n1, nbase2, xdiv in Z.ROWS_D_CASES:
        c = R.gram_case(kind, d, n1, nbase2, xdiv)
        Np = nbase2 * xdiv
        G, _ = R.gram_bwd_inputs(n1, Np, seed=d)
        ref = Z.gram_rows_hp(kind, c, xdiv, G)
        res = _run(kind, d, n1, nbase2, xdiv, c, _store(n1, Np, G))
        _check(res, ref, xdiv, n1, d, f"kind={kind} d={d} n1={n1} nbase2={nbase2} xdiv={xdiv}")


_ACT = {"middle_off": lambda n: [0 if 0 < i < n - 1 else 1 for i in range(n)], "first_only": lambda n: [1] + [0] * (n - 1),
        "none": lambda n: [0] * n, "scattered": lambda n: [1 if i % 3 == 1 or i == n - 1 else 0 for i in range(n)]}


@pytest.mark.parametrize("pattern", list(_ACT))
@pytest.mark.parametrize("kind,xdiv,nbase2", [(0, 1, 385), (0, 3, 129), (1, 3, 171), (1, 8, 50), (1, 16, 40)])
def test_gram_rows_column_activity(kind, xdiv, nbase2, pattern):
    """At least three 128-column blocks; the inactive ones hold NaN in G, are never read and count as exact zeros."""
    d, n1 = 3, 65
    Np = nbase2 * xdiv
    nblk = (Np + 127) // 128
    assert nblk >= 3
    act = _ACT[pattern](nblk)
    mask = R.column_mask(act, Np)
    c = R.gram_case(kind, d, n1, nbase2, xdiv)
    G, _ = R.gram_bwd_inputs(n1, Np, seed=xdiv)
    Gn = np.where(mask[None, :], G, np.nan)
    assert np.isnan(Gn).sum() == n1 * int((~mask).sum())
    ref = Z.gram_rows_hp(kind, c, xdiv, Gn, act)
    res = _run(kind, d, n1, nbase2, xdiv, c, _store(n1, Np, Gn), torch.tensor(act, dtype=torch.int32, device=DEV))
    assert not np.isnan(res.out["g_x1"]).any()
    _check(res, ref, xdiv, n1, d, f"kind={kind} xdiv={xdiv} nbase2={nbase2} {pattern}")
    if pattern == "none":
        assert not res.out["g_x1"].any(), "exact zeros"


@pytest.mark.parametrize("n", [1, 33, 65])
@pytest.mark.parametrize("kind", [0, 1])
def test_gram_rows_symmetric_mode(kind, n):
    d = 3
    c, G = Z.symmetric_case(kind, d, n)
    ref = Z.gram_rows_hp(kind, c, 1, G, symmetric=True)
    res = _run(kind, d, n, n, 1, c, _store(n, n, G), symmetric=1)
    _check(res, ref, 1, n, d, f"symmetric kind={kind} n={n}")
    one = _run(kind, d, n, n, 1, c, _store(n, n, G), symmetric=0)
    assert np.array_equal(res.out["g_x1"], 2.0 * one.out["g_x1"])


@pytest.mark.parametrize("kind,xdiv", [(0, 1), (1, 8), (1, 3)])
def test_gram_rows_misaligned_pointers_and_determinism(kind, xdiv):
    """G and f2 only 8-byte aligned and an odd ldk: the same values, bit for bit; two calls are bitwise equal."""
    d, n1, nbase2 = 3, 33, 129
    Np = nbase2 * xdiv
    c = R.gram_case(kind, d, n1, nbase2, xdiv)
    G, _ = R.gram_bwd_inputs(n1, Np, seed=3)
    a = _run(kind, d, n1, nbase2, xdiv, c, _store(n1, Np, G))
    b = _run(kind, d, n1, nbase2, xdiv, c, _store(n1, Np, G))
    assert np.array_equal(a.out["g_x1"], b.out["g_x1"]) and torch.equal(a.ws[:a.geometry[0] * n1 * d], b.ws[:a.geometry[0] * n1 * d])
    _check(a, Z.gram_rows_hp(kind, c, xdiv, G), xdiv, n1, d, f"kind={kind} xdiv={xdiv}")
    for g_off, pad, f_off in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        Gs = _store(n1, Np, G, pad + ((Np + pad + 1) % 2 if pad else 0), g_off)
        assert Gs.view.data_ptr() % 16 == 8 * g_off and (not pad or Gs.ld % 2 == 1)
        f2 = _offset(c["f2"], 1) if (f_off and kind == 1) else None
        r = _run(kind, d, n1, nbase2, xdiv, c, Gs, f2=f2)
        assert r.untouched and np.array_equal(r.out["g_x1"], a.out["g_x1"]), (g_off, pad, f_off)


def test_gram_rows_refuses_bad_arguments():
    from mobocmf_amd import _lib
    kind, d, n1, nbase2, xdiv = 1, 3, 31, 127, 8
    c = R.gram_case(kind, d, n1, nbase2, xdiv)
    Np = nbase2 * xdiv
    G, _ = R.gram_bwd_inputs(n1, Np)
    a = dict(x1=dev(c["x1"]), f1=dev(c["f1"]), x2=dev(c["x2"]), f2=dev(c["f2"]), hyp=dev(c["hyp"]), G=dev(G))

    def call(ldk=Np, ws_bytes=None, symmetric=0, **kw):
        v = dict(a, kind=kind, d=d, n1=n1, nbase2=nbase2, xdiv=xdiv)
        v.update(kw)
        return Z.gram_rows(v["kind"], v["d"], v["x1"], v["f1"], v["n1"], v["x2"], v["f2"], v["nbase2"], v["xdiv"], v["hyp"], v["G"],
                           ldk, None, symmetric, ws_bytes=ws_bytes, check=False, **{k: kw[k] for k in ("g_x1", "ws") if k in kw})

    nbytes, geo = Z.gram_rows_geometry(kind, d, n1, nbase2, xdiv)
    assert geo[0] * n1 * d * 8 <= nbytes < geo[0] * n1 * d * 8 + 256
    assert not isinstance(call(), int)
    assert call(ws_bytes=nbytes - 8) == _lib.WORKSPACE_TOO_SMALL and call(ws_bytes=0) == _lib.WORKSPACE_TOO_SMALL
    assert call(ldk=Np - 1) == _lib.BAD_ARG
    for k in ("x1", "f1", "x2", "f2", "hyp", "G", "g_x1", "ws"):
        assert call(**{k: None}) == _lib.BAD_ARG, k
    assert call(symmetric=1) == _lib.BAD_ARG and call(symmetric=2) == _lib.BAD_ARG          # n1 != nbase2, xdiv != 1
    assert call(symmetric=1, nbase2=n1, xdiv=8, ldk=Np) == _lib.BAD_ARG
    lib, nb, g3 = R.lib(), ctypes.c_size_t(), (ctypes.c_int32 * 3)()
    q = lambda kind=kind, d=d, n1=n1, nbase2=nbase2, xdiv=xdiv, out=ctypes.byref(nb): \
        lib.mobocmf_gram_backward_rows_workspace_bytes(kind, d, n1, nbase2, xdiv, out, g3)
    assert q() == _lib.OK and nb.value == nbytes and q(out=None) == _lib.BAD_ARG
    for kw in (dict(kind=2), dict(kind=-1), dict(d=0), dict(d=33), dict(n1=0), dict(nbase2=0), dict(xdiv=0), dict(xdiv=49),
               dict(n1=65535 * 64 + 1)):
        assert q(**kw) == _lib.BAD_ARG, kw
        if kw.get("n1", 0) <= n1:
            assert call(**kw) == _lib.BAD_ARG, kw
    # kind 0 needs neither f1 nor f2
    c0 = R.gram_case(0, d, n1, nbase2, 1)
    G0, _ = R.gram_bwd_inputs(n1, nbase2)
    r = Z.gram_rows(0, d, dev(c0["x1"]), None, n1, dev(c0["x2"]), None, nbase2, 1, dev(c0["hyp"]), dev(G0), nbase2)
    assert r.untouched and np.isfinite(r.out["g_x1"]).all()


def test_gram_rows_wide_launch_geometry():
    """M = 512 against 16 384 columns (xdiv 8): eight row groups, more than one tile per wavefront is not needed yet (the
    grid stays under the cap); and a launch wide enough that the chunks double.  Only eight column blocks are active, so the
    reference covers 512 x 1024 elements."""
    kind, d, n1, xdiv = 1, 2, 512, 8
    for nbase2 in (2048, 16384):
        Np = nbase2 * xdiv
        nblk = Np // 128
        _, geo = Z.gram_rows_geometry(kind, d, n1, nbase2, xdiv)
        assert geo[1] == 8 and geo[0] * geo[1] <= 2048 and geo[0] == -(-nbase2 // geo[2])
        assert (geo[2] == 16) == (nbase2 == 2048)
        blocks = sorted({0, nblk - 1} | {(nblk * i) // 7 + (i % 2) for i in range(1, 7)})
        act = [1 if b in blocks else 0 for b in range(nblk)]
        c = R.gram_case(kind, d, n1, nbase2, xdiv)
        Gb, _ = R.gram_bwd_inputs(n1, 128 * len(blocks), seed=5)
        cols = np.concatenate([np.arange(128 * b, 128 * b + 128) for b in blocks])
        sub = dict(c, x2=c["x2"][cols[::xdiv] // xdiv], f2=c["f2"][cols])
        ref = Z.gram_rows_hp(kind, sub, xdiv, Gb)
        Gd = torch.full((n1, Np), R.NAN, dtype=torch.float64, device=DEV)
        Gd[:, torch.as_tensor(cols, device=DEV)] = dev(Gb)
        res = Z.gram_rows(kind, d, dev(c["x1"]), dev(c["f1"]), n1, dev(c["x2"]), dev(c["f2"]), nbase2, xdiv, dev(c["hyp"]), Gd, Np,
                          torch.tensor(act, dtype=torch.int32, device=DEV))
        assert res.geometry == geo
        _check(res, ref, xdiv, n1, d, f"wide nbase2={nbase2} geometry={geo}")
