"""The Gram kernels directly: every forward instantiation (kind x d-bucket x replica path) through
mobocmf_gram_forward_rep against an extended-precision reference with a componentwise bound, and the backward
instantiations the layer tests did not reach (kind 1, every d-bucket, xdiv 8 / 16, with and without d/dx, and the general
path an f that is only 8-byte aligned falls back to) through the layer against its oracle.

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
