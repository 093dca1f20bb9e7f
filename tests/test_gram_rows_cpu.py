"""CPU side of the row-side Gram backward's yardsticks (tests/gram_rows_reference.py): the transposed-case reference against
autograd over the oracle's Gram matrix, the float64 restatement against the longdouble reference on every shape the GPU test
uses (the constant GRAM_BWD_RATIO_MEASURED must carry over: an addend of g_x1 is an addend of the transposed case's g_x2),
the summation depth, and a finite-difference check of oracle.elbo with respect to Z_x -- the model-level yardstick."""
import numpy as np
import pytest
import torch

from mobocmf_amd.util import synthetic
from oracle import mfdgp_oracle as O
from tests import gram_rows_reference as Z
from tests import kernel_reference as R
from tests.helpers import oracle_state, to_t


def _shapes():
    out = [(kind, 3, n1, nb, xdiv) for kind in (0, 1) for n1 in Z.ROWS_N1 for nb in Z.ROWS_NBASE2 for xdiv in Z.ROWS_XDIV]
    out += [(kind, d, n1, nb, xdiv) for kind in (0, 1) for d in Z.ROWS_D for n1, nb, xdiv in Z.ROWS_D_CASES]
    return out


def _ratio(f64, hp):
    v, W, _ = hp["g_x1"]
    err = np.abs(R.ld(f64["g_x1"][0]) - v)
    tiny = W < R.ld(1e-290)
    assert bool(np.all(err[tiny] <= R.ld(1e-300)))
    return float(np.max(np.where(tiny, 0, err / (R.ld(R.U) * np.where(tiny, 1, W))), initial=0.0))


@pytest.mark.parametrize("kind", [0, 1])
def test_restatement_stays_within_the_measured_constant(kind):
    worst = 0.0
    for k, d, n1, nb, xdiv in _shapes():
        if k != kind:
            continue
        c = R.gram_case(kind, d, n1, nb, xdiv)
        G, _ = R.gram_bwd_inputs(n1, nb * xdiv, seed=n1 + nb)
        r = _ratio(Z.gram_rows_f64(kind, c, xdiv, G), Z.gram_rows_hp(kind, c, xdiv, G))
        assert r <= R.GRAM_BWD_RATIO_MEASURED, (kind, d, n1, nb, xdiv, r)
        worst = max(worst, r)
    for n in (1, 33, 65):
        c, G = Z.symmetric_case(kind, 3, n)
        r = _ratio(Z.gram_rows_f64(kind, c, 1, G, symmetric=True), Z.gram_rows_hp(kind, c, 1, G, symmetric=True))
        assert r <= R.GRAM_BWD_RATIO_MEASURED, (kind, n, r)
        worst = max(worst, r)
    print(f"kind {kind}: worst err / (2^-53 W) of the float64 restatement {worst:.2f} of {R.GRAM_BWD_RATIO_MEASURED}")


def _hyp(kind, hyp, d):
    return {k: to_t(v) for k, v in R.hyp_dict(kind, hyp, d).items()}


@pytest.mark.parametrize("kind", [0, 1])
def test_reference_matches_autograd_over_the_oracle_gram(kind):
    """Away from near-coincident points (where autograd's x / ls - z / ls cancels, kernel_reference "Gram backward") the two
    agree to a few ulps of the sum of magnitudes A."""
    d, n1, nb, xdiv = 3, 33, 129, 3
    c = dict(R.gram_case(kind, d, n1, nb, xdiv))
    G, _ = R.gram_bwd_inputs(n1, nb * xdiv, seed=1)
    ref, _, A = Z.gram_rows_hp(kind, c, xdiv, G)["g_x1"]
    x1 = to_t(c["x1"], True)
    X1 = x1 if kind == 0 else torch.cat([x1, to_t(c["f1"])[:, None]], 1)
    x2 = to_t(c["x2"]).repeat_interleave(xdiv, 0)
    X2 = x2 if kind == 0 else torch.cat([x2, to_t(c["f2"])[:, None]], 1)
    (O.gram(_hyp(kind, c["hyp"], d), X1, X2) * to_t(G)).sum().backward()
    err = np.abs(R.ld(x1.grad.numpy()) - ref)
    assert float(np.max(err / A)) < 1e-10, float(np.max(err / A))
    # symmetric mode against autograd with ONE leaf on both sides
    cs, Gs = Z.symmetric_case(kind, d, 33)
    ref, _, A = Z.gram_rows_hp(kind, cs, 1, Gs, symmetric=True)["g_x1"]
    z = to_t(cs["x1"], True)
    Zt = z if kind == 0 else torch.cat([z, to_t(cs["f1"])[:, None]], 1)
    (O.gram(_hyp(kind, cs["hyp"], d), Zt, Zt) * to_t(Gs)).sum().backward()
    err = np.abs(R.ld(z.grad.numpy()) - ref)
    assert float(np.max(err / A)) < 1e-10, float(np.max(err / A))


def test_depth_follows_the_geometry():
    """No device needed: the size query is a host computation."""
    for n1, nb, xdiv, want in ((33, 129, 1, (2, 1, 128)), (65, 257, 3, (6, 2, 44)), (512, 2048, 8, (128, 8, 16)),
                               (512, 16384, 8, (256, 8, 64)), (31, 1, 16, (1, 1, 8))):
        nbytes, geo = Z.gram_rows_geometry(1, 3, n1, nb, xdiv)
        assert geo == want and nbytes == (geo[0] * n1 * 3 * 8 + 255) // 256 * 256, (geo, nbytes)
        wb = geo[2] // 4
        D = Z.gram_rows_depth(geo, xdiv, n1, 3)["g_x1"]
        assert D == xdiv + wb + -(-wb * xdiv // 32) + 4 + R.GRAM_BWD_MULS + R.sum_depth(geo[0], n1 * 3)


@pytest.mark.parametrize("cfg", [dict(d=2, L=2, M=8, N=96, S=1, seed=0), dict(d=3, L=2, M=16, N=128, S=1, seed=2),
                                 dict(d=4, L=2, M=12, N=150, S=1, seed=3), dict(d=3, L=3, M=10, N=16, S=2, seed=7)])
def test_oracle_elbo_gradient_wrt_Zx_matches_central_differences(cfg):
    prob = synthetic.make_problem(**cfg)
    st = oracle_state(prob)
    x, y, fid = to_t(prob["x"]), to_t(prob["y"]), to_t(prob["fid"])
    eps = [None] + [to_t(e) for e in prob["eps"][1:]]
    S = cfg["S"]

    def f(Zx):
        return O.elbo(dict(st, Zx=Zx), x, y, fid, eps=eps, S=S)[0]

    Z0 = st["Zx"].clone().requires_grad_(True)
    f(Z0).backward()
    g = Z0.grad
    h = 1e-6
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(12):
        i, k = int(rng.integers(Z0.shape[0])), int(rng.integers(Z0.shape[1]))
        E = torch.zeros_like(st["Zx"])
        E[i, k] = h
        with torch.no_grad():
            fd = float((f(st["Zx"] + E) - f(st["Zx"] - E)) / (2 * h))
        worst = max(worst, abs(fd - float(g[i, k])) / float(g.abs().max()))
    print(f"{cfg}: worst |fd - autograd| / max|g| = {worst:.2e}")
    assert worst < 1e-5, worst
