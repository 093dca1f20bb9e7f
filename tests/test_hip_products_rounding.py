"""The product entry points on inexact, badly scaled data: a componentwise a-priori bound against an extended-precision
reference.

Rows of A and columns of B are scaled by 10^U(-6, 6), so the entries of one product span ~24 orders of magnitude -- as
A = L^-1 K_mn does between rows -- and a max-norm comparison would only see the few largest.  The assertion is
    |C - ref| <= (n_ops + 2) 2^-53 R        for every element,
with n_ops the longest chain of floating-point operations behind an element (Kd plus the epilogue's few; Mr + Kd for the
column statistics) and R the same expression evaluated with the absolute values of all operands: the textbook bound for ANY
summation order, with or without FMA (for the sum of squares it is the specified chain length, see the comment there).  No measured constant enters; the reference's own error (K 2^-64 R) is 2^-11 of it.
"""
import numpy as np
import pytest
import torch

from tests import kernel_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float64))).to(DEV)


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


_REFS = {}


def _products(key, A, B):
    """(A B, |A||B|) in extended precision, computed once per data set and shared by the cases that use it."""
    if key not in _REFS:
        _REFS[key] = (R.matmul_hp(A, B), R.matmul_hp(np.abs(A), np.abs(B)))
    return _REFS[key]


def _data(Mr, Nc, Kd, seed, tri=0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((Mr, Kd)) * 10.0 ** rng.uniform(-6, 6, (Mr, 1))
    B = rng.standard_normal((Kd, Nc)) * 10.0 ** rng.uniform(-6, 6, (1, Nc))
    if tri & 3:
        A = A * R.tri_mask(Mr, bool(tri & 1))
    if tri & 12:
        B = B * R.tri_mask(Kd, bool(tri & 4))
    return A, B


def _check(got, ref, Rabs, n_ops, what):
    ok, ratio = R.componentwise_ok(host(got), ref, Rabs, n_ops)
    print(f"{what}: worst |err| / (2^-53 R) = {ratio:.2f}, allowed {n_ops + 2}")
    assert ok, f"{what}: worst |err| / (2^-53 R) = {ratio:.2f} > {n_ops + 2}"


GEMM_CASES = [("small", (208, 176, 240), {}), ("mid32", (256, 256, 512), dict(mid_gemm_waves=32)),
              ("mid8", (256, 256, 512), dict(mid_gemm_waves=8)), ("mid4", (256, 256, 512), dict(mid_gemm_waves=4)),
              ("tiled", (256, 256, 512), dict(R.TILED, small_panel_max=16))]


@pytest.mark.parametrize("trans_b", [0, 1])
@pytest.mark.parametrize("family,shape,kw", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_componentwise(family, shape, kw, trans_b):
    Mr, Nc, Kd = shape
    tune = R.make_tuning(**kw)
    A, B = _data(Mr, Nc, Kd, seed=Mr + Kd)
    ref, Rabs = _products(("gemm", shape), A, B)
    Ad = R.Strided(Mr, Kd, 2, 2, fill=A)
    Bd = R.Strided(Nc, Kd, 2, 2, fill=B.T) if trans_b else R.Strided(Kd, Nc, 2, 2, fill=B)
    C = R.Strided(Mr, Nc, 2, 2)
    R.gemm(Ad, Bd, C, Mr, Nc, Kd, trans_b=trans_b, tune=tune)
    _check(C.view, ref, Rabs, Kd, f"{family} trans_b={trans_b}")
    assert C.slack_untouched()
    # accumulate with a scale: C0 + alpha A B, two more operations per element
    C0 = np.random.default_rng(1).standard_normal((Mr, Nc)) * np.asarray(Rabs, np.float64)
    C.set(C0)
    R.gemm(Ad, Bd, C, Mr, Nc, Kd, trans_b=trans_b, alpha=-0.3, accumulate=1, tune=tune)
    _check(C.view, R.ld(C0) + R.ld(-0.3) * ref, np.abs(R.ld(C0)) + R.ld(0.3) * Rabs, Kd + 2, f"{family} accumulate")


@pytest.mark.parametrize("family,shape,kw", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_cancellation(family, shape, kw):
    """A = [P, -P], B = [Q; Q (1 + 1e-9)]: the result is 1e-9 of the sum of absolute values behind it -- a kernel that loses
    low-order terms (a dropped k-slice boundary, a truncated partial) is outside the bound, one that only reorders is inside."""
    Mr, Nc, Kd = shape
    P, Q = _data(Mr, Nc, Kd // 2, seed=5)
    A, B = np.concatenate([P, -P], 1), np.concatenate([Q, Q * (1 + 1e-9)], 0)
    ref, Rabs = _products(("cancel", shape), A, B)
    assert float(np.median(np.abs(ref) / Rabs)) < 1e-8
    Ad, Bd, C = R.Strided(Mr, Kd, fill=A), R.Strided(Kd, Nc, fill=B), R.Strided(Mr, Nc)
    R.gemm(Ad, Bd, C, Mr, Nc, Kd, tune=R.make_tuning(**kw))
    _check(C.view, ref, Rabs, Kd, f"{family} cancellation")


EPI_CASES = [("panel", {}), ("tiled64", dict(small_panel_max=16, tile_rows=64, pair_mode=2)),
             ("tiled128", dict(small_panel_max=16, tile_rows=128, pair_mode=2))]


@pytest.mark.parametrize("tri", [1, 2], ids=["lowerA", "upperA"])
@pytest.mark.parametrize("name,kw", EPI_CASES, ids=[c[0] for c in EPI_CASES])
def test_epilogues_componentwise(name, kw, tri):
    Mr = Kd = Nc = 256
    tune = R.make_tuning(**kw)
    rng = np.random.default_rng(11)
    A, B = _data(Mr, Nc, Kd, seed=17, tri=tri)
    Aaux = rng.standard_normal((Mr, Nc)) * 10.0 ** rng.uniform(-6, 6, (Mr, 1))
    avec = rng.standard_normal(Mr) * 10.0 ** rng.uniform(-3, 3, Mr)
    bscale, gmu, cgv = (rng.standard_normal(Nc) * 10.0 ** rng.uniform(-3, 3, Nc) for _ in range(3))
    AB, ABabs = _products(("epi", tri), A, B)
    Ad, Bd, C = R.Strided(Mr, Kd, 2, 2, fill=A), R.Strided(Kd, Nc, 2, 2, fill=B), R.Strided(Mr, Nc, 2, 2)
    alpha = 0.7
    # epi 0
    R.gemm_epilogue(Ad, Bd, C, Mr, Nc, Kd, tri, 0, alpha=alpha, tune=tune)
    _check(C.view, R.ld(alpha) * AB, R.ld(alpha) * ABabs, Kd + 1, f"{name} epi0")
    # epi 1: C and the column statistics of the C the kernel formed
    rows = R.colstat_rows(tri, Mr, Nc, Kd, tune)
    p1 = torch.full((rows, Nc), R.NAN, dtype=torch.float64, device=DEV)
    p2 = p1.clone()
    C.poison()
    R.gemm_epilogue(Ad, Bd, C, Mr, Nc, Kd, tri, 1, alpha=alpha, colsq=p1, coldot=p2, avec=dev(avec), tune=tune)
    Cr, Ca = R.ld(alpha) * AB, R.ld(alpha) * ABabs
    _check(C.view, Cr, Ca, Kd + 1, f"{name} epi1 C")
    colsq = R.ld(host(p1)).sum(0)                 # the partial rows are added in extended precision: no error of the test's own
    coldot = R.ld(host(p2)).sum(0)
    # Mr + Kd is the chain length the bound is specified with.  It is not the rigorous worst case for colsq: squaring a C that
    # carries (Kd + 1) u of error gives 2 (Kd + 1) + Mr.  It holds because R is formed from absolute values while the actual
    # errors of a sum accumulate like a random walk; should a correct re-tiling ever trip it, revisit this constant, not the kernel.
    _check(colsq, (Cr * Cr).sum(0), (Ca * Ca).sum(0), Mr + Kd, f"{name} colsq")
    _check(coldot, R.ld(avec) @ Cr, np.abs(R.ld(avec)) @ Ca, Mr + Kd, f"{name} coldot")
    # epi 2
    C.poison()
    parts = Nc // 16 if name == "panel" else 2 * (Nc // 128)
    rd = torch.full((parts, Mr), R.NAN, dtype=torch.float64, device=DEV)
    Ax = R.Strided(Mr, Nc, 2, 2, fill=Aaux)
    R.gemm_epilogue(Ad, Bd, C, Mr, Nc, Kd, tri, 2, alpha=alpha, avec=dev(avec), bscale=dev(bscale), gmu=dev(gmu), cgv=dev(cgv),
                    Aaux=Ax, rowdot=rd, tune=tune)
    l = R.ld
    want = l(alpha) * l(bscale)[None, :] * AB + l(avec)[:, None] * l(gmu)[None, :] - 2 * l(Aaux) * l(cgv)[None, :]
    wabs = l(alpha) * np.abs(l(bscale))[None, :] * ABabs + np.abs(l(avec))[:, None] * np.abs(l(gmu))[None, :] \
        + 2 * np.abs(l(Aaux)) * np.abs(l(cgv))[None, :]
    _check(C.view, want, wabs, Kd + 6, f"{name} epi2 C")
    rowdot = R.ld(host(rd)).sum(0)
    _check(rowdot, l(Aaux) @ l(gmu), np.abs(l(Aaux)) @ np.abs(l(gmu)), Nc, f"{name} rowdot")
    assert C.slack_untouched()


@pytest.mark.parametrize("name,Kd,kw", [("small", 256, {}), ("tiled", 512, dict(small_gemm_max=16)),
                                        ("tiled16", 512, dict(small_gemm_max=16, syrk_workgroups=16))])
def test_weighted_syrk_componentwise(name, Kd, kw):
    Mr = 256
    rng = np.random.default_rng(23)
    A = rng.standard_normal((Mr, Kd)) * 10.0 ** rng.uniform(-6, 6, (Mr, 1))
    w = rng.standard_normal(Kd) * 10.0 ** rng.uniform(-3, 3, Kd)
    ref = R.matmul_hp(R.ld(A) * R.ld(w)[None, :], A.T)
    Rabs = R.matmul_hp(np.abs(R.ld(A)) * np.abs(R.ld(w))[None, :], np.abs(A.T))
    H = torch.full((Mr, Mr), R.NAN, dtype=torch.float64, device=DEV)
    R.syrk(R.Strided(Mr, Kd, 2, 2, fill=A), dev(w), H, Mr, Kd, tune=R.make_tuning(**kw))
    # a term is two products, the Kd terms are added in some order (k-slices and slabs are one such order): Kd + 1 operations
    _check(H, ref, Rabs, Kd + 1, f"syrk {name}")
    assert torch.equal(H, H.T)
