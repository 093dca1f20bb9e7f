"""The factorisation chain against extended-precision references, entry by entry ("Kernel conformance tests"):
the three forms of the blocked Cholesky (chol.hip: potrf_coop_kernel, potrf_panel2_kernel, potrf_panel4_kernel, with
potrf_panel_pad_kernel<16> on a last panel of 1 .. 16 real columns), both routes of launch_trtri_z and the one-launch form's own
inverse, gemv_rows, exact_gp_mll_kernel, the column statistics of mobocmf_exact_gp_predict, and mobocmf_mf_kernel_combine.
Cases, references, bounds (each the a-priori bound of the algorithm the form runs, derived in tests/kernel_reference.py and
proved on float64 restatements by tests/test_kernel_reference_cpu.py) and the direct C-ABI callers are shared with that file.
Reference behaviour: torch.linalg.cholesky_ex inside gpytorch's psd_safe_cholesky and the exact-GP
baselines' predictive moments."""
import numpy as np
import pytest
import torch

from tests import kernel_reference as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _bits_zero(t):
    return bool((t.contiguous().view(torch.int64) == 0).all())


FACTOR_CASES = [(n, cols, f) for n in R.FACTOR_ORDERS for cols in R.POTRF_FORMS for f in R.factor_families(n)] \
    + [(R.FACTOR_ORDER_COOP_CAPS, 0, "rbf")]


@pytest.mark.parametrize("n,cols,family", FACTOR_CASES, ids=lambda v: str(v))
def test_factor_inverse_solve_and_likelihood_within_their_bounds(n, cols, family):
    K, y = R.factor_case(family, n)
    g = R.exact_gp(K, n + 3, y, R.make_tuning(potrf_cols=cols))
    assert g.info == 0
    assert g.K.slack_untouched()
    L, Li, npad = g.L, g.Li, g.npad
    # the strict upper triangles are bitwise zero, the padding is bitwise the identity
    assert _bits_zero(torch.triu(L, 1)) and _bits_zero(torch.triu(Li, 1))
    eye = torch.eye(npad - n, dtype=torch.float64, device=DEV)
    for M in (L, Li):
        assert _bits_zero(M[n:, :n])
        assert torch.equal(M[n:, n:], eye) and _bits_zero(M[n:, n:] * (1 - eye))
    assert _bits_zero(g.a[n:])
    Lh, Xh, ah = L[:n, :n].cpu().numpy(), Li[:n, :n].cpu().numpy(), g.a[:n].cpu().numpy()
    assert np.isfinite(Lh).all() and np.isfinite(Xh).all() and np.isfinite(ah).all()
    one = R.one_launch_runs(n, cols)
    okc, rc, fc = R.chol_check(Lh, K, Xh if one else None)
    oki, ri = R.trinv_check(Xh, Lh)
    oka, ra = R.solve_check(ah, Xh, y)
    okm, rm = R.mll_check(float(g.mll), Lh, ah)
    print("n=%d potrf_cols=%d %s (%s): |LL^T-K| %.2f uR = %.3f of its bound, |X-L^-1| %.2f uR of %d, a %.2f of %d, mll %.2f of %d"
          % (n, cols, family, "one launch" if one else "launch pairs", rc, fc, ri, n + R.TRINV_CX, ra, n + 2, rm, n + R.MLL_CLOG))
    assert okc, (rc, fc)
    assert oki, ri
    assert oka, ra
    assert okm, rm


_predict_states = {}


def _predict_state(family, n):
    if (family, n) not in _predict_states:
        K, y = R.factor_case(family, n)
        g = R.exact_gp(K, n + 3, y, R.make_tuning())
        assert g.info == 0
        _predict_states[(family, n)] = (g, g.Li[:n, :n].cpu().numpy(), g.a[:n].cpu().numpy(), g.state.clone())
    return _predict_states[(family, n)]


@pytest.mark.parametrize("family", ("rbf", "signed"))
@pytest.mark.parametrize("nt", R.PREDICT_NT)
@pytest.mark.parametrize("n", R.PREDICT_N)
def test_predictive_moments_within_their_bounds(n, nt, family):
    """mobocmf_exact_gp_predict called directly: nt off the 128 grid, ld > nt with NaN in the slack, Kreal = n < npad real rows
    in the triangular product's column statistics; nothing written beyond nt, the state left as it was."""
    g, Xh, ah, before = _predict_state(family, n)
    Kts, kss = R.cross_kernel(family, n, nt)
    mean, var, untouched = R.exact_gp_predict_direct(g, Kts, nt + 5, kss, R.make_tuning())
    assert untouched
    assert torch.equal(g.state.view(torch.int64), before.view(torch.int64))
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    okm, rm, okv, rv = R.predict_check(mean, var, Xh, ah, Kts, kss)
    print("n=%d nt=%d %s: mean %.2f uR, var %.2f uR of %d" % (n, nt, family, rm, rv, 2 * n + 4))
    assert okm, rm
    assert okv, rv


def _info(K, tune, state):
    return R.exact_gp(K, K.shape[0] + 3, np.ones(K.shape[0]), tune, state=state)


@pytest.mark.parametrize("cols", R.POTRF_FORMS)
@pytest.mark.parametrize("n", (16, 64, 65, 128, 130, 200))
def test_failed_pivot_is_reported_as_lapack_reports_it(n, cols):
    """A diagonal entry of -3, NaN or (first pivot) exactly zero: info is the order of the first leading minor that is not
    positive definite, as torch.linalg.cholesky_ex reports it; the first of two; and a good matrix through the same state
    afterwards reports 0."""
    tune = R.make_tuning(potrf_cols=cols)
    for family in ("rbf", "signed"):
        K, _ = R.factor_case(family, n)
        state = None
        for bad in sorted({b for b in (0, 15, 16, 63, 64, n - 1) if b < n}):
            for v in (-3.0, float("nan")) + ((0.0,) if bad == 0 else ()):
                Kb = K.copy()
                Kb[bad, bad] = v
                want = int(torch.linalg.cholesky_ex(torch.from_numpy(Kb)).info)
                assert want == bad + 1
                g = _info(Kb, tune, state)
                state = g.state
                assert g.info == want, (family, bad, v, g.info)
        pairs = [(5, n - 1)] if n <= 64 else [(5, 64)] + ([(70, 129)] if n > 129 else [])
        for b1, b2 in pairs:
            for v in (-3.0, float("nan")):
                Kb = K.copy()
                Kb[b1, b1] = v
                Kb[b2, b2] = -3.0
                g = _info(Kb, tune, state)
                assert g.info == b1 + 1 == int(torch.linalg.cholesky_ex(torch.from_numpy(Kb)).info), (family, b1, b2, v, g.info)
        g = _info(K, tune, state)
        assert g.info == 0 and bool(torch.isfinite(g.L).all()) and bool(torch.isfinite(g.Li).all())


@pytest.mark.parametrize("diag", (0.0, 3.0))
@pytest.mark.parametrize("with_s", (False, True))
@pytest.mark.parametrize("grid", (False, True), ids=("tight", "pad128"))
@pytest.mark.parametrize("n1,n2", ((1, 1), (37, 129), (130, 64)))
def test_mf_kernel_combine_is_exact_on_integers(n1, n2, grid, with_s, diag):
    """out = s1 s2 Ks + ntab[min(l1, l2)] Kn (+ diag): integer operands, so every output is an exact integer (|.| <= 4^3 + 4 * 4
    + 3); zero padding, identity on the padded diagonal when diag != 0, nothing beyond rows_p x cols_p or in the slack."""
    rows_p, cols_p = ((n1 + 127) // 128 * 128, (n2 + 127) // 128 * 128) if grid else (n1, n2)
    nlev = 4
    Ks, Kn = R.exact_ints((n1, n2), 1), R.exact_ints((n1, n2), 2)
    s1, s2, ntab = R.exact_ints(n1, 3), R.exact_ints(n2, 4), R.exact_ints(nlev, 5)
    rng = np.random.default_rng(6)
    l1, l2 = rng.integers(0, nlev, n1), rng.integers(0, nlev, n2)
    ref = np.zeros((rows_p, cols_p), np.int64)
    if diag != 0.0:
        k = min(rows_p, cols_p)
        ref[np.arange(k), np.arange(k)] = 1
    core = (s1[:, None] * s2[None, :] if with_s else 1) * Ks + ntab[np.minimum(l1[:, None], l2[None, :])] * Kn
    k = min(n1, n2)
    core[np.arange(k), np.arange(k)] += int(diag)
    ref[:n1, :n2] = core
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt).to(DEV)
    A, B = R.Strided(n1, n2, pad=3, fill=Ks), R.Strided(n1, n2, pad=3, fill=Kn)
    out = R.Strided(rows_p + 2, cols_p, pad=5)          # two more rows than the call is told of
    R.mf_combine(A, B, t(s1) if with_s else None, t(s2) if with_s else None, t(l1, torch.int32), t(l2, torch.int32), t(ntab),
                 diag, out, n1, n2, rows_p, cols_p)
    torch.cuda.synchronize()
    assert torch.equal(out.view[:rows_p], t(ref))
    assert out.slack_untouched() and bool(torch.isnan(out.full[rows_p:]).all())
    assert A.slack_untouched() and B.slack_untouched()
