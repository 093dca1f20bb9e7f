"""Greedy conditional-variance selection of inducing points, the parts that need no GPU: the numpy statement of the rules
(``greedy_oracle``, imported by test_hip_inducing_select), that oracle against LAPACK's pivoted Cholesky (dpstrf), and the
surface -- the MFDGP arguments, the no-CPU-fallback error, the exported symbols and their host-side refusals."""
import ctypes

import numpy as np
import pytest
import torch

from mobocmf_amd.util import synthetic
from tests.helpers import to_t

EPS = np.finfo(np.float64).eps


def ard_rbf(x, ls, a):
    xs = np.asarray(x, dtype=np.float64) / np.asarray(ls, dtype=np.float64)
    d2 = ((xs[:, None, :] - xs[None, :, :]) ** 2).sum(-1)
    return a * np.exp(-0.5 * d2)


def greedy_oracle(x, ls, a, max_points, tol_rel=0.0):
    """The selection rules of mobocmf_select_inducing in numpy.  Step j picks the largest residual (np.argmax: the lowest row
    among equal ones), stops before a pick whose residual is <= tol_rel * a or not positive, forms the column
    l = (k(X, x_p) - L[:, :j] L[p, :j]^T) / sqrt(d_p) with l_p = sqrt(d_p), and updates d = max(d - l*l, 0), d_p = 0.
    Returns (idx [count], resid [count], diag [N], gaps [count]): gaps[j] is the distance between the two largest residuals
    when pick j was made (0 at step 0, where all are equal)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    xs = x / np.asarray(ls, dtype=np.float64)
    d = np.full(N, float(a))
    L = np.zeros((max_points, N))
    idx, resid, gaps = [], [], []
    for j in range(max_points):
        p = int(np.argmax(d))
        dp = d[p]
        if not dp > max(tol_rel * a, 0.0):
            break
        gaps.append(dp - np.partition(d, -2)[-2] if N > 1 else np.inf)
        idx.append(p)
        resid.append(dp)
        k = a * np.exp(-0.5 * ((xs - xs[p]) ** 2).sum(1))
        l = (k - L[:j].T @ L[:j, p]) / np.sqrt(dp)
        l[p] = np.sqrt(dp)
        d = np.maximum(d - l * l, 0.0)
        d[p] = 0.0
        L[j] = l
    return np.array(idx, dtype=np.int64), np.array(resid), d, np.array(gaps)


def uniform_rows(N, d, seed=0):
    return np.random.default_rng(seed).random((N, d))


def bo_like_rows():
    """64 uniform rows (an initial design), then 192 rows clustered on a curve (acquisitions closing in on a front)."""
    rng = np.random.default_rng(0)
    t = rng.random(192)
    curve = np.stack([t, 0.5 + 0.4 * np.sin(3.0 * t)], 1) + 0.01 * rng.standard_normal((192, 2))
    return np.concatenate([rng.random((64, 2)), curve], 0)


def nested_rows():
    """100 rows evaluated at two fidelities (every row twice, exactly) and 200 more rows."""
    rng = np.random.default_rng(0)
    base = rng.random((100, 2))
    return np.concatenate([base, base, rng.random((200, 2))], 0)


# ------------------------------------------------------------------ the oracle against LAPACK
@pytest.mark.parametrize("d,N,M,ls", [(2, 512, 128, 0.2), (8, 2048, 256, np.sqrt(8.0) / 2)])
def test_oracle_picks_equal_lapack_pivots(d, N, M, ls):
    from scipy.linalg.lapack import dpstrf
    x = uniform_rows(N, d)
    idx, resid, diag, gaps = greedy_oracle(x, np.full(d, ls), 1.0, M)
    _, piv, rank, _ = dpstrf(ard_rbf(x, np.full(d, ls), 1.0), lower=1)
    assert rank >= M and len(idx) == M
    assert np.array_equal(piv[:M] - 1, idx)
    assert np.all(np.diff(resid) <= M * M * EPS) and diag.max() <= resid[-1] and np.all(diag[idx] == 0.0)


def test_oracle_stop_rule_equals_lapack_rank():
    from scipy.linalg.lapack import dpstrf
    x = uniform_rows(512, 2)
    ls = np.full(2, np.sqrt(2.0) / 2)
    idx, resid, diag, _ = greedy_oracle(x, ls, 1.0, 128, tol_rel=1e-8)
    _, piv, rank, _ = dpstrf(ard_rbf(x, ls, 1.0), tol=1e-8, lower=1)
    assert len(idx) == 36 and rank == 36
    assert np.array_equal(piv[:36] - 1, idx)
    assert resid[-1] > 1e-8 >= diag.max()            # 1.96e-8 before the stop, 7.7e-9 after


def test_oracle_on_duplicate_rows_never_picks_both_of_a_pair():
    idx, resid, diag, _ = greedy_oracle(nested_rows(), np.full(2, 0.2), 1.0, 128)
    picked = set(idx.tolist())
    assert len(picked) == len(idx)
    assert not any(i in picked and i + 100 in picked for i in range(100))


def test_oracle_reaches_the_late_rows_of_a_bo_like_design():
    idx, _, _, _ = greedy_oracle(bo_like_rows(), np.full(2, 0.15), 1.0, 64)
    assert int((idx >= 64).sum()) >= 1               # x_train[:64] holds none of the clustered rows


# ------------------------------------------------------------------ surface
def _forrester(**kw):
    from mobocmf_amd.models import MFDGP
    x, y, fid = synthetic.forrester_problem(0)
    torch.manual_seed(0)
    return MFDGP(to_t(x), to_t(y)[:, None], to_t(fid)[:, None], 2, **kw)


def test_selection_first_is_the_default_model_bitwise():
    a = _forrester(num_inducing=6)
    b = _forrester(num_inducing=6, inducing_selection="first", inducing_tol=0.0)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.hidden_layer_0.variational_strategy.inducing_points,
                       b.hidden_layer_0.variational_strategy.inducing_points)
    assert b.inducing_selection == "first" and b.inducing_indices is None
    with pytest.raises(ValueError):
        _forrester(num_inducing=6, inducing_selection="kmeans")


def test_greedy_selection_has_no_cpu_fallback():
    from mobocmf_amd import _lib
    with pytest.raises(_lib.MobocmfError, match="no CPU fallback"):
        _forrester(num_inducing=6, inducing_selection="greedy_variance")
    with pytest.raises(_lib.MobocmfError, match="no CPU fallback"):
        _forrester(num_inducing=6, inducing_selection="greedy_variance", inducing_device="cpu")


def test_explicit_inducing_points_ignore_the_selection_arguments():
    x, _, _ = synthetic.forrester_problem(0)
    Z = to_t(x)[[7, 2, 5]]
    m = _forrester(inducing_points=Z, num_inducing=6, inducing_selection="greedy_variance", inducing_tol=1e-3)
    assert torch.equal(m.hidden_layer_0.variational_strategy.inducing_points, Z) and m.inducing_indices is None


def test_library_refuses_bad_shapes_before_touching_a_gpu():
    from mobocmf_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "mobocmf_select_inducing") and hasattr(lib, "mobocmf_select_inducing_workspace_bytes")
    nb = ctypes.c_size_t()
    assert lib.mobocmf_select_inducing_workspace_bytes(512, 128, ctypes.byref(nb)) == _lib.OK
    assert nb.value >= 512 * 128 * 8
    big = ctypes.c_size_t()
    assert lib.mobocmf_select_inducing_workspace_bytes(8192, 512, ctypes.byref(big)) == _lib.OK
    assert 32 * 2 ** 20 <= big.value < 33 * 2 ** 20                  # the factor, [max_points][N] doubles
    assert lib.mobocmf_select_inducing_workspace_bytes(0, 1, ctypes.byref(nb)) == _lib.BAD_ARG          # N < 1
    assert lib.mobocmf_select_inducing_workspace_bytes(16, 17, ctypes.byref(nb)) == _lib.BAD_ARG        # max_points > N
    assert lib.mobocmf_select_inducing_workspace_bytes(16, 4, None) == _lib.BAD_ARG
    # never dereferenced: every call below is refused on the host
    p = ctypes.c_void_p(4096)

    def call(N=512, d=2, x=p, hyp=p, M=128, tol=0.0, form=0, idx=p, ws=p, ws_bytes=None):
        ws_bytes = nb512 if ws_bytes is None else ws_bytes
        return lib.mobocmf_select_inducing(N, d, x, hyp, M, tol, form, idx, p, p, p, p, ws, ws_bytes, None)

    nb512 = 32768 + 512 * 128 * 8
    assert call(N=0) == _lib.BAD_ARG
    assert call(N=-5) == _lib.BAD_ARG
    assert call(M=513) == _lib.BAD_ARG
    assert call(M=0) == _lib.BAD_ARG
    assert call(x=None) == _lib.BAD_ARG
    assert call(hyp=None) == _lib.BAD_ARG
    assert call(idx=None) == _lib.BAD_ARG
    assert call(ws=None) == _lib.BAD_ARG
    assert call(ws_bytes=512 * 128 * 8) == _lib.BAD_ARG                # short by the header
    assert call(d=0) == _lib.BAD_ARG and call(d=33) == _lib.BAD_ARG
    assert call(tol=float("nan")) == _lib.BAD_ARG and call(tol=-1.0) == _lib.BAD_ARG
    assert call(form=3) == _lib.BAD_ARG
    # one workgroup over more than INDUCING_ONE_WG_MAX_ROWS rows is refused; the other forms take them up to INDUCING_MAX_ROWS
    big_n = _lib.INDUCING_ONE_WG_MAX_ROWS + 1
    assert call(N=big_n, M=4, form=1, ws_bytes=32768 + big_n * 4 * 8) == _lib.BAD_ARG
    assert lib.mobocmf_select_inducing_workspace_bytes(_lib.INDUCING_MAX_ROWS, 4, ctypes.byref(nb)) == _lib.OK
    assert lib.mobocmf_select_inducing_workspace_bytes(_lib.INDUCING_MAX_ROWS + 1, 4, ctypes.byref(nb)) == _lib.BAD_ARG

