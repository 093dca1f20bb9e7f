"""Natural-gradient update of q(u), without a GPU: the tests' own restatement (tests/natgrad_reference.py) against the closed-form
optimum of a conjugate problem, and the argument checks of the C-ABI, which refuse on the host before any HIP call."""
import ctypes

import torch

from tests import natgrad_reference as R


def test_restatement_hits_the_conjugate_optimum_in_one_step():
    """One step of length gamma = 1 on a one-layer conjugate problem (M = 12, N = 40, d = 2) lands on
    S* = (K^-1 + K^-1 K_mn K_nm K^-1 / s2)^-1, m* = S* K^-1 K_mn y / s2 from any start; with gamma = 0.5 the natural parameters
    contract by 1/2 per step.  This pins the reference the GPU tests compare against."""
    Kmm, Kmn, knn, y, noise = R.conjugate_problem(M=12, N=40, d=2, seed=0)
    m_opt, S_opt, Lam_opt = R.conjugate_optimum(Kmm, Kmn, y, noise)
    g = torch.Generator().manual_seed(1)
    M = 12
    m0 = torch.randn(M, dtype=torch.float64, generator=g)
    L0 = 0.5 * torch.eye(M, dtype=torch.float64) + 0.1 / M ** 0.5 * torch.tril(torch.randn(M, M, dtype=torch.float64, generator=g))
    L0[2, 2] = -L0[2, 2]      # the sign of a diagonal entry is free in S = L L^T and must survive the step
    L0 = L0 + torch.triu(torch.randn(M, M, dtype=torch.float64, generator=g), 1)      # never read

    def grads(m, L):
        m, L = m.clone().requires_grad_(True), L.clone().requires_grad_(True)
        R.conjugate_neg_elbo(m, L, Kmm, Kmn, knn, y, noise).backward()
        return m.grad, L.grad

    gm, gL = grads(m0, L0)
    m1, L1, B, ok = R.natgrad_update(m0, L0, gm, gL, 1.0)
    assert ok and bool((torch.triu(L1, 1) == 0).all())
    assert bool((torch.sign(torch.diagonal(L1)) == torch.sign(torch.diagonal(L0))).all())
    S1 = L1 @ L1.T
    err_S = float((S1 - S_opt).abs().max() / S_opt.abs().max())
    err_m = float((m1 - m_opt).abs().max() / m_opt.abs().max())
    print("one step, gamma = 1: rel err S %.3e, m %.3e, cond(B) %.3e" % (err_S, err_m, float(torch.linalg.cond(B))))
    assert err_S < 1e-8 and err_m < 1e-8
    # gamma = 0.5: Lambda_t = Lambda* + 0.5^t (Lambda_0 - Lambda*), and the same for Lambda_t m_t
    m, L = m0, L0
    S0 = torch.tril(L0) @ torch.tril(L0).T
    Lam0, th0, th_opt = torch.linalg.inv(S0), torch.linalg.solve(S0, m0), Lam_opt @ m_opt
    for t in range(1, 6):
        gm, gL = grads(m, L)
        m, L, _, ok = R.natgrad_update(m, L, gm, gL, 0.5)
        assert ok
        S = L @ L.T
        want_Lam = Lam_opt + 0.5 ** t * (Lam0 - Lam_opt)
        want_th = th_opt + 0.5 ** t * (th0 - th_opt)
        assert float((torch.linalg.inv(S) - want_Lam).abs().max() / want_Lam.abs().max()) < 1e-8
        assert float((torch.linalg.solve(S, m) - want_th).abs().max() / want_th.abs().max()) < 1e-8


def test_restatement_leaves_a_non_pd_step_alone_and_schedule_endpoints():
    M = 5
    L = torch.eye(M, dtype=torch.float64)
    m = torch.ones(M, dtype=torch.float64)
    m1, L1, B, ok = R.natgrad_update(m, L, m, -2.0 * L, 1.0)      # Psi = -I: B = -I
    assert not ok and torch.equal(m1, m) and torch.equal(L1, L) and torch.allclose(B, -torch.eye(M, dtype=torch.float64))
    assert R.gamma_at(0, 0.1, 1e-4, 100) == 1e-4 and R.gamma_at(100, 0.1, 1e-4, 100) == 0.1
    assert R.gamma_at(101, 0.1, 1e-4, 100) == 0.1 and R.gamma_at(3, 0.1, 1e-4, 0) == 0.1
    assert abs(R.gamma_at(50, 0.1, 1e-4, 100) / (1e-4 * 1000 ** 0.5) - 1) < 1e-15


def _step_args(lib, n=1, M=8, gamma=0.1, gamma_init=1e-4, warmup=100, scale=1.0, bytes_=None, null=None):
    """A call whose pointers are never dereferenced on the host: fake non-NULL device addresses (refused calls launch nothing)."""
    fake = 4096
    tab = lambda: (ctypes.c_void_p * n)(*([fake] * n))
    nb = ctypes.c_size_t()
    from mobocmf_amd import _lib
    if lib.mobocmf_natgrad_workspace_bytes(M, n, ctypes.byref(nb)) != _lib.OK:
        nb.value = 1 << 20
    args = [n, M, tab(), tab(), tab(), tab(), gamma, gamma_init, warmup, scale, ctypes.c_void_p(fake), tab(), tab(),
            ctypes.c_void_p(fake), nb.value if bytes_ is None else bytes_, None, None]
    if null is not None:
        if isinstance(null, tuple):      # one NULL entry inside a table
            args[null[0]][null[1]] = None
        else:
            args[null] = None
    return args


def test_natgrad_arguments_are_validated_on_the_host():
    from mobocmf_amd import _lib
    lib = _lib.load()
    step = lib.mobocmf_natgrad_step
    # every refusal of the header, none of which reaches a HIP call (this machine may have no GPU at all)
    for null in (2, 3, 4, 5, 10, 11, 12, 13, (2, 0), (3, 0), (4, 0), (5, 0), (11, 0), (12, 0)):
        assert step(*_step_args(lib, null=null)) == _lib.BAD_ARG, null
    for kw in (dict(M=0), dict(M=-3), dict(M=_lib.NATGRAD_MAX_M + 1), dict(n=0), dict(n=_lib.NATGRAD_MAX_LAYERS + 1),
               dict(gamma=0.0), dict(gamma=-0.1), dict(gamma=float("nan")), dict(gamma_init=0.2, gamma=0.1), dict(warmup=-1),
               dict(gamma_init=0.0), dict(scale=0.0)):
        assert step(*_step_args(lib, **kw)) == _lib.BAD_ARG, kw
    bad_tuning = _lib.Tuning()
    lib.mobocmf_tuning_init(ctypes.byref(bad_tuning))
    bad_tuning.potrf_cols = 3
    args = _step_args(lib)
    args[15] = ctypes.byref(bad_tuning)
    assert step(*args) == _lib.BAD_ARG
    nb = ctypes.c_size_t()
    assert lib.mobocmf_natgrad_workspace_bytes(8, 1, ctypes.byref(nb)) == _lib.OK
    assert step(*_step_args(lib, bytes_=nb.value - 1)) == _lib.WORKSPACE_TOO_SMALL
    assert step(*_step_args(lib, n=3, bytes_=3 * nb.value - 256)) == _lib.WORKSPACE_TOO_SMALL
    # the size query: refusals, growth with M (in steps of the 128-padding) and proportional to n
    assert lib.mobocmf_natgrad_workspace_bytes(8, 1, None) == _lib.BAD_ARG
    for M, n in ((0, 1), (_lib.NATGRAD_MAX_M + 1, 1), (8, 0), (8, 5)):
        assert lib.mobocmf_natgrad_workspace_bytes(M, n, ctypes.byref(nb)) == _lib.BAD_ARG, (M, n)
    size = {}
    for M in (1, 128, 129, 256, 700, 1024):
        for n in (1, 2, 4):
            assert lib.mobocmf_natgrad_workspace_bytes(M, n, ctypes.byref(nb)) == _lib.OK
            size[(M, n)] = nb.value
        assert size[(M, 2)] == 2 * size[(M, 1)] and size[(M, 4)] == 4 * size[(M, 1)] and size[(M, 1)] % 256 == 0
    assert size[(1, 1)] == size[(128, 1)] < size[(129, 1)] == size[(256, 1)] < size[(700, 1)] < size[(1024, 1)]
    assert size[(1024, 1)] >= 10 * 1024 * 1024 * 8      # the M x M operands of the sequence


def test_natgrad_has_no_cpu_path_and_unknown_optimisers_are_refused():
    """'natgrad' on CPU tensors, on a row-sharded step and an unknown name raise ValueError; the wrapper refuses CPU tensors."""
    import pytest
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as F
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.parallel import RowShardedELBOStep
    from mobocmf_amd.util import synthetic
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    from mobocmf_amd.util.graphed_step import GraphedELBOStep
    from tests.helpers import to_t
    prob = synthetic.make_problem(d=2, L=2, M=8, N=12, S=3, seed=0)
    model = synthetic.model_from_problem(prob, device="cpu")
    x, y, fid = to_t(prob["x"]), to_t(prob["y"])[:, None], to_t(prob["fid"])[:, None]
    elbo = VariationalELBOMF(model, 12, 2)
    with pytest.raises(ValueError, match="GPU only"):
        GraphedELBOStep(model, elbo, x, y, fid, lr=1e-2, use_graph=False, variational_optimizer="natgrad")
    with pytest.raises(ValueError, match="row-sharded"):
        RowShardedELBOStep(model, elbo, x, y, fid, lr=1e-2, use_graph=False, variational_optimizer="natgrad")
    with pytest.raises(ValueError, match="'adam' or 'natgrad'"):
        BlackBoxMFDGPFitter(2, 12, variational_optimizer="newton")
    fitter = BlackBoxMFDGPFitter(2, 12, num_epochs_1=1, num_epochs_2=1, device="cpu", variational_optimizer="natgrad")
    fitter.initialize_mfdgp(x, y, fid, "f0")
    with pytest.raises(ValueError, match="use_graphs=False"):
        fitter.train_mfdgps(use_graphs=False)
    with pytest.raises(ValueError, match="use_graphs=False"):
        fitter.train_mfdgps()      # CPU tensors: the default is the host loader
    with pytest.raises(ValueError):
        F.FusedNatGradAdam(model, lr=1e-2)
    z = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(_lib.MobocmfError):
        F.natgrad_step([z], [torch.eye(8, dtype=torch.float64)], [z], [torch.eye(8, dtype=torch.float64)], 0.1, 1e-4, 100, 1.0,
                       torch.zeros((), dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


def test_run_verified_prints_when_the_skip_count_has_grown(capsys):
    """The training loop reports skipped natural-gradient steps at its verification cadence, from what check() read."""
    from mobocmf_amd.util.blackbox_mfdgp_fitter import REDO_EAGERLY, run_verified

    class Step:
        skipped = [0, 0]
        n = 0

        def step(self):
            self.n += 1

        def check(self):
            self.skipped = [1, 2] if self.n >= 2 else [0, 0]

        def snapshot(self):
            pass

        def close(self):
            pass

    assert run_verified([Step()], 3, REDO_EAGERLY, ["toy: "], "epochs") == (3, None)
    out = capsys.readouterr().out
    assert out.count("natural-gradient steps skipped") == 1 and "toy: 3 natural-gradient steps skipped so far" in out
