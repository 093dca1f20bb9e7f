"""mobocmf_natgrad_step on the GPU against the float64 restatement of tests/natgrad_reference.py: the update itself over the
sizes where the launch sequence changes path, the gamma schedule evaluated on the device, and the rule for a step whose
I + 2 gamma Psi is not positive definite."""
import pytest
import torch

from tests import natgrad_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -52


def _layer_inputs(M, seed, c=20.0):
    """L_S = 0.5 I + (0.1 / sqrt(M)) tril(randn) with two diagonal entries negated and a random (never read) upper triangle;
    g_LS = tril(2 G L_S) for the PSD G = c R R^T / M, so that B = I + 2 gamma L_S^T G L_S is PD for every gamma; random g_m, m."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    L = 0.5 * torch.eye(M, dtype=torch.float64) + 0.1 / M ** 0.5 * torch.tril(rn(M, M))
    L[1, 1], L[M - 2, M - 2] = -L[1, 1], -L[M - 2, M - 2]
    stored = L + torch.triu(rn(M, M), 1)
    Rm = rn(M, M)
    G = c * Rm @ Rm.T / M
    return rn(M), stored, rn(M), torch.tril(2.0 * G @ L)


def _relerr(a, b):
    return float((a.cpu() - b).abs().max() / b.abs().max())


def _call(ms, Ls, gms, gLs, gamma, gamma_init, warmup, scale, step, skipped, info):
    from mobocmf_amd import functional as F
    F.natgrad_step(ms, Ls, gms, gLs, gamma, gamma_init, warmup, scale, step, skipped, info)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("M", [8, 70, 130])
def test_kernel_matches_the_restatement(M, n):
    """M = 8: one partial tile; 70: crosses the 64-wide panel, no multiple of 16; 130: padded to 256, three 64-blocks (the one-launch
    Cholesky's range), reversal of M differs from reversal of Mp.  Relative error of L_new (lower, signs kept), L_new L_new^T and
    m_new within 50 M eps cond_2(B) -- the forward-error form of a Cholesky solve -- with cond_2(B) from the restatement's B."""
    gamma, scale = 0.7, 3.0
    cpu = [_layer_inputs(M, 100 * M + z) for z in range(n)]
    refs = [R.natgrad_update(m, L, gm, gL, gamma, scale) for m, L, gm, gL in cpu]
    runs = []
    for _ in range(2):
        ms = [t[0].to(DEV) for t in cpu]
        Ls = [t[1].to(DEV) for t in cpu]
        step = torch.zeros((), dtype=torch.int64, device=DEV)
        skipped, info = torch.zeros(n, dtype=torch.int32, device=DEV), torch.full((n,), 7, dtype=torch.int32, device=DEV)
        _call(ms, Ls, [t[2].to(DEV) for t in cpu], [t[3].to(DEV) for t in cpu], gamma, 1e-4, 0, scale, step, skipped, info)
        assert int(step) == 1 and skipped.tolist() == [0] * n and info.tolist() == [0] * n
        runs.append((ms, Ls))
    for z, ((m0, L0, _, _), (m_ref, L_ref, B, ok)) in enumerate(zip(cpu, refs)):
        assert ok
        cond = float(torch.linalg.cond(B))
        assert cond < 1e3
        tol = 50 * M * EPS * cond
        m_new, L_st = runs[0][0][z].cpu(), runs[0][1][z].cpu()
        assert torch.equal(torch.triu(L_st, 1), torch.triu(L0, 1))                    # the upper triangle is never written
        L_new = torch.tril(L_st)
        errs = (_relerr(L_new, L_ref), _relerr(L_new @ L_new.T, L_ref @ L_ref.T), _relerr(m_new, m_ref))
        print("M %d n %d layer %d: cond(B) %.3g, tol %.3g, rel err L %.3g S %.3g m %.3g" % ((M, n, z, cond, tol) + errs))
        assert max(errs) <= tol, errs
        assert bool((torch.sign(torch.diagonal(L_new)) == torch.sign(torch.diagonal(L0))).all())
        assert torch.equal(runs[1][0][z].cpu(), m_new) and torch.equal(runs[1][1][z].cpu(), L_st)      # bitwise reproducible


def test_gamma_schedule_is_evaluated_on_the_device():
    """gamma_t = min(gamma, gamma_init rho^t) after t = 0, 1, 50, 100, 101 calls, to 1e-14 relative.  With L_S = I and
    g_LS = 2 s I (G = s I) B = (1 + 2 gamma_t s) I, so L_new = I / sqrt(1 + 2 gamma_t s); s = 2^20 makes 2 gamma_t s >> 1 and the
    recovery gamma_t = (1 / L_new[0][0]^2 - 1) / (2 s) loses no digits."""
    M, s = 8, 2.0 ** 20
    gamma, gamma_init, warmup = 0.1, 1e-4, 100
    eye = torch.eye(M, dtype=torch.float64, device=DEV)
    gL, gm = 2.0 * s * eye, torch.zeros(M, dtype=torch.float64, device=DEV)
    step = torch.zeros((), dtype=torch.int64, device=DEV)
    skipped, info = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    from mobocmf_amd import functional as F
    seen = {}
    for t in range(102):
        L, m = eye.clone(), gm.clone()
        F.natgrad_step([m], [L], [gm], [gL], gamma, gamma_init, warmup, 1.0, step, skipped, info)
        if t in (0, 1, 50, 100, 101):
            assert int(step) == t + 1
            seen[t] = (1.0 / float(L[0, 0]) ** 2 - 1.0) / (2.0 * s)
            assert float((L - L[0, 0] * eye).abs().max()) == 0.0
    assert skipped.tolist() == [0]
    for t, got in seen.items():
        want = R.gamma_at(t, gamma, gamma_init, warmup)
        print("t %d: gamma_t %.17g, formula %.17g, rel %.2e" % (t, got, want, abs(got / want - 1)))
        assert abs(got / want - 1) < 1e-14, t
    # warmup_steps = 0: gamma from the first call
    L, step0 = eye.clone(), torch.zeros((), dtype=torch.int64, device=DEV)
    _call([gm.clone()], [L], [gm], [gL], gamma, gamma_init, 0, 1.0, step0, skipped, info)
    assert abs((1.0 / float(L[0, 0]) ** 2 - 1.0) / (2.0 * s) / gamma - 1) < 1e-14


@pytest.mark.parametrize("M", [8, 70])
def test_a_non_pd_step_is_skipped_and_counted(M):
    """Layer 0 has Psi = -I (L_S = I, g_LS = -2 I) and gamma = 1: B = -I, the factorisation reports pivot 1 -- a report, not a
    fault.  Its m and L_S stay bitwise, skipped counts the step, the other layer of the call is updated, the counter advances, and
    the next call (PD again) succeeds."""
    g = torch.Generator().manual_seed(5)
    eye = torch.eye(M, dtype=torch.float64)
    m0 = torch.randn(M, dtype=torch.float64, generator=g)
    L0 = eye + torch.triu(torch.randn(M, M, dtype=torch.float64, generator=g), 1)
    gm0 = torch.randn(M, dtype=torch.float64, generator=g)
    m1, L1, gm1, gL1 = _layer_inputs(M, 77)
    m1_ref, L1_ref, B1, _ = R.natgrad_update(m1, L1, gm1, gL1, 1.0)
    ms, Ls = [m0.to(DEV), m1.to(DEV)], [L0.to(DEV), L1.to(DEV)]
    step = torch.zeros((), dtype=torch.int64, device=DEV)
    skipped, info = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    _call(ms, Ls, [gm0.to(DEV), gm1.to(DEV)], [(-2.0 * eye).to(DEV), gL1.to(DEV)], 1.0, 1.0, 0, 1.0, step, skipped, info)
    assert torch.equal(ms[0].cpu(), m0) and torch.equal(Ls[0].cpu(), L0)
    assert skipped.tolist() == [1, 0] and int(info[0]) > 0 and int(info[1]) == 0 and int(step) == 1
    tol = 50 * M * EPS * float(torch.linalg.cond(B1))
    assert _relerr(torch.tril(Ls[1].cpu()), L1_ref) <= tol and _relerr(ms[1].cpu(), m1_ref) <= tol
    # the next call: layer 0 with Psi = +I -> B = 3 I
    m0_ref, L0_ref, _, ok = R.natgrad_update(m0, L0, gm0, 2.0 * eye, 1.0)
    assert ok
    ms[1].copy_(m1)      # (g_LS of layer 1 was built for its first L_S: B is PD for that one)
    Ls[1].copy_(L1)
    _call(ms, Ls, [gm0.to(DEV), gm1.to(DEV)], [(2.0 * eye).to(DEV), gL1.to(DEV)], 1.0, 1.0, 0, 1.0, step, skipped, info)
    assert skipped.tolist() == [1, 0] and info.tolist() == [0, 0] and int(step) == 2
    assert _relerr(torch.tril(Ls[0].cpu()), L0_ref) <= 50 * M * EPS and _relerr(ms[0].cpu(), m0_ref) <= 50 * M * EPS      # cond(3 I) = 1
    assert torch.equal(torch.triu(Ls[0].cpu(), 1), torch.triu(L0, 1))
