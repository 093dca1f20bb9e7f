"""mobocmf_natgrad_small_step -- the natural-gradient update of small layers (M <= 128), one workgroup per layer, every layer of
a launch free to have its own M -- against the float64 restatement of tests/natgrad_reference.py: both size families and their
boundary, a mixed launch, the memory contract, the per-layer gamma schedule, the skip rule, the guard and argument validation."""
import ctypes

import pytest
import torch

from tests import natgrad_reference as R
from tests.test_hip_natgrad import _layer_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -52
NAN = float("nan")


def _relerr(a, b):
    return float((a.cpu() - b).abs().max() / b.abs().max())


def _poisoned(t):
    """The strict upper triangle replaced by NaN: a value read from it shows in every result."""
    M = t.shape[0]
    iu = torch.triu_indices(M, M, 1)
    t = t.clone()
    t[iu[0], iu[1]] = NAN
    return t


def _records(cpu, scales, **extra):
    """Device copies of the layers (m, L_S, g_m, g_LS) with NaN above the diagonals of L_S and g_LS."""
    recs = []
    for z, ((m, L, gm, gL), sc) in enumerate(zip(cpu, scales)):
        rec = dict(m=m.to(DEV), L_S=_poisoned(L).to(DEV), g_m=gm.to(DEV), g_LS=_poisoned(gL).to(DEV), scale=sc)
        rec.update({k: v[z] for k, v in extra.items()})
        recs.append(rec)
    return recs


def _run(recs, gamma, gamma_init=None, warmup=0):
    from mobocmf_amd import functional as F
    table = F.natgrad_small_step(recs, gamma, gamma if gamma_init is None else gamma_init, warmup)
    torch.cuda.synchronize()
    return table


def _bits(t):
    return t.cpu().contiguous().view(torch.int64)


_REF = {}


def _reference(M, seed, gamma, scale):
    """The restatement's answer for _layer_inputs(M, seed), computed once per case and left unchanged."""
    key = (M, seed, gamma, scale)
    if key not in _REF:
        cpu = _layer_inputs(M, seed)
        m_ref, L_ref, B, ok = R.natgrad_update(*cpu, gamma, scale)
        _REF[key] = (cpu, m_ref, L_ref, float(torch.linalg.cond(B)), ok)
    return _REF[key]


def _assert_matches(M, cpu, rec, m_ref, L_ref, cond, ok, what):
    assert ok and cond < 1e3, (what, cond)
    tol = 50 * M * EPS * cond
    L0 = cpu[1]
    L_st, m_new = rec["L_S"].cpu(), rec["m"].cpu()
    iu = torch.triu_indices(M, M, 1)
    assert torch.equal(_bits(L_st[iu[0], iu[1]]), _bits(_poisoned(L0)[iu[0], iu[1]]))      # the upper triangle: bitwise unchanged ...
    L_new = torch.tril(L_st)
    assert bool(torch.isfinite(L_new).all()) and bool(torch.isfinite(m_new).all())    # ... and never read (it holds NaN)
    errs = (_relerr(L_new, L_ref), _relerr(L_new @ L_new.T, L_ref @ L_ref.T), _relerr(m_new, m_ref))
    print("%s M %d: cond(B) %.3g, tol %.3g, rel err L %.3g S %.3g m %.3g" % ((what, M, cond, tol) + errs))
    assert max(errs) <= tol, (what, errs, tol)
    assert bool((torch.sign(torch.diagonal(L_new)) == torch.sign(torch.diagonal(L0))).all())


@pytest.mark.parametrize("M", [8, 16, 17, 32, 33, 70, 128])
def test_one_layer_matches_the_restatement(M):
    """8: one partial 16-tile; 16: exactly one tile; 17: one tile + 1; 32: the top of the plain-FMA family; 33: the first size on
    the MFMA tiles; 70: no multiple of 16; 128: the limit and the LDS budget.  gamma = 0.7, scale = 3, no warm-up, seeds 100 M +
    {0, 1, 2}.  Relative error of L_new, L_new L_new^T and m_new within 50 M eps cond_2(B) (the bound of test_hip_natgrad.py); the
    stored upper triangle is bitwise untouched and, like the one of g_LS, holds NaN that must not reach a result; diagonal signs
    kept; counters 1, skipped 0, info 0; a second run is bitwise equal."""
    gamma, scale = 0.7, 3.0
    for z in range(3):
        cpu, m_ref, L_ref, cond, ok = _reference(M, 100 * M + z, gamma, scale)
        runs = []
        for _ in range(2):
            recs = _records([cpu], [scale])
            table = _run(recs, gamma)
            assert table.natgrad_steps.tolist() == [1] and table.skipped.tolist() == [0] and table.info.tolist() == [0]
            runs.append(recs[0])
        _assert_matches(M, cpu, runs[0], m_ref, L_ref, cond, ok, "seed %d" % (100 * M + z))
        assert torch.equal(_bits(runs[0]["m"]), _bits(runs[1]["m"])) and torch.equal(_bits(runs[0]["L_S"]), _bits(runs[1]["L_S"]))


def test_mixed_launch_runs_both_families_with_a_scale_and_a_counter_per_layer():
    Ms, scales, gamma = [8, 33, 128, 17, 32], [3.0, 1.0, 2.0, 0.5, 4.0], 0.7
    refs = [_reference(M, 100 * M, gamma, sc) for M, sc in zip(Ms, scales)]
    recs = _records([r[0] for r in refs], scales)
    table = _run(recs, gamma)
    assert table.natgrad_steps.tolist() == [1] * 5 and table.skipped.tolist() == [0] * 5 and table.info.tolist() == [0] * 5
    for M, rec, (cpu, m_ref, L_ref, cond, ok) in zip(Ms, recs, refs):
        _assert_matches(M, cpu, rec, m_ref, L_ref, cond, ok, "mixed")


def test_gamma_schedule_is_evaluated_per_layer_on_the_device():
    """gamma_t at t = 0, 1, 50, 100, 101 with 1e-4 -> 0.1 over 100 steps, to 1e-14 relative, from per-layer counters preset to those
    t in ONE launch (M = 8 and M = 40 alternating).  With L_S = I and g_LS = 2 s I, B = (1 + 2 gamma_t s) I and L_new = I /
    sqrt(1 + 2 gamma_t s); s = 2^20 makes 2 gamma_t s >> 1, so gamma_t = (1 / L_new[0][0]^2 - 1) / (2 s) loses no digits."""
    s, ts = 2.0 ** 20, [0, 1, 50, 100, 101]
    gamma, gamma_init, warmup = 0.1, 1e-4, 100
    steps = torch.tensor(ts, dtype=torch.int64, device=DEV)
    recs = []
    for z, t in enumerate(ts):
        M = 8 if z % 2 == 0 else 40
        eye = torch.eye(M, dtype=torch.float64, device=DEV)
        recs.append(dict(m=torch.zeros(M, dtype=torch.float64, device=DEV), L_S=eye.clone(),
                         g_m=torch.zeros(M, dtype=torch.float64, device=DEV), g_LS=2.0 * s * eye, step_count=steps[z:z + 1]))
    table = _run(recs, gamma, gamma_init, warmup)
    assert steps.tolist() == [t + 1 for t in ts] and table.skipped.tolist() == [0] * 5
    for t, rec in zip(ts, recs):
        L = rec["L_S"]
        assert float((L - L[0, 0] * torch.eye(L.shape[0], dtype=torch.float64, device=DEV)).abs().max()) == 0.0
        got, want = (1.0 / float(L[0, 0]) ** 2 - 1.0) / (2.0 * s), R.gamma_at(t, gamma, gamma_init, warmup)
        print("t %d: gamma_t %.17g, formula %.17g, rel %.2e" % (t, got, want, abs(got / want - 1)))
        assert abs(got / want - 1) < 1e-14, t


@pytest.mark.parametrize("M", [8, 70])
def test_a_non_pd_step_is_skipped_and_counted(M):
    """Layer 0 has Psi = -I (L_S = I, g_LS = -2 I) and gamma = 1: B = -I, the factorisation reports a pivot -- a report, not a
    fault.  Its m and L_S stay bitwise, skipped counts the step, its counter advances; the healthy layer of the launch is updated."""
    g = torch.Generator().manual_seed(5)
    eye = torch.eye(M, dtype=torch.float64)
    m0 = torch.randn(M, dtype=torch.float64, generator=g)
    L0 = eye + torch.triu(torch.randn(M, M, dtype=torch.float64, generator=g), 1)
    gm0 = torch.randn(M, dtype=torch.float64, generator=g)
    cpu1 = _layer_inputs(M, 77)
    m1_ref, L1_ref, B1, ok = R.natgrad_update(*cpu1, 1.0)
    bad = dict(m=m0.to(DEV), L_S=L0.to(DEV), g_m=gm0.to(DEV), g_LS=(-2.0 * eye).to(DEV))
    good = _records([cpu1], [1.0])[0]
    table = _run([bad, good], 1.0)
    assert torch.equal(_bits(bad["m"]), _bits(m0)) and torch.equal(_bits(bad["L_S"]), _bits(L0))
    assert table.skipped.tolist() == [1, 0] and int(table.info[0]) > 0 and int(table.info[1]) == 0
    assert table.natgrad_steps.tolist() == [1, 1]
    _assert_matches(M, cpu1, good, m1_ref, L1_ref, float(torch.linalg.cond(B1)), ok, "next to a skipped layer")


@pytest.mark.parametrize("guard", ["info", "loss", "status"])
def test_a_guarded_layer_is_left_bitwise_untouched(guard):
    """The producing step reported a failed Cholesky (a non-zero info word), a non-finite loss, or an abandoned wait (its status
    word): m, L_S, the counter, skipped and info of that layer are all bitwise what they were; the neighbour, whose producer is
    healthy, is updated."""
    M, gamma, scale = 33, 0.7, 3.0
    cpu, m_ref, L_ref, cond, ok = _reference(M, 100 * M, gamma, scale)
    infos = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    losses = torch.tensor([1.5, 2.5], dtype=torch.float64, device=DEV)
    status = torch.zeros(2, dtype=torch.int64, device=DEV)
    if guard == "info":
        infos[0, 2] = 4
    elif guard == "loss":
        losses[0] = NAN
    else:
        status[0] = 1
    steps = torch.tensor([5, 5], dtype=torch.int64, device=DEV)
    words = torch.tensor([[2, 2], [9, 9]], dtype=torch.int32, device=DEV)
    recs = _records([cpu, cpu], [scale, scale], guard_info=[infos[0], infos[1]], guard_loss=[losses[0:1], losses[1:2]],
                    guard_status=[status[0:1], status[1:2]], step_count=[steps[0:1], steps[1:2]],
                    skipped=[words[0, 0:1], words[0, 1:2]], info=[words[1, 0:1], words[1, 1:2]])
    before = (recs[0]["m"].clone(), recs[0]["L_S"].clone())
    _run(recs, gamma)
    assert torch.equal(_bits(recs[0]["m"]), _bits(before[0])) and torch.equal(_bits(recs[0]["L_S"]), _bits(before[1]))
    assert steps.tolist() == [5, 6] and words.tolist() == [[2, 2], [9, 0]]
    _assert_matches(M, cpu, recs[1], m_ref, L_ref, cond, ok, "next to a guarded layer")


def test_bad_arguments_are_refused_before_anything_is_written():
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as F
    lib = _lib.require_device()
    M = 40
    cpu = _layer_inputs(M, 3)
    recs = _records([cpu], [1.0])
    table = F.NatGradSmallLayers(recs)
    before = [recs[0][k].clone() for k in ("m", "L_S")]
    host, dev = ctypes.cast(table.host, ctypes.c_void_p), ctypes.c_void_p(table._dev_table.data_ptr())
    call = lambda h, d, n, g, g0, w: lib.mobocmf_natgrad_small_step(h, d, n, g, g0, w, None)
    inf = float("inf")
    for args in ((None, dev, 1, 0.1, 0.1, 0), (host, None, 1, 0.1, 0.1, 0), (host, dev, 0, 0.1, 0.1, 0), (host, dev, 1, 0.0, 0.1, 0),
                 (host, dev, 1, -0.1, 0.1, 0), (host, dev, 1, inf, 0.1, 0), (host, dev, 1, NAN, 0.1, 0), (host, dev, 1, 0.1, 0.0, 0),
                 (host, dev, 1, 0.1, NAN, 0), (host, dev, 1, 0.1, 0.2, 0), (host, dev, 1, 0.1, 0.1, -1)):
        assert call(*args) == _lib.BAD_ARG, args
    rec = table.host[0]
    for field, values in (("M", (0, -1, 129)), ("scale", (0.0, -1.0, inf, NAN)), ("n_guard_info", (-1, 2)),
                          ("m", (None,)), ("L_S", (None,)), ("g_m", (None,)), ("g_LS", (None,)), ("step_count", (None,)),
                          ("skipped", (None,)), ("info", (None,)), ("work", (None,))):
        keep = getattr(rec, field)
        for v in values:
            setattr(rec, field, v)
            assert call(host, dev, 1, 0.1, 0.1, 0) == _lib.BAD_ARG, (field, v)
        setattr(rec, field, keep)
    nbytes = ctypes.c_size_t()
    for Mbad in (0, 129):
        assert lib.mobocmf_natgrad_small_work_bytes(Mbad, ctypes.byref(nbytes)) == _lib.BAD_ARG
    assert lib.mobocmf_natgrad_small_work_bytes(M, None) == _lib.BAD_ARG
    torch.cuda.synchronize()
    assert torch.equal(_bits(recs[0]["m"]), _bits(before[0])) and torch.equal(_bits(recs[0]["L_S"]), _bits(before[1]))
    assert table.natgrad_steps.tolist() == [0] and table.words.tolist() == [[0], [0]]
    assert call(host, dev, 1, 0.1, 0.1, 0) == _lib.OK      # the record is whole again
    torch.cuda.synchronize()
    assert table.natgrad_steps.tolist() == [1]
