"""mobocmf_mes_group_forward (csrc/acq_search.hip) against the 50-digit golden values (tests/golden/mes_kernel_cases.npz, written
by tests/golden/make_mes_golden.py) under the gate of tests/mes_reference.py, the tracking rule, and the refusals."""
import numpy as np
import pytest
import torch

from tests import acq_search_reference as R1
from tests import mes_reference as M

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("shape", M.MES_SHAPES, ids=lambda s: "o%d_c%d_T%d" % s)
def test_value_and_seeds_pass_the_gate(shape):
    """|got - ref| <= C u kappa_max (1 + |ref|) for the value, d/dmean and d/dvar, C = 4 x MES_RATIO_MEASURED; both regimes of
    the cdf clamp occur over the shapes (asserted on the file in test_mes_reference_cpu.py); want_seeds = 0 gives the same bits."""
    from mobocmf_amd import functional as F
    g = M.mes_golden()[shape]
    n_obj, n_con, T = shape
    mom, noise, best = _dev(g["moments"]), _dev(g["noise"]), _dev(g["best"])
    acq, seeds, acq0 = _nan(T + 8), _nan(n_obj + n_con, 2, T), _nan(T)
    F.mes_group_forward(mom, noise, best, n_obj, n_con, T, acq, seeds=seeds)
    F.mes_group_forward(mom, noise, best, n_obj, n_con, T, acq0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(acq[T:]).all())
    assert torch.equal(_bits(acq[:T]), _bits(acq0))
    cl = g["clamped"]
    assert (g["term"][~cl] > 0).all()      # every unclamped term is positive in the reference (the clamped ones: see the CPU test)
    ok, r = M.mes_gate(acq[:T].cpu().numpy(), seeds.cpu().numpy(), g["acq"], g["seeds"], M.mes_kappa_max(g["kappa"], cl))
    print(shape, "device ratios", r, "allowed", M.MES_C)
    assert ok, r
    again = _nan(T)
    seeds2 = _nan(n_obj + n_con, 2, T)
    F.mes_group_forward(mom, noise, best, n_obj, n_con, T, again, seeds=seeds2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(again), _bits(acq0)) and torch.equal(_bits(seeds2), _bits(seeds))


def test_tracks_the_best_iterate():
    """The three-call scenario of tests/test_hip_acq_search.py: the element-wise larger value and its row stay (strict), the -inf
    the caller starts from is replaced by any finite value, a NaN value -- here from a NEGATIVE variance, as on the host --
    never replaces anything."""
    from mobocmf_amd import functional as F
    n_obj, n_con, T, d = 2, 1, 70, 3
    gen = torch.Generator().manual_seed(2)
    best_v = torch.full((T,), float("-inf"), dtype=torch.float64, device=DEV)
    best_x = torch.zeros(T, d, dtype=torch.float64, device=DEV)
    acq = torch.zeros(T, dtype=torch.float64, device=DEV)
    for call in range(3):
        c = M.mes_case(n_obj, n_con, T, seed=20 + call)
        mom = torch.tensor(c["moments"])
        if call == 0:
            mom[0, 1, 1] = -0.3      # test point 1: a negative variance, no value on the first call
        if call == 1:
            mom[2, 1, 0] = -0.1      # test point 0 (the constraint's model): no value on the second
        x = torch.rand(T, d, dtype=torch.float64, generator=gen)
        prev_v, prev_x = best_v.cpu(), best_x.cpu()
        F.mes_group_forward(mom.to(DEV), _dev(c["noise"]), _dev(c["best"]), n_obj, n_con, T, acq, x=x.to(DEV), best_v=best_v, best_x=best_x)
        torch.cuda.synchronize()
        a, got_v, got_x = acq.cpu(), best_v.cpu(), best_x.cpu()
        ref = M.mes_torch(mom, torch.tensor(c["noise"]), torch.tensor(c["best"]), n_obj, n_con)
        ok = torch.isfinite(ref)
        assert torch.equal(ok, torch.isfinite(a)) and bool(((a - ref).abs()[ok] <= 1e-9 * (1.0 + ref.abs()[ok])).all())
        want_v, want_x = R1.track_best(a, x, prev_v, prev_x)      # the rule on the values the launch itself computed
        assert torch.equal(_bits(got_v), _bits(want_v)) and torch.equal(got_x, want_x)
        moved = a > prev_v
        if call == 0:
            assert bool(torch.isnan(a[1])) and float(got_v[1]) == float("-inf") and not bool(got_x[1].any())
            assert bool(torch.isfinite(got_v[0])) and bool(torch.isfinite(got_v[2:]).all()) and int(moved.sum()) == T - 1
        if call == 1:
            assert bool(torch.isnan(a[0])) and float(got_v[0]) == float(prev_v[0]) and torch.equal(got_x[0], prev_x[0])
            assert bool(moved[1]) and bool(torch.isfinite(got_v).all())
        if call >= 1:
            assert 0 < int(moved.sum()) < T


def test_refuses_bad_arguments():
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as F
    z = lambda *s: torch.ones(*s, dtype=torch.float64, device=DEV)
    T, d = 3, 2
    lib = _lib.require_device()
    P = F._ptr
    mom, noise, best, acq, seeds, x, bv, bx = z(3, 2, T), z(3), z(3), z(T), z(3, 2, T), z(T, d), z(T), z(T, d)

    def rc(moments=mom, noise=noise, best=best, n_obj=2, n_con=1, T=T, acq=acq, want=0, seeds=None, track=0, x=None, d=0, bv=None,
           bx=None):
        return lib.mobocmf_mes_group_forward(P(moments), P(noise), P(best), n_obj, n_con, T, P(acq), want, P(seeds), track, P(x), d,
                                             P(bv), P(bx), F._stream())

    assert rc() == _lib.OK and rc(want=1, seeds=seeds) == _lib.OK and rc(track=1, x=x, d=d, bv=bv, bx=bx) == _lib.OK
    assert rc(n_obj=3, n_con=0) == _lib.OK
    for kw in (dict(moments=None), dict(noise=None), dict(best=None), dict(acq=None), dict(n_obj=0), dict(n_obj=0, n_con=3),
               dict(n_con=-1), dict(n_obj=2 * _lib.ACQ_MAX_PAIRS, n_con=1), dict(n_obj=1, n_con=2 * _lib.ACQ_MAX_PAIRS),
               dict(T=0), dict(T=_lib.ACQ_MAX_COLUMNS + 1), dict(want=2), dict(want=-1), dict(want=1, seeds=None), dict(track=2),
               dict(track=-1), dict(track=1, x=None, d=d, bv=bv, bx=bx), dict(track=1, x=x, d=d, bv=None, bx=bx),
               dict(track=1, x=x, d=d, bv=bv, bx=None), dict(track=1, x=x, d=0, bv=bv, bx=bx),
               dict(track=1, x=x, d=_lib.MAX_D + 1, bv=bv, bx=bx)):
        assert rc(**kw) == _lib.BAD_ARG, kw
    torch.cuda.synchronize()
