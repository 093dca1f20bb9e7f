"""mobocmf_exact_predict (csrc/exact_predict.hip) through the C ABI: componentwise against the longdouble restatement on the L^-1
and a GIVEN (tests/mes_reference.py: the bounds and where their constants come from), determinism, what is never written,
and the refusals.  The training covariances are factor_case("rbf", n) -- the workload's conditioning, 1e6 .. 1e9 -- factorised
by mobocmf_exact_gp_factor; the kernel inputs (training points, levels, lengthscales) are independent of them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import kernel_reference as KR
from tests import mes_reference as M

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 8
FORWARD, INPUT_GRADIENTS = 2, 3      # MOBOCMF_STEP_FORWARD / MOBOCMF_STEP_INPUT_GRADIENTS
_gp = {}


def _factor(n):
    """The factorisation of factor_case("rbf", n) by mobocmf_exact_gp_factor, once per order (left unchanged)."""
    if n not in _gp:
        K, y = KR.factor_case("rbf", n)
        g = KR.exact_gp(K, n, y, KR.make_tuning())
        assert g.info == 0
        g.Li_host, g.a_host = g.Li.cpu().numpy().copy(), g.a.cpu().numpy().copy()
        _gp[n] = g
    return _gp[n]


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


class Launch:
    """The descriptors of ``cases`` (one model each; they share T, d and x) over NaN-filled outputs with GUARD doubles behind
    each; ``run(mode)`` launches and synchronises."""

    def __init__(self, cases, x=None):
        from mobocmf_amd import _lib
        self._lib, self.cases = _lib, cases
        T, d = cases[0]["T"], cases[0]["d"]
        dv = lambda a, dt=torch.float64: torch.tensor(np.array(a), dtype=dt).to(DEV)      # (the cases are read-only: a copy)
        self.x = dv(cases[0]["x"] if x is None else x)
        self.host = (_lib.ExactPredictModel * len(cases))()
        self.keep, self.mean, self.var, self.grad = [], [], [], []
        for i, c in enumerate(cases):
            g = _factor(c["n"])
            t = dict(xtr=dv(c["xtr"]), lev=dv(c["lev"], torch.int32), sig=dv(c["sig"]), ntab=dv(c["ntab"]), hyp_s=dv(c["hyp_s"]),
                     hyp_n=dv(c["hyp_n"]), gm=dv(c["gm"]), gv=dv(c["gv"]))
            self.keep.append(t)
            self.mean.append(_nan(T + GUARD)); self.var.append(_nan(T + GUARD)); self.grad.append(_nan(T * d + GUARD))
            r = self.host[i]
            r.n, r.d, r.T, r.n_levels, r.level, r.reserved, r.ld = c["n"], d, T, c["n_levels"], c["level"], 0, g.npad
            r.xtr, r.lev, r.sig, r.ntab = t["xtr"].data_ptr(), t["lev"].data_ptr(), t["sig"].data_ptr(), t["ntab"].data_ptr()
            r.hyp_s, r.hyp_n, r.Linv, r.a, r.kss = t["hyp_s"].data_ptr(), t["hyp_n"].data_ptr(), g.Li.data_ptr(), g.a.data_ptr(), c["kss"]
            r.x, r.top_mean, r.top_var = self.x.data_ptr(), self.mean[i].data_ptr(), self.var[i].data_ptr()
            r.seed_gmean, r.seed_gvar, r.grad, r.work = t["gm"].data_ptr(), t["gv"].data_ptr(), self.grad[i].data_ptr(), None
        self.table = torch.zeros(ctypes.sizeof(self.host), dtype=torch.uint8, device=DEV)
        self.upload()

    def upload(self):
        self.table.copy_(torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8))

    def poison(self):
        for t in self.mean + self.var + self.grad:
            t.fill_(float("nan"))

    def call(self, mode, n_models=None, host=None, table=True):
        n = len(self.cases) if n_models is None else n_models
        return KR.lib().mobocmf_exact_predict(ctypes.cast(self.host if host is None else host, ctypes.c_void_p),
                                              KR._p(self.table) if table else None, n, mode, KR._stream())

    def run(self, mode):
        assert self.call(mode) == 0
        torch.cuda.synchronize()
        return self

    def out(self, i):
        T, d = self.cases[i]["T"], self.cases[i]["d"]
        return (self.mean[i][:T].cpu().numpy(), self.var[i][:T].cpu().numpy(), self.grad[i][:T * d].cpu().numpy().reshape(T, d))

    def guards_nan(self, grad_written):
        T, d = self.cases[0]["T"], self.cases[0]["d"]
        ok = all(bool(torch.isnan(t[T:]).all()) for t in self.mean + self.var)
        return ok and all(bool(torch.isnan(t[T * d if grad_written else 0:]).all()) for t in self.grad)


def _check(c, L, i, with_grad):
    g = _factor(c["n"])
    ref = M.exact_predict_ref(c, g.Li_host, g.a_host)
    mean, var, grad = L.out(i)
    ok, r = M.exact_predict_check(c, ref, mean, var, grad if with_grad else None)
    print("n=%d d=%d T=%d %s level %d:" % (c["n"], c["d"], c["T"], c["kind"], c["level"]),
          {k: round(v, 1) for k, v in r.items()}, "allowed", M.moments_units(c["n"]), M.grad_units(c["n"]))
    assert ok, r
    return ref


CASES = [(n, d, T, kind, level) for n, d, T in M.EXACT_PREDICT_CASES for kind, nl in M.EXACT_PREDICT_KINDS.items() for level in range(nl)]


@pytest.mark.parametrize("n,d,T,kind,level", CASES, ids=lambda v: str(v))
def test_moments_and_input_gradient_within_their_componentwise_bounds(n, d, T, kind, level):
    """FORWARD writes the moments and nothing else; with ALL outputs poisoned in between, INPUT_GRADIENTS writes the same
    moments bit for bit and the gradient (it does not need the first call); a second call repeats every bit; the NaN guards
    behind every output stay NaN and exactly T rows are written."""
    c = M.exact_predict_case(n, d, T, kind, level)
    L = Launch([c]).run(FORWARD)
    assert L.guards_nan(grad_written=False)
    _check(c, L, 0, False)
    fwd = [a.copy() for a in L.out(0)[:2]]
    L.poison()
    L.run(INPUT_GRADIENTS)
    assert L.guards_nan(grad_written=True)
    ref = _check(c, L, 0, True)
    got = [a.copy() for a in L.out(0)]
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(fwd, got[:2]))
    zero = (c["gm"] == 0) & (c["gv"] == 0)
    assert (got[2][zero] == 0).all() and (np.abs(ref["grad"][~zero]).max(initial=1.0) > 0)
    L.poison()
    L.run(INPUT_GRADIENTS)
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(got, L.out(0)))


def test_models_of_different_n_in_one_launch():
    """n = 17, 65 and 130 together (the grid and the LDS are sized for the largest): each equals its own single-model launch
    bit for bit, and passes its bound."""
    cases = [M.exact_predict_case(n, 2, 17, kind, level) for n, kind, level in ((17, "mf", 1), (65, "lin", 2), (130, "lin", 0))]
    x = cases[0]["x"]
    cases = [dict(c, x=x) for c in cases]
    L = Launch(cases).run(INPUT_GRADIENTS)
    assert L.guards_nan(grad_written=True)
    for i, c in enumerate(cases):
        _check(c, L, i, True)
        single = Launch([c]).run(INPUT_GRADIENTS)
        assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(L.out(i), single.out(0)))


@pytest.mark.parametrize("T", [1, 16, 17])
def test_exactly_T_rows_are_written(T):
    c = M.exact_predict_case(65, 2, T, "mf", 1)
    L = Launch([c]).run(INPUT_GRADIENTS)
    mean, var, grad = L.out(0)
    assert np.isfinite(mean).all() and np.isfinite(var).all() and np.isfinite(grad).all()
    assert L.guards_nan(grad_written=True)
    _check(c, L, 0, True)


def test_a_level_out_of_range_gives_nan_moments_for_that_model_alone():
    """The levels are device data the host cannot check: a lev_r outside [0, n_levels) makes that model's moments NaN (it is
    never used as an index); the other model of the launch is untouched by it."""
    a, b = M.exact_predict_case(65, 2, 17, "mf", 1), M.exact_predict_case(17, 2, 17, "mf", 0)
    b = dict(b, x=a["x"])
    L = Launch([a, b])
    clean = [x.copy() for x in Launch([b]).run(FORWARD).out(0)[:2]]
    for bad in (2, -1, 1 << 30):
        L.keep[0]["lev"][40] = bad
        L.poison()
        L.run(FORWARD)
        assert np.isnan(L.out(0)[0]).all() and np.isnan(L.out(0)[1]).all()
        assert all(np.array_equal(p, q) for p, q in zip(clean, L.out(1)[:2]))


def test_refusals_come_before_any_launch():
    """The BAD_ARG table of include/mobocmf_hip.h; every refused call leaves the outputs NaN."""
    from mobocmf_amd import _lib
    c = M.exact_predict_case(17, 3, 16, "lin", 1)
    L = Launch([c])
    base = bytes(L.host)

    def refused(mode=INPUT_GRADIENTS, n_models=None, table=True, **fields):
        ctypes.memmove(L.host, base, len(base))
        for k, v in fields.items():
            setattr(L.host[0], k, v)
        rc = L.call(mode, n_models=n_models, table=table)
        ctypes.memmove(L.host, base, len(base))
        return rc == KR.BAD_ARG

    for fields in (dict(n=0), dict(n=_lib.EXACT_PREDICT_MAX_N + 1), dict(d=0), dict(d=_lib.MAX_D + 1), dict(T=0),
                   dict(T=_lib.TOPK_MAX_N + 1), dict(n_levels=0), dict(n_levels=_lib.EXACT_PREDICT_MAX_LEVELS + 1), dict(level=-1),
                   dict(level=3), dict(ld=16)):
        assert refused(**fields), fields
    for name in ("xtr", "lev", "sig", "ntab", "hyp_s", "hyp_n", "Linv", "a", "x", "top_mean", "top_var"):
        assert refused(**{name: None}), name
        assert refused(mode=FORWARD, **{name: None}), name
    for name in ("seed_gmean", "seed_gvar", "grad"):
        assert refused(**{name: None}), name
        assert not refused(mode=FORWARD, **{name: None}), name      # FORWARD does not read them
    for mode in (0, 1, 4, 2 | 16, -1):
        assert refused(mode=mode), mode
    assert refused(n_models=0) and refused(n_models=2 * _lib.ACQ_MAX_PAIRS + 1) and refused(table=False)
    assert L.call(INPUT_GRADIENTS, host=ctypes.c_void_p(0)) == KR.BAD_ARG
    torch.cuda.synchronize()
    assert L.guards_nan(grad_written=False)      # only the FORWARD calls above wrote, and only the moments
    nb = ctypes.c_size_t(7)
    lib = KR.lib()
    assert lib.mobocmf_exact_predict_work_bytes(ctypes.byref(L.host[0]), 5, ctypes.byref(nb)) == KR.BAD_ARG
    assert lib.mobocmf_exact_predict_work_bytes(ctypes.byref(L.host[0]), FORWARD, None) == KR.BAD_ARG
    assert lib.mobocmf_exact_predict_work_bytes(None, FORWARD, ctypes.byref(nb)) == KR.BAD_ARG


def test_work_bytes_is_honest():
    """0 bytes for both modes at the largest size: the launch runs with work = NULL (one byte less does not exist), and a
    non-NULL work is left untouched."""
    from mobocmf_amd import functional as F
    c = M.exact_predict_case(512, 2, 5, "mf", 0)
    L = Launch([c])
    for mode in (FORWARD, INPUT_GRADIENTS):
        assert F.exact_predict_work_bytes(L.host[0], mode) == 0
    null = [a.copy() for a in L.run(INPUT_GRADIENTS).out(0)]
    work = _nan(64)
    L.host[0].work = work.data_ptr()
    L.upload()
    L.poison()
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(null, L.run(INPUT_GRADIENTS).out(0)))
    assert bool(torch.isnan(work).all())


def test_wrapper_launches_the_same_bits():
    from mobocmf_amd import functional as F
    c = M.exact_predict_case(130, 8, 33, "lin", 2)
    L = Launch([c]).run(INPUT_GRADIENTS)
    ref = [a.copy() for a in L.out(0)]
    L.poison()
    F.exact_predict_launch(L.host, L.table, INPUT_GRADIENTS)
    torch.cuda.synchronize()
    assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(ref, L.out(0)))
