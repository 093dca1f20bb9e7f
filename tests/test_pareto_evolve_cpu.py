"""MOOP(search="evolve") without a GPU: the numpy restatement of the two NSGA kernels (tests/nsga_reference.py) against the
definitions, keyword validation and defaults, the refusals of the entry points, and the restatement on host chain samples."""
import ctypes
import functools

import numpy as np
import pytest

from tests import nsga_reference as R
from tests.test_rff_refine_cpu import _random_chain


def _brute_ranks(F, viol):
    """Peeling depth straight from the definition: 0 without a dominator, else 1 + the deepest dominator."""
    k, n = F.shape
    v = np.zeros(n) if viol is None else np.array(viol, dtype=float)
    for i in range(n):
        if np.isnan(F[:, i]).any() or np.isnan(v[i]):
            v[i] = np.inf

    def dominates(i, j):
        fi, fj = v[i] == 0, v[j] == 0
        if fi != fj:
            return fi
        if not fi:
            return v[i] < v[j]
        return all(F[c, i] <= F[c, j] for c in range(k)) and any(F[c, i] < F[c, j] for c in range(k))

    @functools.lru_cache(maxsize=None)
    def depth(j):
        return max([depth(i) + 1 for i in range(n) if i != j and dominates(i, j)], default=0)

    return np.array([depth(j) for j in range(n)], dtype=np.int32)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_restatement_ranks_are_the_peeling_depth(k):
    rng = np.random.default_rng(k)
    F = np.round(rng.random((k, 40)) * 6) / 6            # exact ties
    viol = np.where(rng.random(40) < 0.3, np.round(rng.random(40) * 4) / 4, 0.0)
    F[0, 3], viol[5] = np.nan, np.nan
    F[:, 7] = F[:, 8]                                     # equal rows: neither dominates
    for vv in (viol, None):
        dom, _ = R.dominance(F, vv)
        assert np.array_equal(R.ranks(dom), _brute_ranks(F, vv))
    out = R.survive(rng.random((40, 2)), F, viol, 20)
    assert out["src"].shape == (20,) and np.all(np.diff(out["rank"]) >= 0)
    assert np.isinf(out["viol"][out["src"] == 3]).all()


def test_restatement_crowding_on_a_hand_computed_front():
    F = np.array([[0.0, 1.0, 2.0, 4.0, 8.0], [8.0, 5.0, 3.0, 1.0, 0.0]])
    rank = np.zeros(5, dtype=np.int32)
    # interior rows: (next - prev) / (max - min) per objective, objective 0 first
    want = [np.inf, (2.0 - 0.0) / 8.0 + (8.0 - 3.0) / 8.0, (4.0 - 1.0) / 8.0 + (5.0 - 1.0) / 8.0,
            (8.0 - 2.0) / 8.0 + (3.0 - 0.0) / 8.0, np.inf]
    assert np.array_equal(R.crowding(F, rank), np.array(want))
    out = R.survive(np.zeros((5, 1)), F, None, 3)
    assert out["src"].tolist() == [0, 4, 3]                # the ends, then the loneliest interior row
    # a constant objective adds nothing; a one-row and a two-row rank are all ends
    assert np.array_equal(R.crowding(np.array([[1.0, 1.0, 1.0, 1.0]]), np.zeros(4, dtype=np.int32)), [np.inf, 0.0, 0.0, np.inf])
    assert np.isinf(R.crowding(np.array([[1.0, 2.0, 3.0]]), np.array([0, 1, 1], dtype=np.int32))).all()


def test_restatement_philox_and_vary_properties():
    u = R.philox_uniform(7, 3, np.arange(4096, dtype=np.uint64))
    assert u.min() > 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.02
    assert np.array_equal(u, R.philox_uniform(7, 3, np.arange(4096, dtype=np.uint64)))
    assert not np.array_equal(u, R.philox_uniform(7, 4, np.arange(4096, dtype=np.uint64)))
    # Philox4x32-10 known answer (Random123 kat_vectors: zero counter, zero key)
    r = R.philox4x32_10((np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1)), (0, 0))
    assert [int(v[0]) for v in r] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    rng = np.random.default_rng(0)
    X = rng.random((16, 3))
    rank, crowd = rng.integers(0, 3, 16).astype(np.int32), rng.random(16)
    ch, par = R.vary(X, rank, crowd, 5, 0)
    assert ch.shape == (16, 3) and ch.min() >= 0.0 and ch.max() <= 1.0 and par.shape == (16,)
    ch0, par0 = R.vary(X, rank, crowd, 5, 0, p_c=0.0, p_m=1e-300)
    assert np.array_equal(par, par0) and np.array_equal(ch0, X[par0])


def test_moop_search_keywords():
    from mobocmf_amd.util.moop import MOOP
    f = lambda x, gradient=False: np.zeros(len(x))
    for kw in ({"search": "nope"}, {"evolve_population": 2}, {"evolve_population": 514}, {"evolve_population": 65},
               {"evolve_generations": 0}):
        with pytest.raises(ValueError):
            MOOP([f], [], input_dim=2, **kw)
    m = MOOP([f], [], input_dim=2)
    assert (m.search, m.evolve_population, m.evolve_generations, m.evolve_seed) == ("grid", 128, 100, None)
    # no host fallback: host callables, and chain samples that live on no GPU, are refused
    for samples in ([f, f], [_random_chain(2, 8, 0), _random_chain(2, 8, 1)]):
        for refine in ("slsqp", "device"):
            moop = MOOP(samples, [], input_dim=2, grid_size=10, search="evolve", refine=refine, rng=np.random.default_rng(0))
            with pytest.raises(ValueError, match="RFFChainSample"):
                moop.compute_pareto_solution_from_samples(np.zeros((1, 2)))


def test_fitter_pareto_search_keywords():
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    fit = BlackBoxMFDGPFitter(2, 10, device="cpu", pareto_search="evolve", pareto_evolve_population=64,
                              pareto_evolve_generations=7, inducing_selection="first")
    assert fit.model_kwargs == {"inducing_selection": "first"}
    assert fit._moop_search_kwargs() == {"search": "evolve", "evolve_population": 64, "evolve_generations": 7}
    dflt = BlackBoxMFDGPFitter(2, 10, device="cpu")
    assert dflt._moop_search_kwargs() == {"search": "grid", "evolve_population": 128, "evolve_generations": 100}
    assert fit.copy_uncond().pareto_search == "evolve"
    for kw in ({"pareto_search": "nope"}, {"pareto_evolve_population": 3}, {"pareto_evolve_population": 1024},
               {"pareto_evolve_generations": 0}):
        with pytest.raises(ValueError):
            BlackBoxMFDGPFitter(2, 10, device="cpu", **kw)


def test_omitting_search_is_the_grid_mode_bit_for_bit():
    from mobocmf_amd.util.moop import MOOP
    d = 2
    chains = [_random_chain(d, 24, 10 + k) for k in range(3)]
    inputs = np.random.default_rng(1).random((5, d))
    thr = np.array([float(np.quantile(chains[2](np.random.default_rng(2).random((400, d))), 0.4))])
    res, after = [], []
    for kw in ({}, {"search": "grid"}, {"search": "grid", "evolve_population": 8, "evolve_generations": 3, "evolve_seed": 1}):
        rng = np.random.default_rng(4)
        moop = MOOP(chains[:2], chains[2:], input_dim=d, grid_size=150, pareto_set_size=8, feasible_values=thr, rng=rng, **kw)
        out = moop.compute_pareto_solution_from_samples(inputs)
        assert out is not None
        res.append((out[0].numpy(), out[1].numpy()))
        after.append(rng.random())                        # the generator was advanced by the grid draw only
    for s, f in res[1:]:
        assert np.array_equal(s, res[0][0]) and np.array_equal(f, res[0][1])
    rng = np.random.default_rng(4)
    rng.uniform(size=(d * 150, d))
    assert after == [rng.random()] * 3


def test_entry_points_refuse_bad_arguments():
    from mobocmf_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                # never dereferenced: every call below is refused before a launch
    BAD = _lib.BAD_ARG

    def survive(n_in=8, n_keep=4, d=2, k=2, ldf=8, ldf_out=4, viol=None, viol_out=None, **ptr):
        a = {name: ptr.get(name, p) for name in ("X", "F", "X_out", "F_out", "rank_out", "crowd_out", "src_out")}
        return lib.mobocmf_nsga_survive(n_in, n_keep, d, k, a["X"], a["F"], ldf, viol, a["X_out"], a["F_out"], ldf_out,
                                        viol_out, a["rank_out"], a["crowd_out"], a["src_out"], None, None)

    assert survive(k=0) == BAD and survive(k=_lib.PARETO_MAX_K + 1) == BAD
    assert survive(d=0) == BAD and survive(d=_lib.MAX_D + 1) == BAD
    assert survive(n_keep=1) == BAD and survive(n_keep=9) == BAD and survive(n_in=1, n_keep=1) == BAD
    assert survive(n_in=_lib.NSGA_MAX_ROWS + 1, ldf=2048) == BAD
    assert survive(ldf=7) == BAD and survive(ldf_out=3) == BAD
    assert survive(viol=p, viol_out=None) == BAD
    for name in ("X", "F", "X_out", "F_out", "rank_out", "crowd_out", "src_out"):
        assert survive(**{name: None}) == BAD, name

    opt = _lib.NsgaOptions()
    assert lib.mobocmf_nsga_options_init(None) == BAD
    assert lib.mobocmf_nsga_options_init(ctypes.byref(opt)) == _lib.OK
    assert opt.struct_size == ctypes.sizeof(_lib.NsgaOptions)
    assert (opt.eta_c, opt.p_c, opt.eta_m, opt.p_m) == (15.0, 0.9, 20.0, 0.0)

    def vary(Np=8, d=2, o=None, **ptr):
        a = {name: ptr.get(name, p) for name in ("X", "rank", "crowd", "generation", "children")}
        return lib.mobocmf_nsga_vary(Np, d, a["X"], a["rank"], a["crowd"], 1, a["generation"],
                                     None if o is None else ctypes.byref(o), a["children"], None, None)

    assert vary(Np=0) == BAD and vary(Np=7) == BAD and vary(Np=_lib.NSGA_MAX_ROWS + 2) == BAD
    assert vary(d=0) == BAD and vary(d=_lib.MAX_D + 1) == BAD
    for name in ("X", "rank", "crowd", "generation", "children"):
        assert vary(**{name: None}) == BAD, name
    for field, values in (("eta_c", (-1.0, 1001.0, float("nan"))), ("p_c", (-0.1, 1.1, float("nan"))),
                          ("eta_m", (-1.0, 1001.0, float("nan"))), ("p_m", (-0.1, 1.1, float("nan"))),
                          ("struct_size", (0, ctypes.sizeof(_lib.NsgaOptions) + 8))):
        for v in values:
            o = _lib.NsgaOptions()
            lib.mobocmf_nsga_options_init(ctypes.byref(o))
            setattr(o, field, v)
            assert vary(o=o) == BAD, (field, v)


def d8_fixture():
    """Two objectives and one constraint at its 0.4 quantile on d = 8 host chain samples; (chains, thr)."""
    d = 8
    chains = [_random_chain(d, 24, 20 + k) for k in range(3)]
    thr = np.array([float(np.quantile(chains[2](np.random.default_rng(2).random((2000, d))), 0.4))])
    return chains, thr


def host_evaluate(chains, n_obj, thr):
    def evaluate(X):
        vals = np.stack([np.asarray(c(X)).reshape(-1) for c in chains])
        viol = np.zeros(X.shape[0])
        for c in range(n_obj, len(chains)):              # the order of mobocmf_rff_feasibility
            viol = viol + np.minimum(vals[c] - thr[c - n_obj], 0.0)
        return vals[:n_obj], -viol
    return evaluate


def grid_population(evaluate, d, n_grid, Np, seed):
    """(feasible grid values (n, 2), Np starting rows): the non-dominated feasible rows first, then the others in row order."""
    X = np.random.default_rng((seed, 99)).random((n_grid, d))
    F, viol = evaluate(X)
    ok = viol == 0.0
    X, Fm = X[ok], F[:, ok].T
    from mobocmf_amd.util.moop import MOOP
    front = np.flatnonzero(MOOP.compute_pareto_front(Fm))[:Np // 2]
    rest = np.setdiff1d(np.arange(len(X)), front)[:Np - len(front)]
    return Fm, X[np.concatenate((front, rest))]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_evolves_host_chains(seed):
    chains, thr = d8_fixture()
    evaluate = host_evaluate(chains, 2, thr)
    Fgrid, x0 = grid_population(evaluate, 8, 1500, 32, seed)
    ref = Fgrid.max(0) + 0.1
    pop = R.evolve(x0, evaluate, 25, seed)
    assert pop["X"].min() >= 0.0 and pop["X"].max() <= 1.0
    good = pop["viol"] == 0.0
    Fe, ve = evaluate(pop["X"][good])
    # (a host chain evaluates a batch through matrix products: another batch, another summation order)
    assert np.allclose(Fe, pop["F"][:, good], rtol=1e-10, atol=1e-12) and np.all(ve <= 1e-10)
    hv_grid, hv_both = R.hv2d(Fgrid, ref), R.hv2d(np.vstack((Fgrid, pop["F"][:, good].T)), ref)
    print("seed %d: hypervolume grid %.6f, grid + evolved %.6f" % (seed, hv_grid, hv_both))
    assert hv_both >= hv_grid
