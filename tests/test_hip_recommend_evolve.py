"""mobocmf_recommend_scores against its numpy restatement (tests/recommend_reference.py) and against the surrogates it scores,
the captured generation of util/recommend_evolve.py against tests/nsga_reference.py, and ``recommend(search="evolve")``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import nsga_reference as R
from tests import recommend_reference as RR
from tests.test_hip_model import rel
from tests.test_hip_pareto_evolve import _dominated_by_any, _fitter

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(shape, scaled) for shape in RR.SHAPES for scaled in (False, True)]

# The fitter of tests/test_hip_pareto_evolve.py has constraints whose predictive z = mean / sqrt(variance) passes neither the
# default rule's Phi^-1(0.999) = 3.09 nor Phi^-1(0.9) = 1.28 at any row of the 300-row grid below.  The tests of the search
# therefore use this probability and these (mean, std) of ``output_scaling`` -- a shift of both constraints by 1 -- under which 97
# of the 300 rows are feasible (measured; ``test_recommend_evolve`` asserts at least 4 and fewer than all).
P_MIN = 0.9
SCALING = {"obj0": (0.0, 1.0), "obj1": (0.0, 1.0), "con0": (1.0, 1.0), "con1": (1.0, 1.0)}


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


# ---------------------------------------------------------------------------------------------- 1. the scores kernel
@pytest.mark.parametrize("shape,scaled", CASES)
def test_scores_against_restatement(shape, scaled):
    from mobocmf_amd import functional as Fn
    n_obj, n_con, T, S = shape
    mom, scale = RR.fixture(*shape)
    scale = scale if scaled else None
    want_F, want_v, prob = RR.scores(mom, n_obj, T, S, scale)
    assert prob.size == 0 or np.abs(prob - RR.P_MIN).min() > 1e-9      # (math.erfc and the device's erfc agree far closer)
    md = _t(mom)
    F, viol = Fn.recommend_scores(md, n_obj, T, S, scale=None if scale is None else _t(scale), p_min=RR.P_MIN)
    assert np.array_equal(F.cpu().numpy(), want_F)
    if n_con == 0:
        assert viol is None
        viol = torch.full((T,), 7.0, dtype=torch.float64, device=DEV)
        Fn.recommend_scores(md, n_obj, T, S, p_min=RR.P_MIN, viol=viol)      # given all the same: written as 0.0
        assert bool((viol == 0).all())
        return
    got = viol.cpu().numpy()
    assert np.array_equal(got == 0.0, want_v == 0.0)
    assert np.array_equal(np.isinf(got), np.isinf(want_v)) and not np.isnan(got).any()
    pos = (want_v > 0.0) & np.isfinite(want_v)
    if pos.any():
        print("largest distance of a violation: %.2f ulp" % _ulps(got[pos], want_v[pos]).max())
        assert _ulps(got[pos], want_v[pos]).max() <= 4.0
    F2, viol2 = Fn.recommend_scores(md, n_obj, T, S, scale=None if scale is None else _t(scale), p_min=RR.P_MIN)
    assert torch.equal(F, F2) and torch.equal(viol, viol2)
    # in place into a column slice of a wider array, as the engine calls it
    wide, vw = torch.zeros(n_obj, 2 * T + 3, dtype=torch.float64, device=DEV), torch.zeros(2 * T, dtype=torch.float64, device=DEV)
    Fn.recommend_scores(md, n_obj, T, S, scale=None if scale is None else _t(scale), p_min=RR.P_MIN, F=wide[:, T:], viol=vw[T:])
    assert torch.equal(wide[:, T:2 * T], F) and torch.equal(vw[T:], viol)
    assert bool((wide[:, :T] == 0).all()) and bool((wide[:, 2 * T:] == 0).all()) and bool((vw[:T] == 0).all())


def test_scores_degenerate_variances():
    """v < 0, 0 / 0 and a NaN are +inf at the restatement's places; v == 0 leaves the sign of the mean to decide."""
    from mobocmf_amd import functional as Fn
    mom, _ = RR.fixture(2, 2, 64, 3)
    mom[2, 1, 3 * 5:3 * 6] = -5.0                  # constraint 0, test point 5: v < 0
    mom[3, 0, 3 * 9] = np.nan                      # constraint 1, test point 9
    mom[0, 0, 3 * 11 + 1] = np.nan                 # an objective: F is NaN, the violation is untouched
    want_F, want_v, _ = RR.scores(mom, 2, 64, 3)
    F, viol = Fn.recommend_scores(_t(mom), 2, 64, 3, p_min=RR.P_MIN)
    assert np.array_equal(F.cpu().numpy(), want_F, equal_nan=True) and np.isnan(want_F[0, 11])
    got = viol.cpu().numpy()
    assert np.isinf(want_v[[5, 9]]).all() and np.array_equal(np.isinf(got), np.isinf(want_v))
    assert np.array_equal(got == 0.0, want_v == 0.0)
    one = np.array([[[0.0, 0.0, 1e-300, -1e-300]] * 2, [[0.0, -1.0, 1e-300, -1e-300], [0.0, 0.0, 0.0, 0.0]]])      # S = 1
    _, v1 = Fn.recommend_scores(_t(one), 1, 4, 1, p_min=RR.P_MIN)
    assert v1.cpu().numpy().tolist() == RR.scores(one, 1, 4, 1)[1].tolist() == [np.inf, np.inf, 0.0, np.inf]


def test_scores_refuses_bad_arguments():
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as Fn
    lib = _lib.require_device()
    T, S = 8, 3
    mom = torch.ones(4, 2, T * S, dtype=torch.float64, device=DEV)
    F, viol = torch.zeros(2, T, dtype=torch.float64, device=DEV), torch.zeros(T, dtype=torch.float64, device=DEV)
    good = dict(moments=Fn._ptr(mom), n_obj=2, n_con=2, T=T, S=S, scale=None, p_min=0.999, z_min=3.0902, F=Fn._ptr(F), ldf=T,
                viol=Fn._ptr(viol))

    def call(**kw):
        a = dict(good, **kw)
        return lib.mobocmf_recommend_scores(a["moments"], a["n_obj"], a["n_con"], a["T"], a["S"], a["scale"], a["p_min"], a["z_min"],
                                            a["F"], a["ldf"], a["viol"], Fn._stream())
    assert call() == _lib.OK
    null = ctypes.c_void_p(0)
    bad = [dict(moments=null), dict(F=null), dict(viol=null), dict(n_obj=0), dict(n_obj=-1), dict(n_obj=_lib.PARETO_MAX_K + 1, n_con=0),
           dict(n_con=-1), dict(n_obj=16, n_con=49), dict(T=0), dict(T=-3), dict(S=0), dict(T=4097, S=4096, ldf=4097),
           dict(ldf=T - 1), dict(p_min=0.0), dict(p_min=1.0), dict(p_min=-0.5), dict(p_min=1.5), dict(p_min=float("nan")),
           dict(z_min=float("inf")), dict(z_min=float("-inf")), dict(z_min=float("nan"))]
    for kw in bad:
        assert call(**kw) == _lib.BAD_ARG, kw
    assert call(n_con=0, viol=null) == _lib.OK      # without constraints the violation may be NULL
    torch.cuda.synchronize()
    with pytest.raises(_lib.MobocmfError, match="BAD_ARG"):
        Fn.recommend_scores(mom, 2, T, S, p_min=1.0)
    with pytest.raises(_lib.MobocmfError):
        Fn.recommend_scores(mom, 2, T, S + 1)
    with pytest.raises(_lib.MobocmfError):
        Fn.recommend_scores(mom, 2, T, S, F=torch.zeros(2, 2 * T, dtype=torch.float64, device=DEV)[:, ::2])


# ---------------------------------------------------------------------------------------------- 2. the scores and the model
def _models(fitter):
    """Objectives, then constraints, each in global-index order: the models as ``recommend`` hands them to the engine."""
    return [fitter.get_model("obj0"), fitter.get_model("obj1"), fitter.get_model("con0", True), fitter.get_model("con1", True)]


def test_scores_against_the_model():
    """The kernel on a predict group's moments against MFDGP.predict_for_acquisition at the top fidelity: the means, and the
    variances less the likelihood noise, to what tests/test_hip_tiny_step.py holds TinyPredictGroup to against it (moments:
    1e-9 the means, 1e-8 the variances)."""
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as Fn
    from mobocmf_amd.util.recommend_evolve import choose_group
    from mobocmf_amd.util.tiny_step import TinyPredictGroup
    fitter = _fitter()
    models, T = _models(fitter), 32
    X = torch.rand(T, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).to(DEV)
    ref_m, ref_v = [], []
    with torch.no_grad():
        for m in models:
            m.eval()
            mu, v = m.predict_for_acquisition(X, 1)
            m.train()
            ref_m.append(mu.reshape(-1))
            ref_v.append(v.reshape(-1) - getattr(m, m.name_hidden_layer_likelihood + "1").noise.reshape(-1)[0])
    ref_m, ref_v = torch.stack(ref_m), torch.stack(ref_v)
    grp = choose_group(models, 1, T, 2)
    assert type(grp) is TinyPredictGroup
    grp.x.copy_(X)
    grp._launch(_lib.STEP_FORWARD)
    means, _ = Fn.recommend_scores(grp.moments, 4, T, grp.S)              # every model as an objective: F is mbar
    assert rel(means, ref_m) < 1e-9, rel(means, ref_m)
    want_F, want_v, prob = RR.scores(grp.moments.cpu().numpy(), 2, T, grp.S, p_min=P_MIN)
    F, viol = Fn.recommend_scores(grp.moments, 2, T, grp.S, p_min=P_MIN)
    assert np.array_equal(F.cpu().numpy(), want_F) and np.array_equal(viol.cpu().numpy() == 0.0, want_v == 0.0)
    # the variance the kernel uses, recovered from what it wrote: with p_min = 0.5 and z_min = 0 a lone constraint with z < 0
    # fails with viol = -z exactly, z = mbar / sqrt(v).  Every model in turn as that constraint, once as it is and once with its
    # mean's sign turned (factor -1 leaves v as it is): a row fails in one of the two calls.
    for c in range(4):
        pair = grp.moments[[0, c]].contiguous()
        w = [Fn.recommend_scores(pair, 1, T, grp.S, scale=_t([[0.0, 1.0], [0.0, f]]), p_min=0.5, z_min=0.0)[1] for f in (1.0, -1.0)]
        assert bool(((w[0] == 0) != (w[1] == 0)).all())
        v = (means[c] / torch.maximum(w[0], w[1])) ** 2
        assert rel(v, ref_v[c]) < 1e-8, (c, rel(v, ref_v[c]))


# ---------------------------------------------------------------------------------------------- 3. the engine
def _scale_rows():
    return [list(SCALING[name]) for name in ("obj0", "obj1", "con0", "con1")]


def test_generations_against_restatement():
    """Np = 32, d = 2, six generations: the engine (graph replays) against nsga_reference.evolve around the same group class's
    forward launch and the scores kernel -- bitwise, two forward launches on the same rows being bitwise equal."""
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as Fn
    from mobocmf_amd.util.recommend_evolve import RecommendEvolve, choose_group
    fitter = _fitter()
    models, Np, d, gens = _models(fitter), 32, 2, 6
    scale = _t(np.array(_scale_rows()))
    grp = choose_group(models, 1, Np, d)

    def evaluate(X):
        grp.x.copy_(_t(X))
        grp._launch(_lib.STEP_FORWARD)
        F, viol = Fn.recommend_scores(grp.moments, 2, Np, grp.S, scale=scale, p_min=P_MIN)
        return F.cpu().numpy(), viol.cpu().numpy()

    x0 = np.random.default_rng(3).random((Np, d))
    first = evaluate(x0)
    again = evaluate(x0)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])      # the precondition of what follows
    assert (first[1] == 0.0).any() and (first[1] > 0.0).any()

    def run(seed, use_graph=True):
        eng = RecommendEvolve(models, 2, 1, Np, d, seed, p_min=P_MIN, scale=_scale_rows())
        eng.use_graph = use_graph
        assert type(eng.group) is type(grp)
        eng.start(_t(x0))
        eng.run(gens)
        out = {k: v.cpu().numpy() for k, v in eng.result().items()}
        eng.finish()
        assert (eng._graph is not None) == use_graph
        return out

    got = run(9)
    want = R.evolve(x0, evaluate, gens, 9)
    for key in ("X", "F", "viol", "rank", "crowd"):
        assert np.array_equal(got[key], want[key]), key
    assert int(got["generation"][0]) == gens
    eager, same, other = run(9, use_graph=False), run(9), run(10)
    for key in ("X", "F", "viol", "rank", "crowd"):
        assert np.array_equal(got[key], eager[key]) and np.array_equal(got[key], same[key]), key
    assert not np.array_equal(got["X"], other["X"])
    assert got["X"].min() >= 0.0 and got["X"].max() <= 1.0


def test_engine_refuses_what_it_cannot_run():
    from mobocmf_amd.util.recommend_evolve import RecommendEvolve
    models = _models(_fitter())
    for kw in (dict(Np=3), dict(Np=6, n_obj=0), dict(Np=514), dict(Np=8, p_min=1.0), dict(Np=8, d=33)):
        a = dict(dict(n_obj=2, Np=8, d=2, p_min=0.9), **kw)
        with pytest.raises(ValueError):
            RecommendEvolve(models, a["n_obj"], 1, a["Np"], a["d"], 0, p_min=a["p_min"])
    from mobocmf_amd.util import synthetic
    on_host = [synthetic.model_from_problem(synthetic.make_problem(d=2, L=2, M=16, N=16, S=1, output=o, seed=o),
                                            num_samples_for_training=1, device="cpu") for o in range(3)]
    with pytest.raises(ValueError, match="TinyPredictGroup.*CoopPredictGroup.*PanelPredictGroup.*SplitPredictGroup"):
        RecommendEvolve(on_host, 2, 1, 8, 2, 0)          # parameters on the host: every class says why not, no fallback


# ---------------------------------------------------------------------------------------------- 4. the fitter
@functools.lru_cache(maxsize=None)
def _recommendations():
    fitter = _fitter()
    grid = np.random.default_rng(7).random((300, 2))
    kw = dict(min_feasible_prob=P_MIN, output_scaling=SCALING)
    plain = fitter.recommend(grid, **kw)
    named = fitter.recommend(grid, search="grid", evolve_population=32, evolve_generations=10, evolve_seed=5, **kw)
    evolved = fitter.recommend(grid, search="evolve", evolve_population=32, evolve_generations=10, **kw)
    return fitter, grid, kw, plain, named, evolved


def test_recommend_grid_keeps_its_bits():
    _, _, _, plain, named, _ = _recommendations()
    assert np.array_equal(plain[0], named[0]) and np.array_equal(plain[1], named[1])
    assert set(plain[2]) == set(named[2]) == {"mask", "num_feasible", "num_front", "num_nan"}
    assert np.array_equal(plain[2]["mask"], named[2]["mask"]) and all(plain[2][k] == named[2][k] for k in plain[2] if k != "mask")


def test_recommend_evolve():
    """Measured on an MI355X: hypervolume of the grid's recommendation 4.843266175 (13 rows), of the evolved one 5.890493825
    (30 rows, 26 of them evolved), against max + 0.1 over both predicted fronts."""
    from mobocmf_amd.util.hypervolume import HV
    fitter, grid, kw, (gs, gf, ginfo), _, (es, ef, info) = _recommendations()
    assert ginfo["num_feasible"] >= 4 and ginfo["num_feasible"] < 300       # the precondition: the constants above
    assert info["mask"].shape == (300,) and info["mask"].dtype == bool
    assert info["population"].shape == (32, 2) and info["evolved_mask"].shape == (32,)
    assert info["generations"] == 10 and info["engine"] == "TinyPredictGroup"
    n_grid = int(info["mask"].sum())
    assert info["num_evolved"] == int(info["evolved_mask"].sum()) == es.shape[0] - n_grid and ef.shape == (es.shape[0], 2)
    assert np.array_equal(es[:n_grid], grid[info["mask"]])
    assert np.array_equal(es[n_grid:], info["population"][info["evolved_mask"]])
    assert es.min() >= 0.0 and es.max() <= 1.0
    # every row of the grid's front is in the result or dominated by one of its rows
    for x, p in zip(gs, gf):
        assert (es == x).all(1).any() or _dominated_by_any(ef, p), (x, p)
    # every returned row passes the grid rule
    again = fitter.recommend(es, **kw)
    assert again[2]["mask"].all() and again[2]["num_nan"] == 0
    ref = np.maximum(gf.max(0), ef.max(0)) + 0.1
    hv_grid, hv_evolve = HV(ref_point=ref)(gf), HV(ref_point=ref)(ef)
    print("hypervolume: grid %.9f (%d rows), evolve %.9f (%d rows, %d of them evolved)"
          % (hv_grid, len(gf), hv_evolve, len(ef), info["num_evolved"]))
    assert hv_evolve >= hv_grid
    # the same call again: the same bits
    es2, ef2, _ = fitter.recommend(grid, search="evolve", evolve_population=32, evolve_generations=10, **kw)
    assert np.array_equal(es, es2) and np.array_equal(ef, ef2)


def test_recommend_refuses_bad_keywords():
    fitter, grid, kw, *_ = _recommendations()
    for bad in (dict(search="nsga"), dict(evolve_population=3), dict(evolve_population=33), dict(evolve_population=514),
                dict(evolve_generations=0), dict(search="evolve", evolve_population=2)):
        with pytest.raises(ValueError):
            fitter.recommend(grid, **dict(kw, **bad))
