"""``warm_start="posterior"`` on the host: the q(u) extension against the oracle, the constructor's wiring, its refusals, and the
unchanged default.  The extension is exact: the extended state must give the OLD state's moments and KL.  Bounds: 1e-8 (about 100x
the 7.6e-11 / 4.1e-11 the oracle itself showed on these cases)."""
import copy

import numpy as np
import pytest
import torch

from mobocmf_amd.models import MFDGP, TL
from mobocmf_amd.util import synthetic, warm_start
from oracle import mfdgp_oracle as O
from tests.helpers import oracle_state, small_problem, to_t
from tests.test_hip_model import _raw_from_model

TOL = 1e-8
# (d, L, M, M', one new row duplicates an old one)
CASES = [(2, 2, 8, 9, False), (2, 3, 13, 16, False), (1, 2, 16, 18, True), (8, 2, 33, 38, False)]
IDS = ["d2_L2_8to9", "d2_L3_13to16", "d1_L2_16to18_duplicate", "d8_L2_33to38"]


def packed(hyp):
    """Oracle hyper-parameter dict -> the C-ABI order ``warm_start.gram`` takes."""
    if "alpha" in hyp:
        return torch.cat([hyp["alpha"].reshape(1), hyp["ls"].reshape(-1)])
    return torch.cat([hyp[k].reshape(-1) for k in ("a1", "af", "nu", "a2", "lsf", "ls1", "ls2")])


def new_rows(d, n, duplicate_of=None, seed=11):
    z = torch.rand(n, d, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    if duplicate_of is not None:
        z[0] = duplicate_of
    return z


def extended_state(st, Z_new):
    """The oracle state ``st`` with every layer's q(u) extended to the inducing inputs [Z_x; Z_new]."""
    M = st["Zx"].shape[0]
    layers, f_old, f_new = [], None, None
    for l, lay in enumerate(st["layers"]):
        Zo = st["Zx"] if l == 0 else torch.cat([st["Zx"], f_old[:, None]], 1)
        Zn = Z_new if l == 0 else torch.cat([Z_new, f_new[:, None]], 1)
        m, L_S, _ = warm_start.extend_qu(packed(lay["hyp"]), min(l, 1), Zo, Zn, lay["m"], lay["L_S"], O.JITTER)
        assert torch.equal(m[:M], lay["m"]) and torch.equal(L_S[:M, :M], lay["L_S"])      # old rows: bitwise
        layers.append({"hyp": lay["hyp"], "m": m, "L_S": L_S})
        f_old, f_new = m[:M], m[M:]
    return {"Zx": torch.cat([st["Zx"], Z_new]), "layers": layers, "noise": st["noise"], "samples": st["samples"]}


def assert_same_function(st_new, st_old, d, seed=5):
    """Every layer's moments at 17 random inputs with the same eps, train and eval branch, and every layer's KL."""
    g = torch.Generator().manual_seed(seed)
    L = len(st_old["layers"])
    x = torch.rand(17, d, dtype=torch.float64, generator=g)
    eps = [None] + [torch.randn(17, dtype=torch.float64, generator=g) for _ in range(1, L)]
    worst = 0.0
    for training in (True, False):
        new = O.model_forward(st_new, x, eps=eps, training=training)
        old = O.model_forward(st_old, x, eps=eps, training=training)
        for l in range(L):
            for a, b in zip(new[l], old[l]):
                err = ((a - b).abs() / b.abs().clamp_min(1.0)).max().item()
                worst = max(worst, err)
                assert err <= TOL, (l, training, err)
    for l in range(L):
        kn = O.kl_layer(st_new["layers"][l]["hyp"], O.inducing_inputs(st_new, l), st_new["layers"][l]["m"], st_new["layers"][l]["L_S"])
        ko = O.kl_layer(st_old["layers"][l]["hyp"], O.inducing_inputs(st_old, l), st_old["layers"][l]["m"], st_old["layers"][l]["L_S"])
        assert abs(float(kn) - float(ko)) <= TOL * abs(float(ko)), (l, float(kn), float(ko))
    return worst


@pytest.mark.parametrize("d,L,M,M2,dup", CASES, ids=IDS)
def test_extend_qu_preserves_moments_and_kl(d, L, M, M2, dup):
    st = oracle_state(small_problem(d=d, L=L, M=M, N=M + 4, S=2, seed=3))
    Z_new = new_rows(d, M2 - M, duplicate_of=st["Zx"][2] if dup else None)
    st_new = extended_state(st, Z_new)
    assert st_new["layers"][0]["m"].shape[0] == M2
    for lay in st_new["layers"]:      # a proper factor: lower triangular where it is new, positive diagonal
        assert torch.equal(torch.triu(lay["L_S"], 1)[M:], torch.zeros(M2 - M, M2, dtype=torch.float64))
        assert bool((torch.diagonal(lay["L_S"])[M:] > 0).all())
    assert_same_function(st_new, st, d)


def test_extend_qu_pure_copy_and_gram_against_oracle():
    st = oracle_state(small_problem(d=3, L=2, M=7, N=9, S=2, seed=3))
    for l, lay in enumerate(st["layers"]):
        Z = O.inducing_inputs(st, l)
        m, L_S, A = warm_start.extend_qu(packed(lay["hyp"]), l, Z, Z[:0], lay["m"], lay["L_S"], O.JITTER)
        assert torch.equal(m, lay["m"]) and torch.equal(L_S, lay["L_S"]) and A.shape == (7, 0)
        X = torch.rand(5, Z.shape[1], dtype=torch.float64, generator=torch.Generator().manual_seed(l))
        assert torch.allclose(warm_start.gram(packed(lay["hyp"]), l, Z, X), O.gram(lay["hyp"], Z, X), rtol=1e-14, atol=0)


def test_extend_qu_not_positive_definite():
    from mobocmf_amd.layers import NotPSDError
    st = oracle_state(small_problem(d=2, L=2, M=8, N=12, S=2, seed=3))
    lay = st["layers"][0]
    with pytest.raises(NotPSDError):      # a duplicated row without any jitter: C = 0 up to rounding, made negative here
        warm_start.extend_qu(packed(lay["hyp"]), 0, st["Zx"], st["Zx"][2:3], lay["m"], lay["L_S"], -1e-9)


# ------------------------------------------------------------------------------------------------ constructor wiring
def _previous(L, N, seed=3):
    """A model with Z = all N training rows carrying a synthetic problem's parameters, and the problem."""
    prob = synthetic.make_problem(d=2, L=L, M=N, N=N, S=2, seed=seed)
    return synthetic.model_from_problem(prob, device="cpu"), prob


def _grown(prob, n_new, seed=17):
    """The problem's data with ``n_new`` rows appended (lowest fidelity first, then the top one)."""
    xa = np.random.default_rng(seed).random((n_new, prob["d"]))
    fa = np.array([0.0, float(prob["L"] - 1), 0.0][:n_new])
    lo, hi = synthetic.target(xa, 0)
    ya = np.where(fa == 0, lo, hi)
    x, y, fid = np.vstack([prob["x"], xa]), np.concatenate([prob["y"], ya]), np.concatenate([prob["fid"], fa])
    return to_t(x), to_t(y)[:, None], to_t(fid)[:, None]


@pytest.mark.parametrize("L,N", [(2, 10), (3, 12)], ids=["L2", "L3"])
@pytest.mark.parametrize("n_new", [1, 3])
def test_constructor_carries_posterior_over(L, N, n_new):
    prev, prob = _previous(L, N)
    x, y, fid = _grown(prob, n_new)
    new = MFDGP(x, y, fid, L, type_lengthscale=TL.ONES, num_samples_for_acquisition=2, num_samples_for_training=2,
                previously_trained_model=prev, warm_start="posterior")
    assert new.hidden_layer_0.variational_strategy.Zx.shape[0] == N + n_new
    assert all(p.dtype == torch.float64 for p in new.parameters())
    st_old, st_new = O.state_from_raw(_raw_from_model(prev, L)), O.state_from_raw(_raw_from_model(new, L))
    with torch.no_grad():
        assert_same_function(st_new, st_old, prob["d"])
    for l in range(L):
        lo, ln = getattr(prev, f"hidden_layer_{l}"), getattr(new, f"hidden_layer_{l}")
        vo, vn = lo.variational_strategy._variational_distribution, ln.variational_strategy._variational_distribution
        assert torch.equal(vn.variational_mean[:N], vo.variational_mean)
        assert torch.equal(vn.chol_variational_covar[:N, :N], vo.chol_variational_covar)
        so, sn = lo.covar_module.state_dict(), ln.covar_module.state_dict()
        assert so.keys() == sn.keys() and all(torch.equal(so[k], sn[k]) for k in so)
        assert torch.equal(lo.samples, ln.samples)
        assert ln.variational_strategy.jitter_val == lo.variational_strategy.jitter_val
        lik, lik_old = getattr(new, f"hidden_layer_likelihood_{l}"), getattr(prev, f"hidden_layer_likelihood_{l}")
        c = lik.raw_noise_constraint
        assert c.lower_bound < float(lik.noise.detach()) < c.upper_bound and bool(torch.isfinite(lik.raw_noise).all())
        want = min(float(lik_old.noise.detach()), c.upper_bound - warm_start.NOISE_MARGIN_HIGH * (c.upper_bound - c.lower_bound))
        assert float(lik.noise.detach()) == pytest.approx(want, rel=1e-9)


def test_noise_is_clipped_strictly_inside_the_new_interval():
    lo, hi = 1e-8, 0.05
    assert lo < warm_start.clip_noise(lo, lo, hi) < 2e-8 and warm_start.clip_noise(1.0, lo, hi) < hi
    assert warm_start.clip_noise(1e-3, lo, hi) == 1e-3


def test_refusals():
    prev, prob = _previous(2, 10)
    x, y, fid = _grown(prob, 1)
    kw = dict(type_lengthscale=TL.ONES, warm_start="posterior")
    with pytest.raises(ValueError, match="previously_trained_model"):
        MFDGP(x, y, fid, 2, **kw)
    perm = torch.arange(x.shape[0])
    perm[0], perm[1] = 1, 0
    with pytest.raises(ValueError, match="row 0 differs"):
        MFDGP(x[perm], y[perm], fid[perm], 2, previously_trained_model=prev, **kw)
    changed = x.clone()
    changed[4, 1] = torch.nextafter(changed[4, 1], torch.tensor(2.0, dtype=torch.float64))      # one bit
    with pytest.raises(ValueError, match="row 4 differs"):
        MFDGP(changed, y, fid, 2, previously_trained_model=prev, **kw)
    with pytest.raises(ValueError, match="fewer"):
        MFDGP(x, y, fid, 2, num_inducing=9, previously_trained_model=prev, **kw)
    with pytest.raises(ValueError, match="use_only_highest_fidelity"):
        MFDGP(x, y, fid, 2, use_only_highest_fidelity=True, previously_trained_model=prev, **kw)
    with pytest.raises(ValueError, match="float64"):      # bitwise copies need the previous model in float64
        MFDGP(x, y, fid, 2, previously_trained_model=copy.deepcopy(prev).float(), **kw)
    with pytest.raises(ValueError, match="warm_start must be"):
        MFDGP(x, y, fid, 2, previously_trained_model=prev, type_lengthscale=TL.ONES, warm_start="q")


def test_default_is_unchanged():
    """``warm_start="hypers"`` is today's behaviour: bitwise the parameters of a call without the keyword, same torch seed."""
    prev, prob = _previous(2, 10)
    x, y, fid = _grown(prob, 1)
    models = []
    for kw in ({}, {"warm_start": "hypers"}):
        torch.manual_seed(4)
        models.append(MFDGP(x, y, fid, 2, previously_trained_model=prev, **kw))
    a, b = models[0].state_dict(), models[1].state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    vd = models[1].hidden_layer_0.variational_strategy._variational_distribution
    assert vd.variational_mean.dtype == torch.float32      # and nothing of the posterior mode leaked in
