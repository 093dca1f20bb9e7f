"""The restatement of mobocmf_recommend_scores (tests/recommend_reference.py) against closed forms: what the GPU test holds the
kernel to is itself checked here, without a GPU."""
import math
import statistics

import numpy as np
import pytest

from tests import recommend_reference as RR

CASES = [(shape, scaled) for shape in RR.SHAPES for scaled in (False, True)]


def test_one_sample_passes_the_moments_through():
    mom, _ = RR.fixture(2, 2, 64, 1)
    F, _, _ = RR.scores(mom, 2, 64, 1)
    assert np.array_equal(F, mom[:2, 0])
    for m in range(4):
        for t in (0, 17, 63):
            assert RR.model_moments(mom[m, 0, t:t + 1], mom[m, 1, t:t + 1]) == (mom[m, 0, t], mom[m, 1, t])


def test_constant_sample_has_the_variance_of_its_columns():
    # dyadic values: every sum and product below is exact
    for S in (2, 4, 8):
        assert RR.model_moments([1.5] * S, [0.25] * S) == (1.5, 0.25)
        assert RR.model_moments([-0.75] * S, [2.0] * S) == (-0.75, 2.0)
    # a spread of the means adds their variance: means -1, 1 -> mbar 0, v = var + 1
    assert RR.model_moments([-1.0, 1.0], [0.5, 0.5]) == (0.0, 1.5)
    # scale: mean * factor + shift, variance * factor^2
    assert RR.model_moments([1.5] * 4, [0.25] * 4, (0.5, 2.0)) == (3.5, 1.0)


def test_positive_factor_leaves_z_unchanged():
    z_min = RR.z_min_of(RR.P_MIN)
    rng = np.random.default_rng(1)
    for _ in range(50):
        mu, var = rng.standard_normal(5) + 1.0, rng.uniform(0.01, 0.5, 5)
        m0, v0 = RR.model_moments(mu, var)
        z0, _, w0 = RR.constraint_term(m0, v0, RR.P_MIN, z_min)
        m4, v4 = RR.model_moments(mu, var, (0.0, 4.0))      # a power of two: exact
        assert RR.constraint_term(m4, v4, RR.P_MIN, z_min) == RR.constraint_term(m0, v0, RR.P_MIN, z_min)
        mf, vf = RR.model_moments(mu, var, (0.0, 1.7))
        zf, _, wf = RR.constraint_term(mf, vf, RR.P_MIN, z_min)
        assert abs(zf - z0) <= 4 * np.spacing(abs(z0)) and (wf == 0.0) == (w0 == 0.0)


def test_degenerate_variances():
    z_min = RR.z_min_of(RR.P_MIN)
    assert RR.constraint_term(5.0, -1e-3, RR.P_MIN, z_min)[2] == math.inf          # v < 0
    assert RR.constraint_term(0.0, 0.0, RR.P_MIN, z_min)[2] == math.inf            # 0 / 0
    assert RR.constraint_term(1e-300, 0.0, RR.P_MIN, z_min)[2] == 0.0              # v == 0: the sign of the mean decides
    assert RR.constraint_term(-1e-300, 0.0, RR.P_MIN, z_min)[2] == math.inf
    assert RR.constraint_term(math.nan, 1.0, RR.P_MIN, z_min)[2] == math.inf
    # an infeasible row is never graded 0, however close z is to z_min
    z = z_min * (1.0 - 1e-16)
    assert RR.phi(z) <= RR.P_MIN and RR.constraint_term(z, 1.0, RR.P_MIN, z_min)[2] >= RR.DBL_MIN
    # the violations add up in the order of the constraints, from 0.0
    mom = np.array([[[0.0], [1.0]], [[1.0], [1.0]], [[2.0], [1.0]], [[9.0], [1.0]]])
    _, viol, _ = RR.scores(mom, 1, 1, 1)
    assert viol[0] == ((0.0 + (z_min - 1.0)) + (z_min - 2.0)) + 0.0


@pytest.mark.parametrize("shape,scaled", CASES)
def test_feasibility_is_the_rule_of_pareto_mask(shape, scaled):
    """viol == 0 exactly where Phi(m / sqrt(v)) > p_min for every constraint (functional.pareto_mask's docstring with noise-free
    variances), the moments formed by vectorised numpy and Phi by the statistics module."""
    n_obj, n_con, T, S = shape
    mom, scale = RR.fixture(*shape)
    F, viol, prob = RR.scores(mom, n_obj, T, S, scale if scaled else None)
    assert prob.size == 0 or np.abs(prob - RR.P_MIN).min() > 1e-9      # the precondition of this and of the GPU test
    mu, var = mom[:, 0].reshape(-1, T, S), mom[:, 1].reshape(-1, T, S)
    mbar = mu.mean(2)
    v = (var + mu * mu).mean(2) - mbar * mbar
    if scaled:
        mbar, v = mbar * scale[:, 1:] + scale[:, :1], v * scale[:, 1:] ** 2
    assert np.allclose(F, mbar[:n_obj], rtol=1e-13, atol=1e-13)
    cdf = np.vectorize(statistics.NormalDist().cdf)
    want = np.ones(T, dtype=bool)
    if n_con:
        want = (cdf(mbar[n_obj:] / np.sqrt(v[n_obj:])) > RR.P_MIN).all(0)
    assert np.array_equal(viol == 0.0, want)
    assert np.all(viol >= 0.0) and np.all(np.isfinite(viol))


def test_fixture_holds_feasible_and_infeasible_rows():
    mixed = 0
    for shape in RR.SHAPES:
        _, viol, _ = RR.scores(RR.fixture(*shape)[0], shape[0], shape[2], shape[3])
        mixed += bool((viol == 0.0).any() and (viol > 0.0).any())
    assert mixed >= 2
