"""numpy restatement of mobocmf_recommend_scores as include/mobocmf_hip.h states it (written from the header, not from
csrc/recommend.hip): explicit loops over the samples s and the constraints c, one IEEE operation per line, ``math.erfc``; and the
fixture the CPU and the GPU test share.  (The generation loop of util/recommend_evolve.py is ``nsga_reference.evolve`` around an
``evaluate`` made of these scores.)"""
import math
import statistics
import sys

import numpy as np

DBL_MIN = sys.float_info.min
SHAPES = [(1, 0, 1, 1), (2, 1, 5, 1), (2, 2, 64, 3), (3, 2, 66, 25), (16, 16, 7, 2), (1, 3, 130, 48)]      # (n_obj, n_con, T, S)
P_MIN = 0.999


def z_min_of(p_min):
    return statistics.NormalDist().inv_cdf(p_min)


def phi(z):
    """0.5 erfc(-(z / sqrt(2))): the probability the rule compares with p_min."""
    return 0.5 * math.erfc(-(z / 1.4142135623730951))


def model_moments(mu, var, scale=None):
    """(mbar, v) of one model at one test point from its S sample means ``mu`` and noise-free variances ``var``."""
    S = len(mu)
    if S == 1:
        mbar, v = float(mu[0]), float(var[0])
    else:
        a, q = 0.0, 0.0
        for s in range(S):
            ms = float(mu[s])
            a = a + ms
            sq = ms * ms
            q = q + (float(var[s]) + sq)
        mbar = a / S
        sq = mbar * mbar
        v = q / S - sq
    if scale is not None:
        shift, factor = float(scale[0]), float(scale[1])
        mbar = mbar * factor
        mbar = mbar + shift
        v = (v * factor) * factor
    return mbar, v


def constraint_term(mbar, v, p_min, z_min):
    """(z, Phi, viol_c) of one constraint at one test point."""
    with np.errstate(invalid="ignore", divide="ignore"):
        z = float(np.float64(mbar) / np.sqrt(np.float64(v)))
    p = phi(z)
    if v < 0.0 or z != z:
        return z, p, math.inf
    if p > p_min:
        return z, p, 0.0
    return z, p, max(z_min - z, DBL_MIN)


def scores(moments, n_obj, T, S, scale=None, p_min=P_MIN, z_min=None):
    """F (n_obj, T), viol (T,) (zeros without constraints) and, for the tests' preconditions, Phi (n_con, T)."""
    moments = np.asarray(moments, dtype=np.float64)
    n = moments.shape[0]
    n_con = n - n_obj
    z_min = z_min_of(p_min) if z_min is None else z_min
    F, viol, prob = np.zeros((n_obj, T)), np.zeros(T), np.zeros((n_con, T))
    for t in range(T):
        total = 0.0
        for m in range(n):
            mbar, v = model_moments(moments[m, 0, t * S:(t + 1) * S], moments[m, 1, t * S:(t + 1) * S],
                                    None if scale is None else scale[m])
            if m < n_obj:
                F[m, t] = mbar
            else:
                _, prob[m - n_obj, t], w = constraint_term(mbar, v, p_min, z_min)
                total = total + w
        viol[t] = total
    return F, viol, prob


def fixture(n_obj, n_con, T, S):
    """(moments (n, 2, T S), scale (n, 2)): means = 0.3 N(0, 1) per column + 1.5 N(0, 1) per model and test point + 1, variances
    U(0.01, 0.5), scale = (N(0, 1), U(0.5, 2))."""
    rng = np.random.default_rng((n_obj, n_con, T, S))
    n = n_obj + n_con
    means = 0.3 * rng.standard_normal((n, T, S)) + 1.5 * rng.standard_normal((n, T, 1)) + 1.0
    variances = rng.uniform(0.01, 0.5, (n, T, S))
    scale = np.stack((rng.standard_normal(n), rng.uniform(0.5, 2.0, n)), 1)
    return np.ascontiguousarray(np.stack((means.reshape(n, T * S), variances.reshape(n, T * S)), 1)), scale
