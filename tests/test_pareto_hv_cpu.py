"""Host side of the recommendation and its score: a numpy hypervolume oracle (inclusion-exclusion for few points, recursive
slicing otherwise) checked against known answers, the random baseline Random_choice, and HV / recommend refusing to run
without a device (the product path has no CPU fallback)."""
import itertools

import numpy as np
import pytest
import torch

from mobocmf_amd import _lib


# ------------------------------------------------------------------ numpy hypervolume oracle (minimisation)
def _relevant(pts, ref):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, len(ref))
    return pts[np.all(pts <= ref, axis=1)]


def hv_inclusion_exclusion(pts, ref):
    """Sum over the non-empty subsets S of (-1)^(|S|+1) vol(intersection of the boxes [p, ref], p in S)."""
    ref = np.asarray(ref, dtype=np.float64)
    pts = _relevant(pts, ref)
    assert pts.shape[0] <= 10
    total = 0.0
    for r in range(1, pts.shape[0] + 1):
        for S in itertools.combinations(range(pts.shape[0]), r):
            total += (-1.0) ** (r + 1) * float(np.prod(ref - pts[list(S)].max(0)))
    return total


def _hv2(pts, ref):
    if pts.shape[0] == 0:
        return 0.0
    o = np.lexsort((pts[:, 1], pts[:, 0]))
    x, y = pts[o, 0], np.minimum.accumulate(pts[o, 1])
    dx = np.diff(np.append(x, ref[0]))
    return float(np.sum(dx * (ref[1] - y)))


def _hv_slice(pts, ref):
    k = pts.shape[1]
    if pts.shape[0] == 0:
        return 0.0
    if k == 1:
        return float(ref[0] - pts[:, 0].min())
    if k == 2:
        return _hv2(pts, ref)
    o = np.argsort(pts[:, -1], kind="stable")
    p = pts[o]
    z = np.append(p[:, -1], ref[-1])
    total = 0.0
    for i in range(p.shape[0]):
        h = z[i + 1] - z[i]
        if h > 0:
            total += h * _hv_slice(p[:i + 1, :-1], ref[:-1])
    return total


def hv_slicing(pts, ref):
    """Recursive slicing along the last objective: the slab between consecutive values times the (k-1)-dimensional volume of
    the points below it."""
    ref = np.asarray(ref, dtype=np.float64)
    return _hv_slice(_relevant(pts, ref), ref)


def hv_oracle(pts, ref):
    pts = _relevant(pts, np.asarray(ref, dtype=np.float64))
    return hv_inclusion_exclusion(pts, ref) if pts.shape[0] <= 10 else hv_slicing(pts, ref)


def test_oracle_single_box():
    ref = np.array([3.0, 5.0, 2.0])
    p = np.array([[1.0, 1.0, 0.5]])
    assert hv_inclusion_exclusion(p, ref) == pytest.approx(2.0 * 4.0 * 1.5, rel=1e-15)
    assert hv_slicing(p, ref) == pytest.approx(12.0, rel=1e-15)
    assert hv_oracle(np.array([[4.0, 0.0, 0.0]]), ref) == 0.0          # does not dominate ref: nothing
    assert hv_oracle(np.zeros((0, 3)), ref) == 0.0


def test_oracle_2d_staircase():
    # (1, 3), (2, 2), (3, 1) against (4, 4): 3 + 2 + 1 columns of heights 1, 2, 3 -> 1*3 + 1*2 + 1*1 ... by hand:
    # x in [1, 2): height 4 - 3 = 1; [2, 3): 4 - 2 = 2; [3, 4): 4 - 1 = 3  ->  6
    pts = np.array([[1.0, 3.0], [2.0, 2.0], [3.0, 1.0], [2.5, 2.5], [2.0, 2.0]])    # a dominated point and a duplicate
    assert hv_inclusion_exclusion(pts, [4.0, 4.0]) == pytest.approx(6.0, rel=1e-15)
    assert hv_slicing(pts, [4.0, 4.0]) == pytest.approx(6.0, rel=1e-15)


@pytest.mark.parametrize("k,P", [(3, 7), (4, 9), (5, 6)])
def test_oracle_forms_agree(k, P):
    rng = np.random.default_rng(k * 10 + P)
    pts = rng.uniform(size=(P, k))
    ref = np.full(k, 1.1)
    assert hv_slicing(pts, ref) == pytest.approx(hv_inclusion_exclusion(pts, ref), rel=1e-12)


def test_oracle_monte_carlo_k5():
    rng = np.random.default_rng(5)
    pts = rng.uniform(0.1, 0.9, size=(8, 5))
    ref = np.ones(5)
    lo = pts.min(0)
    box = float(np.prod(ref - lo))
    N = 1_000_000
    hits = 0
    for b in range(0, N, 200_000):
        s = rng.uniform(lo, ref, size=(200_000, 5))
        hits += int(np.any(np.all(pts[None, :, :] <= s[:, None, :], axis=2), axis=1).sum())
    frac = hits / N
    est, sigma = box * frac, box * np.sqrt(frac * (1 - frac) / N)
    exact = hv_inclusion_exclusion(pts, ref)
    assert abs(est - exact) < 5 * sigma
    assert hv_slicing(pts, ref) == pytest.approx(exact, rel=1e-12)


# ------------------------------------------------------------------ Random_choice
def _random_choice(seed):
    from mobocmf_amd.acquisition_functions.Random_choice import Random_choice
    rc = Random_choice(input_size=3, num_fidelities=2, seed=seed)
    for f in range(2):
        for name in ("obj1", "obj2", "con1"):
            rc.add_blackbox(f, name, cost_evaluation=1.0 if f == 0 else 10.0)
    return rc


def test_random_choice_surface():
    rc = _random_choice(0)
    assert rc.input_size == 3 and rc.num_fidelities == 2 and rc.seed == 0
    assert rc.costs_blackboxes[0] == {"total": 0.0, "obj1": 1.0, "obj2": 1.0, "con1": 1.0}
    assert rc.costs_blackboxes[1]["con1"] == 10.0
    assert torch.equal(rc.coupled_costs_fidelities, torch.tensor([3.0, 30.0])) and rc.total_cost_fidelities == 33.0
    X = torch.zeros(5, 3)
    assert rc.coupled_acq(X, 0).shape == (5,) and rc.decoupled_acq(X, 1, "obj1").shape == (5,)
    x, f = rc.get_nextpoint_coupled(iteration=0)
    assert x.shape == (3,) and bool(((x >= 0) & (x < 1)).all()) and f in (0, 1) and isinstance(f, int)


def test_random_choice_seeded_and_unseeded():
    a, b = _random_choice(7), None
    xa = [a.get_nextpoint_coupled() for _ in range(5)]
    b = _random_choice(7)
    xb = [b.get_nextpoint_coupled() for _ in range(5)]
    assert all(torch.equal(p[0], q[0]) and p[1] == q[1] for p, q in zip(xa, xb))
    torch.manual_seed(123)
    state = torch.get_rng_state()
    _random_choice(None)                       # the reference's torch.manual_seed(None) raises; here the generator stays
    assert torch.equal(torch.get_rng_state(), state)


def test_random_choice_fidelity_frequencies():
    rc = _random_choice(11)
    N = 20000
    hits = sum(rc.get_nextpoint_coupled()[1] for _ in range(N))
    w = 1.0 - np.array([3.0, 30.0]) / 33.0
    p1 = w[1] / w.sum()
    assert abs(hits / N - p1) < 5 * np.sqrt(p1 * (1 - p1) / N)


# ------------------------------------------------------------------ no device: loud failure
def _no_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_lib, "_arch_checked", False)


def test_hv_raises_without_device(monkeypatch):
    from mobocmf_amd.util.hypervolume import HV
    _no_device(monkeypatch)
    with pytest.raises(_lib.MobocmfError):
        HV(ref_point=np.array([1000.0, 1000.0]))(np.array([[1.0, 2.0], [2.0, 1.0]]))


def test_recommend_raises_without_device(monkeypatch):
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    _no_device(monkeypatch)
    with pytest.raises(_lib.MobocmfError):
        BlackBoxMFDGPFitter(2, 10, device="cpu").recommend(np.random.default_rng(0).uniform(size=(20, 2)))
