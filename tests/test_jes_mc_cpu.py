"""JES averaged over K sampled Pareto sets, on the host: the restatement of mobocmf_jes_mc_group_forward
(tests/jes_mc_reference.py) against torch.autograd and against the single-sample restatement, and ``_JES_MFDGP`` with several
conditioned models.  No GPU."""
import pytest
import torch

from tests import acq_search_reference as R1
from tests import jes_mc_reference as R

SHAPES = [(1, 1, 1, 1), (3, 1, 5, 4), (1, 3, 1, 1), (2, 4, 5, 4), (3, 2, 67, 1), (2, 8, 200, 5)]


def _bits(t):
    return t.detach().contiguous().view(torch.int64)


@pytest.mark.parametrize("n_boxes,K,T,S", SHAPES)
def test_seeds_are_the_autograd_gradient(n_boxes, K, T, S):
    for flip in range(4):
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=10 * T + S + K, flip=flip)
        acq, seeds, _ = R.jes_mc_group_forward(mom, noise, K, T, S)
        m = mom.clone().requires_grad_(True)
        val = R.jes_mc_value(m, noise, K, T, S)
        assert float((val.detach() - acq).abs().max()) <= 1e-14 * float(acq.abs().max().clamp_min(1.0))
        val.sum().backward()
        assert float((seeds - m.grad).abs().max()) <= 1e-13 * float(m.grad.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("n_boxes,K,T,S", [s for s in SHAPES if s[1] >= 2])
def test_inputs_visit_none_some_and_all_samples_passing(n_boxes, K, T, S):
    seen = [set() for _ in range(n_boxes)]
    for flip in range(4):
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=10 * T + S + K, flip=flip)
        count = R.passing(mom, noise, K, T, S).sum(1)      # (n_boxes, T)
        for p in range(n_boxes):
            kinds = {"none" if c == 0 else "all" if c == K else "some" for c in count[p].tolist()}
            assert T < 4 or kinds == {"none", "some", "all"}, (p, flip, kinds)
            seen[p] |= kinds
    assert all(s == {"none", "some", "all"} for s in seen), seen


@pytest.mark.parametrize("n_pairs,T,S", [(1, 1, 1), (3, 5, 4), (2, 67, 1), (3, 200, 5)])
def test_one_sample_is_the_pair_restatement_bitwise(n_pairs, T, S):
    kinds = set()
    for flip in range(2):
        mom, noise = R.mc_inputs(n_pairs, 1, T, S, seed=T + S, flip=flip)
        acq, seeds, scale = R.jes_mc_group_forward(mom, noise, 1, T, S)
        acq1, seeds1, scale1 = R1.jes_group_forward(mom, noise, T, S)
        assert torch.equal(_bits(acq), _bits(acq1)) and torch.equal(_bits(seeds), _bits(seeds1))
        assert float(((scale - scale1) / scale1).abs().max()) <= 1e-15      # (a bound's scale: summed in another order)
        kinds |= set((seeds1[0::2, 1] > 0.0).reshape(-1).tolist())
    assert kinds == {True, False}      # both sides of the clamp


@pytest.mark.parametrize("K", [2, 3, 8])
def test_identical_conditioned_models_give_the_one_sample_value(K):
    n_boxes, T, S = 3, 7, 4
    mom1, noise1 = R.mc_inputs(n_boxes, 1, T, S, seed=3, flip=0)
    idx = torch.tensor([2 * p + (1 if j else 0) for p in range(n_boxes) for j in range(1 + K)])
    mom, noise = mom1[idx], noise1[idx]
    acq1, seeds1, _ = R1.jes_group_forward(mom1, noise1, T, S)
    acq, seeds, _ = R.jes_mc_group_forward(mom, noise, K, T, S)
    assert bool((acq1 > 0.0).any())
    # K equal terms are summed and the sum is scaled by 1/K: K - 1 additions and one product, each within half an ulp
    assert float((acq - acq1).abs().max()) <= (K + 1) * 2.0 ** -53 * float(acq1.abs().max())
    su = seeds.reshape(n_boxes, 1 + K, 2, T * S)
    s1 = seeds1.reshape(n_boxes, 2, 2, T * S)
    assert float((su[:, 0] - s1[:, 0]).abs().max()) <= 4 * 2.0 ** -53 * float(s1[:, 0].abs().max())
    for k in range(1, K + 1):      # each copy carries 1/K of the conditioned model's gradient
        assert float((K * su[:, k] - s1[:, 1]).abs().max()) <= 4 * 2.0 ** -53 * float(s1[:, 1].abs().max())


def test_group_value_at_one_sample_is_the_pair_expression_bitwise():
    """JESMOC_MFDGP._group_value has one expression for every K; at K = 1 -- also on an object made with __new__, which has the
    class default -- it is the pair expression bit for bit, value and gradient (1.0 * the single term is exact, and so is the
    product of the incoming gradient with 1.0).  200 random cases: 2 .. 10 models, T in 1 .. 40, v over twenty decades."""
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP
    acq = JESMOC_MFDGP.__new__(JESMOC_MFDGP)
    assert acq.num_pareto_samples == 1 and "num_pareto_samples" not in acq.__dict__
    g = torch.Generator().manual_seed(5)
    clamped = set()
    for case in range(200):
        n = 2 * int(torch.randint(1, 6, (1,), generator=g))
        T = int(torch.randint(1, 41, (1,), generator=g))
        v = 10.0 ** (20.0 * torch.rand(n, T, dtype=torch.float64, generator=g) - 10.0)
        w = torch.randn(T, dtype=torch.float64, generator=g)      # (a gradient other than ones flows in)
        va, vb = v.clone().requires_grad_(True), v.clone().requires_grad_(True)
        got = acq._group_value(va)
        want = (0.5 * torch.clamp(torch.log(vb[0::2]) - torch.log(vb[1::2]), min=0.0)).sum(0)
        (got * w).sum().backward()
        (want * w).sum().backward()
        assert got.shape == (T,) and torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(va.grad), _bits(vb.grad)), case
        clamped |= set((va.grad == 0.0).reshape(-1).tolist())
    assert clamped == {True, False}      # both sides of the clamp


class _Stub:
    """A model whose predict_for_acquisition returns a fixed variance; counts its evaluations and mode switches."""

    def __init__(self, v):
        self.v, self.calls, self.modes = v, 0, []

    def predict_for_acquisition(self, X, fidelity):
        self.calls += 1
        assert self.modes[-1] == "eval"
        return torch.zeros_like(self.v), self.v

    def eval(self):
        self.modes.append("eval")

    def train(self):
        self.modes.append("train")


def test_jes_mfdgp_is_the_mean_over_the_conditioned_models(monkeypatch):
    from mobocmf_amd import functional as F
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import _JES_MFDGP
    monkeypatch.setattr(F, "jes", lambda vu, vc: 0.5 * torch.clamp(torch.log(vu) - torch.log(vc), min=0.0))
    g = torch.Generator().manual_seed(0)
    vu = 0.5 + torch.rand(9, dtype=torch.float64, generator=g)
    vcs = [0.25 + 1.5 * torch.rand(9, dtype=torch.float64, generator=g) for _ in range(3)]
    u, cs = _Stub(vu), [_Stub(v) for v in vcs]
    jes = _JES_MFDGP(1, u, cs)
    out = jes(torch.zeros(9, 2, dtype=torch.float64))
    terms = [0.5 * torch.clamp(torch.log(vu) - torch.log(v), min=0.0) for v in vcs]
    want = (1.0 / 3) * ((terms[0] + terms[1]) + terms[2])
    assert torch.equal(_bits(out), _bits(want))
    assert bool((terms[0] == 0.0).any()) and bool((terms[0] > 0.0).any())      # both sides of the clamp
    assert u.calls == 1 and all(c.calls == 1 for c in cs)                       # the unconditioned model ONCE
    assert all(m.modes == ["eval", "train"] for m in [u] + cs)
    assert jes.mfdgp_conds == cs and jes.mfdgp_cond is cs[0]
    one = _JES_MFDGP(1, _Stub(vu), _Stub(vcs[1]))                               # a single model: K = 1, as ever
    assert one.mfdgp_conds == [one.mfdgp_cond]
    assert torch.equal(_bits(one(torch.zeros(9, 2, dtype=torch.float64))), _bits(terms[1]))
    with pytest.raises(ValueError):
        _JES_MFDGP(1, u, [])


def test_limits_are_refused_before_any_model_is_touched(monkeypatch):
    from mobocmf_amd import parallel
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    with pytest.raises(ValueError, match="num_pareto_samples"):
        JESMOC_MFDGP(None, num_pareto_samples=0)
    with pytest.raises(ValueError):
        BlackBoxMFDGPFitter.conditioned_copies(None, 0)
    monkeypatch.setattr(parallel, "_no_group", lambda: False)      # as with surrogates sharded over a process group
    with pytest.raises(ValueError, match="one process"):
        JESMOC_MFDGP(None, num_pareto_samples=2)
    with pytest.raises(ValueError, match="one process"):
        JESMOC_MFDGP(None, model_cond=[object(), object()])
    with pytest.raises(ValueError, match="one process"):
        BlackBoxMFDGPFitter.conditioned_copies(None, 2)


def test_pareto_sample_seeds():
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    seed = BlackBoxMFDGPFitter._pareto_sample_seed
    assert seed(None, 0) is None and seed(None, 3) is None      # unseeded: the process generators, in order
    assert seed(7, 0) == 7                                       # one sample: the plain seeded call
    others = [seed(7, k) for k in range(1, 9)]
    assert len(set(others + [7])) == 9 and all(0 <= s < 2 ** 62 for s in others)
    assert others == [seed(7, k) for k in range(1, 9)] and seed(8, 1) != seed(7, 1)
