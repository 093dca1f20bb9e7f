"""The protocol the four predict groups share (util/predict_group.py PredictGroup): TinyPredictGroup, CoopPredictGroup,
PanelPredictGroup and SplitPredictGroup answer ``why_not`` and take ``freeze()`` / ``thaw()`` / ``frozen()`` unconditionally,
which is how JESMOC_MFDGP and DeviceAcqSearch drive them."""
import pytest
import torch

from mobocmf_amd.util import synthetic
from tests.test_hip_model import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, D, S = 5, 2, 5


def _bits(t):
    return t.detach().contiguous().view(torch.int64)


def _classes():
    from mobocmf_amd.util.coop_step import CoopPredictGroup
    from mobocmf_amd.util.panel_predict import PanelPredictGroup, SplitPredictGroup
    from mobocmf_amd.util.tiny_step import TinyPredictGroup
    return {TinyPredictGroup: 8, CoopPredictGroup: 8, PanelPredictGroup: 130, SplitPredictGroup: 130}      # class -> M


_made = {}


def _models(M):
    if M not in _made:
        N = max(M, 12)      # (M = 8: twelve points, the smoke run's problem; eight leave the initial covariance singular)
        _made[M] = [build_model(synthetic.make_problem(d=D, L=2, M=M, N=N, S=S, seed=s), S_train=1, S_acq=S) for s in (1, 2)]
    return _made[M]


def test_moments_inside_frozen_are_the_moments_outside():
    from mobocmf_amd.util.tiny_step import TinyPredictGroup
    grp = TinyPredictGroup(_models(8), 1, T, D)
    X = torch.rand(T, D, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(DEV)
    outside = grp.moments_at(X)
    with grp.frozen() as inside_grp:
        assert inside_grp is grp
        inside = grp.moments_at(X)
    again = grp.moments_at(X)
    assert outside.shape == (2, 2, T * S) and bool(torch.isfinite(outside).all()) and float(outside[:, 1].min()) > 0.0
    assert torch.equal(_bits(inside), _bits(outside)) and torch.equal(_bits(again), _bits(outside))


@pytest.mark.parametrize("name", ["TinyPredictGroup", "CoopPredictGroup", "PanelPredictGroup", "SplitPredictGroup"])
def test_every_group_is_a_predict_group_and_thaw_without_freeze_is_harmless(name):
    from mobocmf_amd import _lib
    from mobocmf_amd.util.predict_group import PredictGroup
    cls, M = next((c, m) for c, m in _classes().items() if c.__name__ == name)
    models = _models(M)
    other = _models(130 if M == 8 else 8)      # the panel kernels start past M = 128, the one-launch kernels end there
    assert issubclass(cls, PredictGroup)
    for f in (0, 1):
        assert all(cls.why_not(m, f, T, D) is None for m in models)
        assert all(isinstance(cls.why_not(m, f, T, D), str) for m in other)
    assert isinstance(cls.why_not(object(), 1, T, D), str)      # not a model at all
    with pytest.raises(_lib.MobocmfError, match="does not fit"):      # the constructor's gate is the class's why_not
        cls(other, 1, T, D)
    grp = cls(models, 1, T, D)
    X = torch.rand(T, D, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).to(DEV)
    grp.thaw()                      # nothing was frozen
    first = grp.moments_at(X)
    grp.thaw()
    grp.thaw()
    second = grp.moments_at(X)
    with grp.frozen():
        third = grp.moments_at(X)
        fourth = grp.moments_at(X)      # (a cooperative group reuses its chains here: STEP_CHAIN_VALID)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(first).all()) and not any(bool(w.any()) for w in grp.info_words)
    assert torch.equal(_bits(second), _bits(first)) and torch.equal(_bits(third), _bits(first))
    assert torch.equal(_bits(fourth), _bits(first))
