"""The part of the one-launch bindings that needs no GPU (util/tiny_step.py): the descriptor builder -- header, trainable bits,
noise bounds, flat-vector segments against mobocmf_tiny_flat_len -- for training and for prediction, and the structural check
both kernels share, on a CPU model."""
import ctypes

import pytest
import torch

from mobocmf_amd import _lib
from mobocmf_amd.util import tiny_step as TS

FID = [2, 2, 1, 1, 1, 0, 0]
NUM_DATA = 21


@pytest.fixture()
def model():
    from mobocmf_amd.models import MFDGP
    from mobocmf_amd.models.mfdgp import TL
    torch.manual_seed(0)
    x = torch.rand(7, 2, dtype=torch.float64)
    y = torch.sin(3.0 * x.sum(1, keepdim=True))
    fid = torch.tensor(FID, dtype=torch.float64)[:, None]
    m = MFDGP(x, y, fid, 3, type_lengthscale=TL.ONES, num_inducing=5, num_samples_for_training=2,
              num_samples_for_acquisition=4).double()
    m.fix_variational_hypers(False)
    layers = m._layers()
    TS._hyper_params(layers[2])[5].requires_grad = False                                        # one lengthscale
    layers[1].variational_strategy._variational_distribution.chol_variational_covar.requires_grad = False
    return m


def test_training_descriptor(model):
    T = _lib.TinyModel()
    desc = TS.Descriptor.for_training(T, model, 2, torch.tensor(FID, dtype=torch.float64), NUM_DATA, natgrad=True)
    assert (T.L, T.M, T.d, T.S, T.N) == (3, 5, 2, 2, 7) and list(T.rows) == [7, 5, 2]
    assert T.kl_scale == 7 / NUM_DATA and T.branch == 0
    layers = model._layers()
    assert T.jitter == layers[0].variational_strategy.jitter_val
    assert T.Zx == desc.keep[0].data_ptr() and torch.equal(desc.keep[0], layers[0].variational_strategy._inducing_points.detach())
    natural = []
    for l, layer in enumerate(layers):
        lik = TS._likelihood(model, l)
        c = lik.raw_noise_constraint
        assert (T.noise_lo[l], T.noise_hi[l]) == (float(c.lower_bound), float(c.upper_bound)) and T.noise_lo[l] < T.noise_hi[l]
        assert T.raw_noise[l] == lik.raw_noise.data_ptr()
        hyper = TS._hyper_params(layer)
        assert len(hyper) == (2 if l == 0 else 7)
        for s, p in enumerate(hyper):
            assert (T.trainable[l] >> s) & 1 == int(p.requires_grad) and T.raw[l][s] == p.data_ptr(), (l, s)
        vd = layer.variational_strategy._variational_distribution
        both = vd.variational_mean.requires_grad and vd.chol_variational_covar.requires_grad
        assert (T.trainable[l] >> 7) & 1 == int(vd.variational_mean.requires_grad and not both)
        assert (T.trainable[l] >> 8) & 1 == int(vd.chol_variational_covar.requires_grad and not both)
        assert (T.trainable[l] >> 9) & 1 == int(lik.raw_noise.requires_grad) == 1
        assert T.m[l] == vd.variational_mean.data_ptr() and T.L_S[l] == vd.chol_variational_covar.data_ptr()
        assert (T.rng[l] is not None) == (l > 0) and T.eps[l] is None      # (a NULL pointer reads as None)
        if both:
            natural.append(l)
    assert natural == [0, 2] == [k[0] for k in desc.natural]
    assert (T.trainable[1] >> 7) & 3 == 1                      # layer 1: m stays with Adam, L_S is frozen
    assert (T.trainable[2] >> 5) & 1 == 0 and T.trainable[2] & 0x5F == 0x5F      # the frozen lengthscale, and only it
    # the flat vector: per layer [hyper-parameters | m | L_S], then the noise parameters; contiguous, as long as the library says
    off = 0
    for p, o, n in desc.segments:
        assert o == off and n == p.numel()
        off += n
    flat = ctypes.c_int64()
    assert _lib.load().mobocmf_tiny_flat_len(ctypes.byref(T), ctypes.byref(flat)) == _lib.OK
    assert off == flat.value == desc.flat_len == (1 + 2) + 2 * (5 + 4) + 3 * (5 + 25) + 3
    at = {o: p for p, o, _ in desc.segments}
    for l, M, om, oL in desc.natural:      # where the natural-gradient launch finds the gradients of m and L_S
        vd = layers[l].variational_strategy._variational_distribution
        assert M == 5 and at[om] is vd.variational_mean and at[oL] is vd.chol_variational_covar
    # without natural gradients every trainable q(u) tensor is Adam's
    T2 = _lib.TinyModel()
    assert TS.Descriptor.for_training(T2, model, 2, torch.tensor(FID), NUM_DATA).natural == []
    assert [(T2.trainable[l] >> 7) & 3 for l in range(3)] == [3, 1, 3]


def test_prediction_descriptor(model):
    T = _lib.TinyModel()
    desc = TS.Descriptor.for_prediction(T, model, 1, 3, 2)
    assert (T.L, T.M, T.d, T.S, T.N) == (2, 5, 2, 4, 3) and list(T.rows) == [3, 3, 0]
    assert T.branch == 1 and T.kl_scale == 0.0
    assert list(T.trainable) == [0, 0, 0]                      # nothing is updated on the eval branch
    samples = model._layers()[1].samples.reshape(-1).to(torch.float64)
    assert samples.numel() == 4 and torch.equal(desc.eps[1], torch.cat([samples] * 3)) and T.eps[1] == desc.eps[1].data_ptr()
    assert desc.eps[0] is None and T.eps[0] is None and T.rng[1] is None
    assert desc.flat_len == (1 + 2) + (5 + 4) + 2 * (5 + 25) + 2
    T0 = _lib.TinyModel()
    TS.Descriptor.for_prediction(T0, model, 0, 3, 2)
    assert (T0.L, T0.S) == (1, 1) and list(T0.rows) == [3, 0, 0]


def test_structural_check(model):
    fits = lambda training, L: TS.structure_fits(model, L, 2, _lib.TINY_MAX_M, training=training, on_gpu=False)
    assert fits(True, 3) and fits(True, None) and fits(False, 3) and fits(False, 2)
    assert not TS.structure_fits(model, 3, 2, _lib.TINY_MAX_M, training=False)           # parameters on the GPU are the default
    assert not TS.structure_fits(model, 3, 2, 4, training=False, on_gpu=False)            # M = 5 inducing points
    assert not TS.structure_fits(model, 3, 3, _lib.TINY_MAX_M, training=False, on_gpu=False)
    model.eval_mode()
    assert not fits(True, 3) and fits(False, 3)
    model.train_mode()
    assert fits(True, 3)
    with torch.no_grad():
        model._layers()[2].variational_strategy._inducing_points[0, 0] += 1e-3
    assert not fits(True, 3) and not fits(False, 3) and fits(False, 2)
