"""Portable chain samples (layers.rff.RFFChainSample) on the host: the same function as the per-layer callables of
``sample_function_from_each_layer``, bitwise pack / unpack round trips, pickling, per-black-box draws that do not depend on
the order of visits, and the sample exchange without a process group."""
import copy

import numpy as np
import pytest
import torch

from mobocmf_amd.layers import rff
from mobocmf_amd.util import synthetic


def _model(d, L, seed=0):
    prob = synthetic.make_problem(d=d, L=L, M=10, N=30, S=1, seed=seed)
    return synthetic.model_from_problem(prob, device="cpu")


@pytest.mark.parametrize("d,L,F", [(2, 2, 64), (3, 3, 40), (8, 2, 50)])
def test_chain_sample_is_the_top_layer_sample(d, L, F):
    model = _model(d, L, seed=d)
    f = model.sample_function_from_each_layer(nFeatures=F, generator=torch.Generator().manual_seed(3))[-1]
    c = rff.sample_chain_from_posterior(model, nFeatures=F, generator=torch.Generator().manual_seed(3))
    assert c.device is None and len(c.layers) == L and c.d == d and c.F == F
    X = np.random.default_rng(1).random((37, d))
    ref = f(X)
    assert np.abs(c(X) - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    for p in X[:3]:
        g_ref = f(p, gradient=True)
        assert np.abs(c(p, gradient=True) - g_ref).max() <= 1e-12 * max(1.0, np.abs(g_ref).max())
    xt = torch.as_tensor(X)
    assert torch.allclose(c._torch(xt), f._torch(xt), rtol=1e-12, atol=1e-12)
    assert callable(c._device)


@pytest.mark.parametrize("d,L", [(2, 2), (3, 3), (5, 1)])
def test_pack_unpack_round_trip_is_bitwise(d, L):
    model = _model(d, max(L, 2), seed=1)
    c = rff.sample_chain_from_posterior(model, nFeatures=33, generator=torch.Generator().manual_seed(0))
    c.layers = c.layers[:L]                                   # a one-layer chain packs too
    buf = c.pack()
    assert buf.dtype == torch.float64 and buf.dim() == 1 and buf.numel() == rff.packed_length(L, d, 33)
    assert rff.RFFChainSample.header(buf) == (rff.PACK_VERSION, L, d, 33, buf.numel())
    padded = torch.cat([buf, torch.full((17,), float("nan"), dtype=torch.float64)])       # padding after the length
    for c2 in (rff.RFFChainSample.unpack(buf), rff.RFFChainSample.unpack(padded)):
        X = np.random.default_rng(2).random((29, d))
        assert np.array_equal(c2(X), c(X))
        assert np.array_equal(c2(X[4], gradient=True), c(X[4], gradient=True))
        assert torch.equal(c2._torch(torch.as_tensor(X)), c._torch(torch.as_tensor(X)))
        assert torch.equal(c2.pack(), buf)
    with pytest.raises(ValueError):
        rff.RFFChainSample.unpack(buf[:-1])
    bad = buf.clone()
    bad[0] = 99.0
    with pytest.raises(ValueError):
        rff.RFFChainSample.unpack(bad)


def test_payload_formula():
    # 2 layers at F = 500, d = 8: F (d + 2) + F (2 d + 6) doubles plus a 21-double header, about 128 KB
    n = rff.packed_length(2, 8, 500)
    assert n == 500 * 10 + 500 * 22 + 5 + 2 + 14
    assert 127_000 < 8 * n < 129_000


def test_chain_sample_survives_deepcopy_and_dill():
    import dill
    c = rff.sample_chain_from_posterior(_model(2, 2), nFeatures=48, generator=torch.Generator().manual_seed(5))
    X = np.random.default_rng(3).random((11, 2))
    for c2 in (copy.deepcopy(c), dill.loads(dill.dumps(c))):
        assert np.array_equal(c2(X), c(X))
        assert np.array_equal(c2(X[0], gradient=True), c(X[0], gradient=True))
        assert torch.equal(c2.pack(), c.pack())


def _fitter(order):
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter, MFDGPHandler
    fitter = BlackBoxMFDGPFitter(2, 12, device="cpu")
    for name, is_con, gi, seed in order:
        h = MFDGPHandler.__new__(MFDGPHandler)
        h.mfdgp, h.global_index = _model(2, 2, seed=seed), gi
        (fitter.mfdgp_handlers_cons if is_con else fitter.mfdgp_handlers_objs)[name] = h
    return fitter


def test_per_blackbox_draws_do_not_depend_on_the_visit_order():
    bbs = [("a", False, 0, 0), ("b", False, 1, 1), ("c", True, 0, 2), ("d", True, 1, 3)]
    got = []
    for order in (bbs, bbs[::-1], [bbs[1], bbs[3], bbs[0], bbs[2]]):
        bufs, idx, roles = _fitter(order)._draw_chain_samples(seed=11, t=2, nFeatures=32)
        got.append({(r, i): b for b, i, r in zip(bufs, idx, roles)})
    for g in got[1:]:
        assert g.keys() == got[0].keys()
        for k in g:
            assert torch.equal(g[k], got[0][k])
    # the generator depends on the seed, role, index and try: any change gives another sample
    fb = _fitter(bbs)
    base = fb._draw_chain_samples(seed=11, t=2, nFeatures=32)[0][0]
    assert not torch.equal(fb._draw_chain_samples(seed=12, t=2, nFeatures=32)[0][0], base)
    assert not torch.equal(fb._draw_chain_samples(seed=11, t=3, nFeatures=32)[0][0], base)


def test_all_gather_samples_without_a_group_is_the_identity():
    from mobocmf_amd import parallel
    bufs = [torch.arange(5, dtype=torch.float64) + 10 * k for k in range(3)]
    out = parallel.all_gather_samples(bufs, [2, 0, 1])
    assert [torch.equal(o, bufs[k]) for o, k in zip(out, [1, 2, 0])] == [True] * 3
    objs, cons = parallel.all_gather_samples(bufs, [0, 0, 1], roles=[0, 1, 1])
    assert len(objs) == 1 and torch.equal(objs[0], bufs[0])
    assert torch.equal(cons[0], bufs[1]) and torch.equal(cons[1], bufs[2])
    assert parallel.all_gather_samples([], []) == []
    with pytest.raises(ValueError, match="permutation"):
        parallel.all_gather_samples(bufs, [0, 0, 1])
    with pytest.raises(ValueError, match="one global index"):
        parallel.all_gather_samples(bufs, [0, 1])
    with pytest.raises(RuntimeError, match="failed"):
        parallel.all_gather_samples([], [], local_error=ValueError("boom"))
