"""mobocmf_rff_eval_chains / mobocmf_rff_feasibility: K chain samples on a grid in one launch against the per-layer kernel
(mobocmf_rff_eval) and the CPU oracle's feature matrices, determinism, the feasibility rule against numpy, argument
checks, and MOOP on the batched path against the per-callable path for the same samples."""
import ctypes

import numpy as np
import pytest
import torch

from mobocmf_amd.util import synthetic
from oracle import rff_oracle as RO

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _chains(d, L, F, K, seed=0):
    """K chain samples (RFFChainSample on the GPU) of two models of depth L, different generators."""
    from mobocmf_amd.layers import rff
    models = [synthetic.model_from_problem(synthetic.make_problem(d=d, L=L, M=10, N=30, S=1, seed=seed + j), device=DEV)
              for j in range(2)]
    return [rff.sample_chain_from_posterior(models[k % 2], nFeatures=F, generator=torch.Generator().manual_seed(100 + k))
            for k in range(K)]


def _operands(samples):
    bufs, layers, base = [], [], 0
    for s in samples:
        b = s.pack()
        layers.append(s.layer_offsets(base))
        bufs.append(b)
        base += b.numel()
    return torch.cat(bufs).to(DEV), layers


def _per_layer(s, xd):
    """The sample through one mobocmf_rff_eval launch per layer."""
    from mobocmf_amd import functional as F
    f = None
    for Lr in s.layers:
        t = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in Lr.items()}
        f = F.rff_eval(Lr["kind"], xd, f, t["W1"], t["b1"], t.get("Wf"), t.get("W2"), t.get("b2"), t["theta"],
                       *Lr["scales"])
    return f


def _oracle(s, X):
    f = None
    for Lr in s.layers:
        n = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in Lr.items()}
        if Lr["kind"] == 0:
            Phi = RO.layer0_features(X, n["W1"], n["b1"][:, None], n["alpha"])
        else:
            Phi = RO.layer1_features(X, f, n["W1"], n["Wf"], n["W2"], n["b1"][:, None], n["b2"][:, None], n["a1"], n["af"],
                                     n["a2"], n["nu"])
        f = n["theta"] @ Phi
    return f


@pytest.mark.parametrize("d,L,F", [(2, 2, 150), (8, 2, 500), (3, 3, 64), (32, 2, 97)])
@pytest.mark.parametrize("K", [1, 3, 9])
def test_chains_match_per_layer_kernel_and_oracle(d, L, F, K):
    from mobocmf_amd import functional as Fn
    samples = _chains(d, L, F, K, seed=d)
    n = 1000 + 37                                            # ragged: the last workgroup is partly empty
    X = np.random.default_rng(K).random((n, d))
    xd = torch.from_numpy(X).to(DEV)
    params, layers = _operands(samples)
    out = Fn.rff_eval_chains(xd, params, layers)
    assert out.shape == (K, n) and out.dtype == torch.float64
    again = Fn.rff_eval_chains(xd, params, layers)
    assert torch.equal(out, again)                           # deterministic: bitwise across launches
    got = out.cpu().numpy()
    for k, s in enumerate(samples):
        ref_layer = _per_layer(s, xd).cpu().numpy()
        ref_oracle = _oracle(s, X)
        scale = max(1.0, np.abs(ref_oracle).max())
        assert np.abs(got[k] - ref_layer).max() <= 1e-11 * scale, (k, np.abs(got[k] - ref_layer).max())
        assert np.abs(got[k] - ref_oracle).max() <= 1e-11 * scale, (k, np.abs(got[k] - ref_oracle).max())
    assert np.abs(samples[0](X) - got[0]).max() <= 1e-11 * max(1.0, np.abs(got[0]).max())     # the callable's grid path


def test_feasibility_matches_numpy():
    from mobocmf_amd import functional as Fn
    g = np.random.default_rng(0)
    for K_con, n in [(1, 5000), (3, 1037), (4, 1)]:
        vals = g.standard_normal((K_con, n))
        vals[:, ::7] = 0.25                                  # slack exactly 0 counts as feasible
        thr = np.full(K_con, 0.25) if K_con > 1 else np.array([0.25])
        ok, viol = Fn.rff_feasibility(torch.from_numpy(vals).to(DEV), torch.from_numpy(thr).to(DEV))
        slack = [vals[c] - thr[c] for c in range(K_con)]
        ok_ref = np.ones(n, dtype=bool)
        viol_ref = np.zeros(n)
        for s in slack:
            ok_ref &= s >= 0
            viol_ref += np.minimum(s, 0.0)
        assert np.array_equal(ok.cpu().numpy(), ok_ref)
        assert np.array_equal(viol.cpu().numpy(), viol_ref)


def test_bad_arguments_raise():
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as Fn
    s = _chains(2, 2, 16, 1)[0]
    params, layers = _operands([s])
    xd = torch.rand(300, 2, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.MobocmfError):
        Fn.rff_eval_chains(xd, params, [layers[0] * 2])                       # 4 layers
    with pytest.raises(_lib.MobocmfError):
        Fn.rff_eval_chains(xd, params, [layers[0][::-1]])                     # kind 1 first
    with pytest.raises(_lib.MobocmfError):
        Fn.rff_eval_chains(xd, params[:-1], layers)                           # operands outside params
    with pytest.raises(_lib.MobocmfError):
        Fn.rff_eval_chains(torch.rand(300, 3, dtype=torch.float64, device=DEV), params[:10], layers)
    with pytest.raises(_lib.MobocmfError):
        Fn.rff_eval_chains(xd.cpu(), params, layers)
    with pytest.raises(_lib.MobocmfError):
        Fn.rff_eval_chains(torch.rand(3, 33, dtype=torch.float64, device=DEV), params, layers)
    with pytest.raises(_lib.MobocmfError):
        Fn.rff_feasibility(torch.rand(2, 10, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV))
    lib = _lib.require_device()
    out = torch.empty(2, 300, dtype=torch.float64, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.mobocmf_rff_eval_chains(0, 2, 300, p(xd), p(params), params.numel(), p(params), p(out), st) == _lib.BAD_ARG
    assert lib.mobocmf_rff_eval_chains(1, 2, 300, None, p(params), params.numel(), p(params), p(out), st) == _lib.BAD_ARG
    assert lib.mobocmf_rff_eval_chains(1, 33, 300, p(xd), p(params), params.numel(), p(params), p(out), st) == _lib.BAD_ARG
    assert lib.mobocmf_rff_eval_chains(1, 2, 300, p(xd), p(params), params.numel(), None, p(out), st) == _lib.BAD_ARG
    ok = torch.empty(300, dtype=torch.int32, device=DEV)
    assert lib.mobocmf_rff_feasibility(1, 300, p(out), 299, p(out), p(ok), p(out), st) == _lib.BAD_ARG
    assert lib.mobocmf_rff_feasibility(0, 300, p(out), 300, p(out), p(ok), p(out), st) == _lib.BAD_ARG
    assert lib.mobocmf_rff_feasibility(1, 300, p(out), 300, None, p(ok), p(out), st) == _lib.BAD_ARG


@pytest.mark.parametrize("n_obj,n_con,allow_negative", [(2, 1, False), (3, 2, False), (2, 0, False), (2, 1, True)])
def test_moop_batched_path_matches_per_callable_path(n_obj, n_con, allow_negative):
    """The same chain samples through MOOP twice: as RFFChainSamples on the GPU (one launch for all of them on the grid, the
    feasibility pass on the device) and as the per-layer callables of sample_function_from_each_layer drawn from the same
    generators (one mobocmf_rff_eval launch per layer and sample)."""
    from mobocmf_amd.layers import rff
    from mobocmf_amd.util.moop import MOOP
    d = 2
    models = [synthetic.model_from_problem(synthetic.make_problem(d=d, L=2, M=10, N=30, S=1, seed=j), device=DEV)
              for j in range(n_obj + n_con)]
    gen = lambda j: torch.Generator().manual_seed(40 + j)
    chains = [rff.sample_chain_from_posterior(m, nFeatures=120, generator=gen(j)) for j, m in enumerate(models)]
    calls = [m.sample_function_from_each_layer(nFeatures=120, generator=gen(j))[-1] for j, m in enumerate(models)]
    inputs = np.random.default_rng(5).random((12, d))
    thr = np.array([1e6] * n_con) if allow_negative else np.array([-0.2] * n_con)
    out = []
    for samples in (chains, calls):
        moop = MOOP(samples[:n_obj], samples[n_obj:], input_dim=d, grid_size=2100, pareto_set_size=10,
                    feasible_values=thr, rng=np.random.default_rng(9))
        assert (moop._batched_device() is not None) == (samples is chains)
        res = moop.compute_pareto_solution_from_samples(inputs, allow_negative_constraints=allow_negative)
        assert res is not None
        out.append((res[0].numpy(), res[1].numpy()))
    (s0, f0), (s1, f1) = out
    assert np.array_equal(s0, s1)                                         # the same grid rows: the same Pareto indices
    assert np.abs(f0 - f1).max() <= 1e-12 * max(1.0, np.abs(f1).max())
