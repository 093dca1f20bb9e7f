"""The refinement mode of MOOP and the fitter, and the argument checks of mobocmf_rff_chains_value_grad / mobocmf_rff_refine
(every check fails before a launch could happen): no GPU needed."""
import ctypes
import math

import numpy as np
import pytest
import torch


def _random_chain(d, F, seed, L=2):
    """A hand-built chain sample on the host (no model needed): unit hyper-parameters, random draws."""
    from mobocmf_amd.layers.rff import RFFChainSample
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    ru = lambda *s: 2.0 * math.pi * torch.rand(*s, dtype=torch.float64, generator=g)
    s = math.sqrt(2.0 / F)
    layers = [{"kind": 0, "F": F, "alpha": 1.0, "scales": (s, 0.0, 0.0), "W1": 2.0 * rn(F, d), "b1": ru(F), "theta": rn(F)}]
    for _ in range(L - 1):
        layers.append({"kind": 1, "F": F, "a1": 1.0, "af": 1.0, "a2": 1.0, "nu": 1.0, "scales": (s, s, s),
                       "W1": 0.5 * rn(F, d), "b1": ru(F), "theta": rn(3 * F), "Wf": rn(F), "W2": 2.0 * rn(F, d), "b2": ru(F)})
    return RFFChainSample(layers, d)


def test_moop_refine_keyword():
    from mobocmf_amd.util.moop import MOOP
    f = lambda x, gradient=False: np.zeros(len(x))
    with pytest.raises(ValueError):
        MOOP([f], [], input_dim=2, refine="nope")
    with pytest.raises(ValueError):
        MOOP([f], [], input_dim=2, refine_starts=0)
    assert MOOP([f], [], input_dim=2).refine == "slsqp" and MOOP([f], [], input_dim=2).refine_starts == 16
    # the device mode has no host fallback: host callables, and chain samples that live on no GPU, are refused
    for samples in ([f, f], [_random_chain(2, 8, 0), _random_chain(2, 8, 1)]):
        moop = MOOP(samples, [], input_dim=2, grid_size=10, refine="device", rng=np.random.default_rng(0))
        with pytest.raises(ValueError, match="RFFChainSample"):
            moop.compute_pareto_solution_from_samples(np.zeros((1, 2)))


def test_fitter_pareto_refine_keyword():
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    fit = BlackBoxMFDGPFitter(2, 10, device="cpu", pareto_refine="device", inducing_selection="first")
    assert fit.pareto_refine == "device" and "pareto_refine" not in fit.model_kwargs
    assert fit.model_kwargs == {"inducing_selection": "first"}
    assert BlackBoxMFDGPFitter(2, 10, device="cpu").pareto_refine == "slsqp"
    with pytest.raises(ValueError):
        BlackBoxMFDGPFitter(2, 10, device="cpu", pareto_refine="nope")


def test_default_moop_is_the_slsqp_mode():
    from mobocmf_amd.util.moop import MOOP
    d = 2
    chains = [_random_chain(d, 24, 10 + k) for k in range(3)]
    inputs = np.random.default_rng(1).random((5, d))
    thr = np.array([float(np.quantile(chains[2](np.random.default_rng(2).random((400, d))), 0.4))])
    res = []
    for kw in ({}, {"refine": "slsqp"}, {"refine": "slsqp", "refine_starts": 3}):
        moop = MOOP(chains[:2], chains[2:], input_dim=d, grid_size=150, pareto_set_size=8, feasible_values=thr,
                    rng=np.random.default_rng(4), **kw)
        out = moop.compute_pareto_solution_from_samples(inputs)
        assert out is not None
        res.append((out[0].numpy(), out[1].numpy()))
    for s, f in res[1:]:
        assert np.array_equal(s, res[0][0]) and np.array_equal(f, res[0][1])


def test_entry_points_refuse_bad_arguments():
    from mobocmf_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                # never dereferenced: every call below is refused before a launch
    vg = lambda K=1, d=2, n=5, x=p, par=p, plen=64, desc=p, vals=p, grads=p: \
        lib.mobocmf_rff_chains_value_grad(K, d, n, x, par, plen, desc, vals, grads, None)
    assert vg(K=0) == _lib.BAD_ARG and vg(K=65536) == _lib.BAD_ARG
    assert vg(d=0) == _lib.BAD_ARG and vg(d=_lib.MAX_D + 1) == _lib.BAD_ARG
    assert vg(n=0) == _lib.BAD_ARG and vg(plen=0) == _lib.BAD_ARG
    for name in ("x", "par", "desc", "vals", "grads"):
        assert vg(**{name: None}) == _lib.BAD_ARG, name

    opt = _lib.RffRefineOptions()
    assert lib.mobocmf_rff_refine_options_init(None) == _lib.BAD_ARG
    assert lib.mobocmf_rff_refine_options_init(ctypes.byref(opt)) == _lib.OK
    assert opt.struct_size == ctypes.sizeof(_lib.RffRefineOptions)
    assert (opt.outer, opt.inner, opt.backtracks, opt.restore, opt.recentre) == (8, 30, 6, 4, 1)
    assert (opt.step0, opt.step_shrink, opt.step_grow, opt.rho0, opt.rho_growth, opt.armijo) == (0.05, 0.25, 2.0, 10.0, 4.0, 1e-4)

    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    names = ("x0", "par", "desc", "xs", "fs", "slack_min", "x_best", "f_best", "start_best", "status")

    def refine(P=1, R=2, d=2, K=3, obj=i32(0), off=i32(0), cnt=i32(2), n_con=2, con=p, thr=p, plen=64, o=None, **ptr):
        a = {k: ptr.get(k, p) for k in names}
        return lib.mobocmf_rff_refine(P, R, d, K, obj, off, cnt, n_con, con, thr, a["x0"], a["par"], plen, a["desc"],
                                      None if o is None else ctypes.byref(o), a["xs"], a["fs"], a["slack_min"], a["x_best"],
                                      a["f_best"], a["start_best"], a["status"], None)

    assert refine(P=0) == _lib.BAD_ARG and refine(P=_lib.REFINE_MAX_PROBLEMS + 1) == _lib.BAD_ARG
    assert refine(R=0) == _lib.BAD_ARG and refine(d=0) == _lib.BAD_ARG and refine(d=_lib.MAX_D + 1) == _lib.BAD_ARG
    assert refine(K=0) == _lib.BAD_ARG and refine(plen=0) == _lib.BAD_ARG
    assert refine(cnt=i32(-1)) == _lib.BAD_ARG and refine(cnt=i32(_lib.REFINE_MAX_CON + 1), n_con=64) == _lib.BAD_ARG
    assert refine(cnt=i32(3)) == _lib.BAD_ARG and refine(off=i32(1)) == _lib.BAD_ARG and refine(off=i32(-1)) == _lib.BAD_ARG
    assert refine(obj=i32(3)) == _lib.BAD_ARG and refine(obj=i32(-1)) == _lib.BAD_ARG
    assert refine(obj=None) == _lib.BAD_ARG and refine(off=None) == _lib.BAD_ARG and refine(cnt=None) == _lib.BAD_ARG
    assert refine(con=None) == _lib.BAD_ARG and refine(thr=None) == _lib.BAD_ARG
    for name in names:
        assert refine(**{name: None}) == _lib.BAD_ARG, name
    for field, bad in (("struct_size", 8), ("outer", 0), ("inner", 0), ("backtracks", -1), ("restore", -1), ("recentre", 2), ("step0", 0.0),
                       ("step_shrink", 1.0), ("step_grow", 0.5), ("rho0", 0.0), ("rho_growth", 0.5), ("armijo", 1.0),
                       ("restore_margin", -1.0), ("step0", float("nan"))):
        ob = _lib.RffRefineOptions.from_buffer_copy(opt)
        setattr(ob, field, bad)
        assert refine(o=ob) == _lib.BAD_ARG, field


def test_wrappers_refuse_cpu_tensors_and_mismatches():
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as Fn
    try:
        _lib.require_device()
    except _lib.MobocmfError:
        pass                                             # without a GPU the wrappers raise the same error class first
    s = _random_chain(2, 8, 0)
    params, layers = s.pack(), [s.layer_offsets(0)]
    with pytest.raises(_lib.MobocmfError):
        Fn.rff_chains_value_grad(torch.rand(4, 2, dtype=torch.float64), params, layers)
    with pytest.raises(_lib.MobocmfError):
        Fn.rff_refine(torch.rand(1, 4, 2, dtype=torch.float64), params, layers, obj=[0])
