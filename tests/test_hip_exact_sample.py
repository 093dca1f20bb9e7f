"""The exact-GP function sample on the GPU (mobocmf_exact_sample_*, mobocmf_amd/util/exact_sample.py, util/mes_front.py, the MES
loop of examples/) against the longdouble restatement tests/exact_sample_reference.py and against the host engine.

The gram launch is checked componentwise under the bound DERIVED in tests/exact_sample_reference.py (``gram_bounds``): a cosine
is off by u ((d + 1) A + 4) -- d fused multiply-adds on an argument of magnitude sum A, |cos'| <= 1, the device cosine -- a sum
over F features in the matrix instruction adds (F + 1) u sum |c c|, the epilogue 8 u on the magnitudes.

The weights launch and the whole device draw are held to the HOST engine's own error on the same inputs:
err_device <= 8 err_host + 64 u, err the maximum error of theta against the restatement relative to max |theta| (8: another
summation order and the device cosine; 64 u: a host error of zero), and the same rule for the interpolation-identity residual
relative to max |y|, the samples evaluated through functional.rff_eval_chains.  Measured figures: DESIGN.md 5.6.8."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import exact_sample_reference as S
from tests import mes_reference as M
from tests.test_exact_sample_cpu import _restate, _split

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = S.U
CHUNK = 16      # MOBOCMF_EXACT_SAMPLE_CHUNK

# (n, d, n_levels, F, kernel, a level no row has)
GRAM_CASES = ((1, 1, 1, 1, "min", None), (15, 2, 2, 3, "lin", None), (16, 9, 3, 4, "min", None), (17, 32, 8, 5, "lin", None),
              (130, 2, 3, CHUNK + 1, "min", 1), (130, 9, 8, 500, "lin", None), (512, 1, 2, CHUNK + 1, "lin", None))


def _on_dev(c):
    ops, rnd = _split(c)
    return {k: v.to(DEV) for k, v in ops.items()}, {k: v.to(DEV) for k, v in rnd.items()}


def _launch(cases, levels=None):
    from mobocmf_amd.util.exact_sample import ExactSampleLaunch
    pairs = [_on_dev(c) for c in cases]
    levels = [list(range(len(c["sig"]))) for c in cases] if levels is None else levels
    return ExactSampleLaunch([p[0] for p in pairs], [p[1] for p in pairs], levels)


def _check_gram(c, G, r, tag):
    n, npad = c["x"].shape[0], (c["x"].shape[0] + 127) // 128 * 128
    R = S.restate(c["x"], c["lev"], c["y"], c["sig"], c["ntab"], c["scal"], c["W_sig"], c["b_sig"], c["W_noi"], c["b_noi"],
                  c["theta0"], c["e"], solve=False)
    bG, br = S.gram_bounds(R)
    G, r = G.cpu().numpy(), r.cpu().numpy()
    assert G.shape == (npad, npad)
    eG, er = np.abs(S.ld(G[:n, :n]) - R["G"]), np.abs(S.ld(r) - R["r"])
    print("gram %s: worst err / bound  G %.3f  r %.3f" % (tag, float((eG / bG).max()), float((er / br).max())))
    assert np.all(eG <= bG) and np.all(er <= br)
    assert np.array_equal(G[:n, :n], G[:n, :n].T)                                   # the mirror is a copy
    assert not G[n:, :n].any() and not G[:n, n:].any()                              # the padding: zeros ...
    assert np.array_equal(G[n:, n:], np.eye(npad - n))                              # ... and identity on the padded diagonal


# --------------------------------------------------------------------------------------------------------- 1. the gram launch
@pytest.mark.skipif(not S.HAVE_LONGDOUBLE, reason="numpy longdouble is float64 on this platform")
@pytest.mark.parametrize("shape", GRAM_CASES, ids=str)
def test_gram_launch_componentwise(shape):
    n, d, nl, F, kern, empty = shape
    c = S.case(n, d, nl, F, kern, empty_level=empty)
    if empty is not None:
        assert not (c["lev"] == empty).any()
    L = _launch([c])
    L.gram()
    _check_gram(c, L.G(0), L.r(0), str(shape))


@pytest.mark.skipif(not S.HAVE_LONGDOUBLE, reason="numpy longdouble is float64 on this platform")
def test_gram_launch_of_several_problems_of_different_n():
    a, b = S.case(17, 2, 2, 21, "min"), S.case(130, 3, 3, 21, "lin")
    cases = []
    for c, seed in ((a, 1), (a, 2), (b, 3), (b, 4)):      # two samples of each model: other theta0 and e
        rng = np.random.default_rng(seed)
        cases.append(dict(c, theta0=rng.standard_normal(c["theta0"].shape), e=0.1 * rng.standard_normal(c["e"].shape)))
    L = _launch(cases)
    L.gram()
    for i, c in enumerate(cases):
        _check_gram(c, L.G(i), L.r(i), "problem %d of 4" % i)
    first = [(L.G(i).clone(), L.r(i).clone()) for i in range(4)]
    L.gram()                                                                        # two runs are bitwise equal
    assert all(torch.equal(L.G(i), g) and torch.equal(L.r(i), r) for i, (g, r) in enumerate(first))


def test_a_level_outside_the_tables_is_nan_and_the_limits_are_refused():
    from mobocmf_amd import _lib
    c = S.case(20, 2, 2, 8, "min")
    c["lev"] = c["lev"].copy()
    c["lev"][3] = 7
    L = _launch([c], levels=[[0]])
    L.gram()
    G = L.G(0).cpu()
    assert bool(torch.isnan(G[3, :20]).all()) and bool(torch.isnan(G[:20, 3]).all()) and bool(torch.isnan(L.r(0)[3]))
    assert bool(torch.isfinite(G[4, [0, 1, 2, 4, 5]]).all())
    L.host[0].F = 0
    with pytest.raises(_lib.MobocmfError):
        L.gram()
    L.host[0].F, L.host[0].n = 8, 513
    with pytest.raises(_lib.MobocmfError):
        L.gram()


# ------------------------------------------------------------------------------------- 2. the weights launch, the whole draw
def _rel_err(got, ref):
    return float(np.abs(S.ld(got) - ref).max() / np.abs(ref).max())


def _residual(draw, c, evaluate):
    x, lev, y = c["x"], c["lev"], c["y"]
    w, e, noise = draw.w.cpu().numpy(), draw.e.cpu().numpy(), float(draw.noise)
    res = np.zeros(x.shape[0])
    for f, smp in draw.samples.items():
        rows = lev == f
        if rows.any():
            res[rows] = evaluate(smp, x[rows]) + e[rows] + noise * w[rows] - y[rows]
    return float(np.abs(res).max() / np.abs(y).max())


@pytest.mark.skipif(not S.HAVE_LONGDOUBLE, reason="numpy longdouble is float64 on this platform")
@pytest.mark.parametrize("shape", [(40, 2, 3, 64, "min"), (17, 32, 8, 5, "lin"), (130, 9, 4, 100, "lin"), (300, 2, 2, CHUNK + 1, "min")], ids=str)
def test_device_draw_is_as_accurate_as_the_host_engine(shape):
    from mobocmf_amd.util.exact_sample import device_draw, host_draw
    n, d, nl, F, kern = shape
    c = S.case(n, d, nl, F, kern)
    R = _restate(c, levels=range(nl))
    ops, rnd = _split(c)
    host = host_draw(ops, rnd, range(nl))
    dops, drnd = _on_dev(c)
    dev = device_draw([dops], [drnd], [list(range(nl))])[0]
    assert dev.engine == "device" and dev.info == 0
    eh, ed = _rel_err(host.theta.numpy(), R["theta"]), _rel_err(dev.theta.cpu().numpy(), R["theta"])
    wh, wd = _rel_err(host.w.numpy(), R["w"]), _rel_err(dev.w.cpu().numpy(), R["w"])
    print("draw %s: theta err host %.3e device %.3e | w err host %.3e device %.3e" % (shape, eh, ed, wh, wd))
    assert ed <= 8 * eh + 64 * U
    assert wd <= 8 * wh + 64 * U
    for f in range(nl):      # the folded operands, written straight into the packed sample
        fh = _rel_err(host.samples[f].layers[0]["theta"].numpy(), R["folded"][f])
        fd = _rel_err(dev.samples[f].layers[0]["theta"].numpy(), R["folded"][f])
        assert fd <= 8 * fh + 64 * U, (f, fh, fd)
        assert torch.equal(dev.samples[f].layers[0]["W1"], host.samples[f].layers[0]["W1"])
        assert torch.equal(dev.samples[f].layers[0]["b1"], host.samples[f].layers[0]["b1"])
        assert dev.samples[f].layers[0]["alpha"] == float(F) and dev.samples[f].layers[0]["scales"] == (1.0, 0.0, 0.0)
    rh = _residual(host, c, lambda s, x: s(x))
    rd = _residual(dev, c, lambda s, x: s._device(torch.as_tensor(x, device=DEV).contiguous()).cpu().numpy())
    print("draw %s: interpolation residual host %.3e device %.3e" % (shape, rh, rd))
    assert rd <= 8 * rh + 64 * U


# ---------------------------------------------------------------------------------------- 3. one generator, both engines
@pytest.mark.skipif(not S.HAVE_LONGDOUBLE, reason="numpy longdouble is float64 on this platform")
@pytest.mark.parametrize("cls", ["MFGP", "MFGP_lin"])
def test_same_generator_gives_the_same_function_on_both_engines(cls):
    from mobocmf_amd.models import mfgp
    from mobocmf_amd.util.exact_sample import draw_operands, model_operands
    model = M.mes_models(24, 2, 3, seed=1, device=DEV, classes={"m": getattr(mfgp, cls)})["m"]
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)
    dev = model.sample_chain_from_posterior(2, nFeatures=40, generator=gen(), engine="device")
    assert model.last_draw.engine == "device"
    host = model.sample_chain_from_posterior(2, nFeatures=40, generator=gen(), engine="host")
    assert model.last_draw.engine == "host"
    assert dev.F == 80 and len(dev.layers) == 1 and dev.device.type == "cuda"
    assert torch.equal(dev.layers[0]["W1"], host.layers[0]["W1"]) and torch.equal(dev.layers[0]["b1"], host.layers[0]["b1"])
    ops = model_operands(model)
    rnd = draw_operands(model, 40, gen(), ops)
    num = lambda t: t.detach().cpu().numpy()
    R = S.restate(num(ops["x"]), num(ops["lev"]), num(ops["y"]), num(ops["sig"]), num(ops["ntab"]), num(ops["scal"]),
                  num(rnd["W_sig"]), num(rnd["b_sig"]), num(rnd["W_noi"]), num(rnd["b_noi"]), num(rnd["theta0"]), num(rnd["e"]),
                  levels=[2])
    eh, ed = _rel_err(num(host.layers[0]["theta"]), R["folded"][2]), _rel_err(num(dev.layers[0]["theta"]), R["folded"][2])
    print("same generator (%s): folded theta err host %.3e device %.3e" % (cls, eh, ed))
    assert ed <= 8 * eh + 64 * U
    with pytest.raises(RuntimeError, match="training rows"):
        big = M.mes_models(513, 2, 2, device=DEV, classes={"m": mfgp.MFGP})["m"]
        big.sample_chain_from_posterior(1, nFeatures=4, engine="device")


# ------------------------------------------------------------------------------------------------ 4. MOOP's batched path
def test_moop_takes_the_samples_on_its_batched_path():
    from mobocmf_amd.util.exact_sample import draw_chain_samples
    from mobocmf_amd.util.moop import MOOP
    models = M.mes_models(24, 2, 2, seed=3, device=DEV)
    res = draw_chain_samples(models, 1, nFeatures=64, generator=torch.Generator(device=DEV).manual_seed(0))
    assert res.engines == {"o0": "device", "o1": "device", "c0": "device"}
    objs, cons = [res.samples["o0"].negated(), res.samples["o1"].negated()], [res.samples["c0"]]
    inputs = models["o0"].x_train[:, :2].cpu().numpy()
    for kw in (dict(refine="device"), dict(search="evolve", evolve_population=16, evolve_generations=4, evolve_seed=1)):
        moop = MOOP(objs, cons, input_dim=2, grid_size=200, feasible_values=np.array([-0.5]), rng=np.random.default_rng(0), **kw)
        assert moop._batched_device() == res.samples["o0"].device and moop._batched_device().type == "cuda"
        out = moop.compute_pareto_solution_from_samples(inputs)
        assert out is not None
        pset, front = out[0].numpy(), out[1].numpy()
        assert front.shape[0] >= 1 and np.isfinite(front).all()
        assert np.allclose(objs[0](pset), front[:, 0], rtol=0, atol=1e-9)
        assert np.all(cons[0](pset) >= -0.5 - 1e-6)


# ------------------------------------------------------------------------------------------------ 5. sample_pareto_front
class _CountReads:
    """Counts the calls that copy a GPU tensor to the host (or read a value off it) while active."""
    NAMES = ("cpu", "item", "tolist", "numpy", "__float__", "__int__", "__bool__", "__index__")

    def __init__(self):
        self.count, self._saved = 0, {}

    def __enter__(self):
        for name in self.NAMES:
            orig = getattr(torch.Tensor, name)
            self._saved[name] = orig

            def wrapped(t, *a, _orig=orig, **k):
                if t.is_cuda:
                    self.count += 1
                return _orig(t, *a, **k)

            setattr(torch.Tensor, name, wrapped)
        orig_to = torch.Tensor.to
        self._saved["to"] = orig_to

        def to(t, *a, **k):
            out = orig_to(t, *a, **k)
            if t.is_cuda and not out.is_cuda:
                self.count += 1
            return out

        torch.Tensor.to = to
        return self

    def __exit__(self, *exc):
        for name, orig in self._saved.items():
            setattr(torch.Tensor, name, orig)


def test_sample_pareto_front_on_the_device(monkeypatch):
    from mobocmf_amd.util import mes_front
    models = M.mes_models(24, 2, 2, seed=2, device=DEV)
    objs = {k: m for k, m in models.items() if k.startswith("o")}
    cons = {k: m for k, m in models.items() if k.startswith("c")}
    inputs = models["o0"].x_train[:, :2].cpu().numpy()
    reads, real = [], mes_front.draw_chain_samples

    def counted(*a, **k):
        with _CountReads() as c:
            out = real(*a, **k)
        reads.append(c.count)
        return out

    monkeypatch.setattr(mes_front, "draw_chain_samples", counted)
    out = mes_front.sample_pareto_front(objs, cons, {"c0": -0.5}, inputs, 2, nFeatures=64,
                                        generator=torch.Generator(device=DEV).manual_seed(0), rng=np.random.default_rng(0),
                                        engine="device", grid_size=200, refine="device")
    assert out.engines == {"o0": "device", "o1": "device", "c0": "device"}
    assert all(np.isfinite(v) for v in out.best_objective_values.values()) and set(out.best_objective_values) == {"o0", "o1"}
    front = out.pareto_front.numpy()
    assert [out.best_objective_values[k] for k in objs] == [-front[:, j].min() for j in range(2)]
    assert len(reads) == 1 + out.tries and reads == [1] * len(reads), reads      # ONE host read per draw call


# ------------------------------------------------------------------------------------------------ 6. the loop
def test_mes_loop_writes_scored_rows_and_searches_on_the_device(tmp_path):
    examples = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    sys.path.insert(0, examples)
    try:
        from bo_loop_hv_toy2d import loop_hv
    finally:
        sys.path.remove(examples)
    record = []
    rows = loop_hv(iters=2, acq="mes", epochs=20, out_dir=str(tmp_path), verbose=False, record=record)
    text = open(os.path.join(str(tmp_path), "hypervolumes.txt")).read().split("\n")
    lines = [ln.split() for ln in text if ln.strip()]
    assert len(rows) == 2 and len(lines) == 2 and all(len(ln) == 6 for ln in lines)
    assert all(np.isfinite(float(v)) for ln in lines for v in ln)
    assert [r["rows"] for r in record] == [20, 21]                                   # the data grow by one row per iteration
    assert all(r["search_engine"] == {0: "device", 1: "device"} for r in record)
    assert all(set(r["sample_engines"].values()) == {"device"} for r in record)
