#!/usr/bin/env python3
"""The stage of a max-value entropy search iteration between the fit and the acquisition search -- one posterior function sample
per model, then the sampled problem's Pareto front -- three ways, for three models (an MFGP, an MFGP_lin, an MFGP; two
fidelities) on n training rows each, at d = 2 / 8 and n = 24 / 64 / 256, ``--features`` random features per kernel:

  reference-style   ``MFGP.sample_from_posterior`` (numpy: an (F nf) x (F nf) factorisation, an explicit inverse, a second
                    factorisation; returns a host callable) -- the only draw the package had, and ``MOOP`` over such callables;
                    ``MFGP_lin`` has no such method, so the ``MFGP_lin`` model is drawn as an ``MFGP`` on the same data here
  host engine       ``draw_chain_samples(engine="host")``: Matheron's rule in float64 torch on the CPU
  device engine     ``draw_chain_samples(engine="device")``: csrc/exact_sample.hip, one read per call

and ``MOOP`` over the host callables against ``MOOP`` over the chain samples with ``refine="slsqp"`` and ``refine="device"``; last
the fit / sample / search split of one whole MES iteration on the toy problem (examples/bo_iteration_mes_toy2d.py).

Every figure is the median of ``--repeats`` runs after one warm-up run, a host clock around a final synchronise.  One JSON line
per (n, d), one for the iteration.

usage: python tools/mes_front_bench.py [--features 500] [--repeats 3] [--sizes 24,64,256] [--dims 2,8]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from mobocmf_amd.models.mfgp import MFGP, MFGP_lin  # noqa: E402
from mobocmf_amd.util.exact_sample import draw_chain_samples  # noqa: E402
from mobocmf_amd.util.moop import MOOP  # noqa: E402

DEV = "cuda"
N_FID = 2


def problem(n, d, seed=0, classes=(MFGP, MFGP_lin, MFGP)):
    g = torch.Generator().manual_seed(seed)
    models = {}
    for k, (name, cls) in enumerate(zip(("o0", "o1", "c0"), classes)):
        x = torch.rand(n, d, generator=g, dtype=torch.float64)
        fid = (torch.arange(n) % N_FID).double()[:, None]
        y = torch.sin(3.0 * x.sum(1) + k) + 0.3 * fid[:, 0] + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
        models[name] = cls(torch.cat([x, fid], 1), y, N_FID).to(DEV)
    return models


def median_s(fn, repeats):
    fn()      # warm-up
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return round(statistics.median(times), 4), out


def moop_seconds(objs, cons, inputs, d, repeats, **kw):
    def once():
        m = MOOP(objs, cons, input_dim=d, grid_size=1000, feasible_values=np.array([-10.0]), rng=np.random.default_rng(0), **kw)
        return m.compute_pareto_solution_from_samples(inputs)
    return median_s(once, repeats)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="24,64,256")
    ap.add_argument("--dims", default="2,8")
    a = ap.parse_args()
    F, top = a.features, N_FID - 1
    for n in [int(s) for s in a.sizes.split(",")]:
        for d in [int(s) for s in a.dims.split(",")]:
            models = problem(n, d)
            plain = problem(n, d, classes=(MFGP, MFGP, MFGP))      # (sample_from_posterior exists on MFGP only)
            inputs = models["o0"].x_train[:, :d].cpu().numpy()
            res = {"n": n, "d": d, "features": F, "repeats": a.repeats}
            rng = np.random.default_rng(0)
            res["draw_reference_style_s"], ref = median_s(
                lambda: {k: m.sample_from_posterior(top, nFeatures=F, rng=rng) for k, m in plain.items()}, a.repeats)
            gen = torch.Generator(device=DEV).manual_seed(0)
            res["draw_host_engine_s"], _ = median_s(
                lambda: draw_chain_samples(models, top, nFeatures=F, generator=gen, engine="host"), a.repeats)
            res["draw_device_engine_s"], drawn = median_s(
                lambda: draw_chain_samples(models, top, nFeatures=F, generator=gen, engine="device"), a.repeats)
            assert set(drawn.engines.values()) == {"device"}, drawn.engines
            neg = lambda f: (lambda x, gradient=False: -f(x, gradient=gradient))      # noqa: E731
            res["moop_host_callables_s"] = moop_seconds([neg(ref["o0"]), neg(ref["o1"])], [ref["c0"]], inputs, d, a.repeats)
            objs, cons = [drawn.samples["o0"].negated(), drawn.samples["o1"].negated()], [drawn.samples["c0"]]
            res["moop_chain_samples_slsqp_s"] = moop_seconds(objs, cons, inputs, d, a.repeats, refine="slsqp")
            res["moop_chain_samples_device_s"] = moop_seconds(objs, cons, inputs, d, a.repeats, refine="device")
            res["stage_before_s"] = round(res["draw_reference_style_s"] + res["moop_host_callables_s"], 4)
            res["stage_device_s"] = round(res["draw_device_engine_s"] + res["moop_chain_samples_device_s"], 4)
            print(json.dumps(res), flush=True)
    from bo_iteration_mes_toy2d import run
    run(verbose=False, nFeatures=F)      # warm-up: library first calls, graph captures
    splits = [run(verbose=False, nFeatures=F, seed=s)[5] for s in range(a.repeats)]
    med = [round(statistics.median(col), 4) for col in zip(*splits)]
    print(json.dumps({"mes_iteration_toy2d": dict(fit_s=med[0], sample_s=med[1], search_s=med[2]), "features": F}), flush=True)


if __name__ == "__main__":
    main()
