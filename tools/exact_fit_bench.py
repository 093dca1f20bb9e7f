#!/usr/bin/env python3
"""Fitting the exact-GP baselines, host engine against device engine: three models (an MFGP, an MFGP_lin, an MFGP; two
fidelities) on n training rows each, ``--iters`` Adam iterations at lr 0.05, at n = 24 / 64 / 256 / 512 and d = 2 / 8.  Host:
``fit(engine="host")`` model after model (the loop the package had before the device engine existed, unchanged by it); device:
``fit_exact_gps`` over the three at once (one captured step replayed per iteration, one read at the end).

Both engines are warmed up once on copies of the models (library first calls, graph capture: reported as the first call's
time), then whole fits of fresh copies are timed with a host clock around a final synchronise, the engines alternating in the
same process; the median of ``--repeats`` fits is reported with the spread, the microseconds per replayed step (the captured
graph replayed back to back), and how far the two engines' fitted parameters and final likelihoods are apart.  The host engine
is the baseline.  One JSON line per (n, d).

usage: python tools/exact_fit_bench.py [--iters 200] [--repeats 3] [--sizes 24,64,256,512] [--dims 2,8]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mobocmf_amd.models.mfgp import MFGP, MFGP_lin  # noqa: E402
from mobocmf_amd.util.exact_fit import ExactGPFitStep, fit_exact_gps  # noqa: E402

DEV = "cuda"
N_FID = 2
LR = 0.05


def problem(n, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    models = {}
    for k, (name, cls) in enumerate((("o0", MFGP), ("o1", MFGP_lin), ("c0", MFGP))):
        x = torch.rand(n, d, generator=g, dtype=torch.float64)
        fid = (torch.arange(n) % N_FID).double()[:, None]
        y = torch.sin(3.0 * x.sum(1) + k) + 0.3 * fid[:, 0] + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
        models[name] = cls(torch.cat([x, fid], 1), y, N_FID).to(DEV)
    return models


def timed(base, engine, iters):
    models = {k: copy.deepcopy(m) for k, m in base.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if engine == "host":
        for m in models.values():
            m.fit(num_iters=iters, lr=LR, engine="host")
    else:
        res = fit_exact_gps(models, iters, LR)
        assert set(res.engines.values()) == {"device"}, res.engines
    torch.cuda.synchronize()
    return time.perf_counter() - t0, models


def replay_us(base, n=200):
    """Microseconds per replayed step of the three models' captured graph, replayed back to back."""
    step = ExactGPFitStep({k: copy.deepcopy(m) for k, m in base.items()}, LR, num_iters=n + 1)
    step.step()
    graph = step.capture()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        graph.replay()
    torch.cuda.synchronize()
    return round(1e6 * (time.perf_counter() - t0) / n, 2), step.launches_per_step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="24,64,256,512")
    ap.add_argument("--dims", default="2,8")
    a = ap.parse_args()
    for n in [int(s) for s in a.sizes.split(",")]:
        for d in [int(s) for s in a.dims.split(",")]:
            base = problem(n, d)
            first = {e: timed(base, e, a.iters)[0] for e in ("host", "device")}      # warm-up
            res = {"n": n, "d": d, "iters": a.iters, "repeats": a.repeats, "first_call_s": {k: round(v, 4) for k, v in first.items()}}
            times, fitted = {"host": [], "device": []}, {}
            for _ in range(a.repeats):
                for e in ("host", "device"):
                    t, fitted[e] = timed(base, e, a.iters)
                    times[e].append(t)
            for e in times:
                res[e] = {"median_s": round(statistics.median(times[e]), 4), "spread_s": round(max(times[e]) - min(times[e]), 4)}
            res["speedup"] = round(res["host"]["median_s"] / res["device"]["median_s"], 2)
            us, (launches, factorisations) = replay_us(base)
            res["replay_us_per_step"], res["launches_per_step"], res["factorisations_per_step"] = us, launches, factorisations
            with torch.no_grad():
                flat = lambda m: torch.cat([p.reshape(-1) for p in m.parameters()])      # noqa: E731
                res["max_parameter_difference"] = max(float((flat(fitted["host"][k]) - flat(fitted["device"][k])).abs().max()) for k in base)
                res["mll"] = {e: [round(float(m.marginal_log_likelihood()), 6) for m in fitted[e].values()] for e in fitted}
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
