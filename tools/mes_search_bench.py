#!/usr/bin/env python3
"""The acquisition search of the MES baseline, host engine against device engine (MESMOC_MFGP(search=...)): two objectives (an
MFGP and an MFGP_lin) and one constraint (MFGP) on n training rows each, two fidelities, 5 restarts of 200 raw candidates,
``--iters`` iterations, at n = 24 / 64 / 256 and d = 2 / 8.  The models are initialised, not fitted: the time of a search does
not depend on the hyper-parameters' values.

Both engines are warmed up once (group construction, graph capture: reported as one-off cost), then whole
``get_nextpoint_coupled`` calls are timed with a host clock around a final synchronise, the engines alternating in the same
process, from equal generator states; the median of ``--repeats`` calls is reported with the spread, and the time per replayed
iterate (the captured four-launch graph replayed back to back against factorisations formed once).  The host engine is the
baseline.  One JSON line per (n, d).

usage: python tools/mes_search_bench.py [--iters 200] [--repeats 3] [--sizes 24,64,256] [--dims 2,8]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mobocmf_amd.acquisition_functions.MESMOC_MFGP import MESMOC_MFGP  # noqa: E402
from mobocmf_amd.models.mfgp import MFGP, MFGP_lin  # noqa: E402

DEV = "cuda"
N_FID = 2


def problem(n, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    models = {}
    for k, (name, cls) in enumerate((("o0", MFGP), ("o1", MFGP_lin), ("c0", MFGP))):
        x = torch.rand(n, d, generator=g, dtype=torch.float64)
        fid = (torch.arange(n) % N_FID).double()[:, None]
        y = torch.sin(3.0 * x.sum(1) + k) + 0.3 * fid[:, 0] + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
        models[name] = cls(torch.cat([x, fid], 1), y, N_FID).to(DEV)
    bounds = torch.tensor([[0.0] * d, [1.0] * d], dtype=torch.float64, device=DEV)
    acq = MESMOC_MFGP({"o0": models["o0"], "o1": models["o1"]}, {"c0": models["c0"]}, d, N_FID, {"o0": 0.3, "o1": -0.2},
                      {"c0": 0.1}, standard_bounds=bounds)
    for f in range(N_FID):
        acq.add_blackbox(f, "o0", cost_evaluation=1.0 + f)
        acq.add_blackbox(f, "o1", cost_evaluation=1.0 + f)
        acq.add_blackbox(f, "c0", is_constraint=True)
    return acq


def timed(acq, engine, iters, seed=0):
    acq.search = engine
    gen = torch.Generator(device=DEV).manual_seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cand, fidelity = acq.get_nextpoint_coupled(maxiter=iters, generator=gen)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, cand.detach().cpu(), fidelity


def replay_us(acq, n=200):
    """Microseconds per iterate of the captured graph replayed back to back, per fidelity (the group frozen for the replays:
    its descriptors point at factorisations that exist between freeze() and thaw())."""
    out = {}
    for f, (_, eng, _) in sorted(acq._device_searches.items()):
        graph = eng._graphs[1]
        with eng.group.frozen():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                graph.replay()
            torch.cuda.synchronize()
            out[f] = round(1e6 * (time.perf_counter() - t0) / n, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="24,64,256")
    ap.add_argument("--dims", default="2,8")
    a = ap.parse_args()
    for n in [int(s) for s in a.sizes.split(",")]:
        for d in [int(s) for s in a.dims.split(",")]:
            acq = problem(n, d)
            first = {e: timed(acq, e, a.iters)[0] for e in ("host", "device")}      # warm-up: groups, descriptors, graph capture
            res = {"n": n, "d": d, "iters": a.iters, "repeats": a.repeats,
                   "first_call_s": {k: round(v, 4) for k, v in first.items()}, "engines": dict(acq.last_search_engine)}
            times = {"host": [], "device": []}
            for _ in range(a.repeats):
                for e in ("host", "device"):
                    t, cand, fidelity = timed(acq, e, a.iters)
                    times[e].append(t)
                    res[e] = {"candidate": [round(float(c), 6) for c in cand], "fidelity": fidelity}
            for e in times:
                res[e]["median_s"] = round(statistics.median(times[e]), 4)
                res[e]["spread_s"] = round(max(times[e]) - min(times[e]), 4)
            res["speedup"] = round(res["host"]["median_s"] / res["device"]["median_s"], 2)
            res["replay_us_per_iterate"] = replay_us(acq)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
