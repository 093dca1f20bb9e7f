#!/usr/bin/env python3
"""``MOOP(search="evolve")`` measured: two objectives and one constraint (at its 0.4 quantile) as hand-built chain samples of 2
layers x 24 features, d in {2, 8}, population Np in {64, 128, 512}.  Per (d, Np), one JSON line with

  * ``replay_us``: microseconds per generation of the captured graph replayed back to back (``--replays`` of them between two
    synchronisations, host clock);
  * ``launch_us``: microseconds per launch of a generation, each step issued eagerly ``--replays`` times back to back in a run
    of its own (device events): vary, eval (mobocmf_rff_eval_chains on the Np children), feasibility, copies (the two
    element-wise ones), survive (2 Np rows);
  * ``moop_s``: seconds of one ``compute_pareto_solution_from_samples`` call with ``refine="device"`` -- ``grid`` (draw, upload,
    evaluation and feasibility of the 1000 d rows), ``evolve`` (the whole evolve stage: engine construction, the eager first
    generation, the capture, ``--generations`` - 1 replays, the read-back, the append) and ``total``; the median of ``--repeats``;
  * ``hv``: hypervolume (reference = max + 0.1 of the feasible values of a 400 000-point random search) of the default
    mode's front, of the evolved front of the same ``rng``, and of that random search's front.

usage: python tools/pareto_evolve_bench.py [--generations 100] [--replays 200] [--repeats 5] [--dims 2,8] [--pops 64,128,512]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobocmf_amd import functional as F  # noqa: E402
from mobocmf_amd.layers.rff import RFFChainSample  # noqa: E402
from mobocmf_amd.util.hypervolume import HV  # noqa: E402
from mobocmf_amd.util.moop import MOOP  # noqa: E402
from mobocmf_amd.util.pareto_evolve import ParetoEvolve  # noqa: E402

DEV = "cuda"


def random_chain(d, nf, seed):
    """A two-layer chain sample with unit hyper-parameters and random draws, on the GPU."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    ru = lambda *s: 2.0 * math.pi * torch.rand(*s, dtype=torch.float64, generator=g)
    s = math.sqrt(2.0 / nf)
    layers = [{"kind": 0, "F": nf, "alpha": 1.0, "scales": (s, 0.0, 0.0), "W1": 2.0 * rn(nf, d), "b1": ru(nf), "theta": rn(nf)},
              {"kind": 1, "F": nf, "a1": 1.0, "af": 1.0, "a2": 1.0, "nu": 1.0, "scales": (s, s, s), "W1": 0.5 * rn(nf, d),
               "b1": ru(nf), "theta": rn(3 * nf), "Wf": rn(nf), "W2": 2.0 * rn(nf, d), "b2": ru(nf)}]
    return RFFChainSample.unpack(RFFChainSample(layers, d).pack(), DEV)


def operands(samples):
    bufs, layers, base = [], [], 0
    for s in samples:
        b = s.pack()
        layers.append(s.layer_offsets(base))
        bufs.append(b)
        base += b.numel()
    return torch.cat(bufs).to(DEV), layers


def event_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(1e3 * a.elapsed_time(b) / n, 2)


def engine_times(params, layers, thr, d, Np, replays):
    eng = ParetoEvolve(params, layers, 2, thr, Np, d, seed=1)
    eng.start(torch.rand(Np, d, dtype=torch.float64, generator=torch.Generator().manual_seed(Np)))
    eng.run(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        eng._graph.replay()
    torch.cuda.synchronize()
    replay = round(1e6 * (time.perf_counter() - t0) / replays, 2)
    p, lib, st = F._ptr, eng.lib, F._stream
    vals = eng.vals
    launch = {
        "vary": event_us(eng._vary, replays),
        "eval": event_us(lambda: lib.mobocmf_rff_eval_chains(eng.K, d, Np, p(eng.X[Np:]), p(eng.params), eng.params.numel(),
                                                             p(eng.desc), p(vals), st()), replays),
        "feasibility": event_us(lambda: lib.mobocmf_rff_feasibility(eng.n_con, Np, p(vals[2:]), Np, p(eng.thr), p(eng.ok),
                                                                    p(eng.viol_raw), st()), replays),
        "copies": event_us(lambda: (torch.neg(eng.viol_raw, out=eng.viol[Np:]), eng.F[:, Np:].copy_(vals[:2])), replays),
        "survive": event_us(lambda: eng._survive(2 * Np, None), replays),
    }
    return replay, launch


def moop_times(samples, thr, d, Np, generations, repeats):
    inputs = np.random.default_rng(5).random((10, d))
    spans = {}

    def timed(name, fn):
        def wrapper(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            spans[name] = time.perf_counter() - t0
            return out
        return wrapper

    rows, fronts = [], {}
    for rep in range(repeats + 1):                        # (the first call loads and warms everything up: dropped)
        for mode in ("grid", "evolve"):
            moop = MOOP(samples[:2], samples[2:], input_dim=d, grid_size=1000, feasible_values=thr, refine="device",
                        rng=np.random.default_rng(9), search=mode, evolve_population=Np, evolve_generations=generations)
            moop._feasible_grid_batched = timed("grid", moop._feasible_grid_batched)
            moop._evolve_device = timed("evolve", moop._evolve_device)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = moop.compute_pareto_solution_from_samples(inputs)
            total = time.perf_counter() - t0
            fronts[mode] = out[1].numpy()
            if mode == "evolve" and rep:
                rows.append((spans["grid"], spans["evolve"], total))
    med = lambda i: round(statistics.median(r[i] for r in rows), 5)
    return {"grid": med(0), "evolve": med(1), "total": med(2)}, fronts


def random_search_front(params, layers, thr, d, n=400000):
    X = torch.rand(n, d, dtype=torch.float64, generator=torch.Generator().manual_seed(77)).to(DEV)
    vals = F.rff_eval_chains(X, params, layers)
    ok, _ = F.rff_feasibility(vals[2:], torch.as_tensor(thr).to(DEV))
    feas = vals[:2, ok].T.contiguous()
    mask, _ = F.pareto_mask(feas.T.contiguous())
    return feas[mask].cpu().numpy(), feas.max(0).values.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=100)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dims", default="2,8")
    ap.add_argument("--pops", default="64,128,512")
    a = ap.parse_args()
    for d in [int(v) for v in a.dims.split(",")]:
        samples = [random_chain(d, 24, 20 + k) for k in range(3)]
        thr = np.array([float(np.quantile(samples[2](np.random.default_rng(2).random((2000, d))), 0.4))])
        params, layers = operands(samples)
        rs_front, rs_max = random_search_front(params, layers, thr, d)
        hv = HV(ref_point=rs_max + 0.1)
        for Np in [int(v) for v in a.pops.split(",")]:
            replay, launch = engine_times(params, layers, thr, d, Np, a.replays)
            secs, fronts = moop_times(samples, thr, d, Np, a.generations, a.repeats)
            print(json.dumps({"d": d, "Np": Np, "generations": a.generations, "replay_us": replay, "launch_us": launch,
                              "launch_sum_us": round(sum(launch.values()), 2), "moop_s": secs,
                              "hv": {"grid": hv(fronts["grid"]), "evolve": hv(fronts["evolve"]), "random_400000": hv(rs_front)},
                              "front_points": {"grid": len(fronts["grid"]), "evolve": len(fronts["evolve"])}}), flush=True)


if __name__ == "__main__":
    main()
