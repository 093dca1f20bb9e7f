#!/usr/bin/env python3
"""The acquisition search of one BO iteration, host engine against device engine (JESMOC_MFDGP(search=...)), at the sizes of
tools/bo_iteration_mid.py -- N = M = 64 (44 low + 20 high fidelity), two objectives + one constraint, 2 fidelities, 5 restarts of
200 raw candidates, 200 iterations: the cooperative kernel -- at N = M = 20 (14 + 6: the one-workgroup kernel), and above the
one-launch kernels at N = M = 160 (112 + 48) and 512 (358 + 154): the frozen-chain predict kernel (util/panel_predict.py), and at
640 (448 + 192) and 1024 (717 + 307): its split form.  ``--force-split`` routes 128 < M <= 512 to the split form too (a measurement
only: the library's routing is untouched).

Both engines are warmed up once (group construction, graph capture: reported as one-off cost), then whole
``get_nextpoint_coupled`` calls are timed with a host clock around a final synchronise, the engines alternating in the same
process, from equal generator states; the median of ``--repeats`` calls is reported, with the time per replayed iterate (the
captured graph replayed back to back), the same with several iterates per graph (``--unroll``), the chosen fidelity and the
distance between the two engines' candidates; ``spread_s`` is the largest minus the smallest of the repeats.  One JSON line per
size.

usage: python tools/acq_search_bench.py [--epochs 300] [--cond-iters 200] [--iters 200] [--repeats 5] [--unroll 1,4,8]
                                        [--sizes 64,20 | 160,512 | 640,1024] [--force-split]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import bo_iteration_toy2d as B  # noqa: E402

SPLIT = {64: (44, 20), 20: (14, 6), 160: (112, 48), 512: (358, 154), 640: (448, 192), 1024: (717, 307)}


def timed(acq, engine, iters, seed=0):
    acq.search = engine
    gen = torch.Generator(device="cuda").manual_seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cand, fidelity = acq.get_nextpoint_coupled(maxiter=iters, generator=gen)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, cand.detach().cpu(), fidelity


def replay_us(acq, per, n=200):
    """Microseconds per iterate of the captured graph of ``per`` iterates replayed back to back, per fidelity.  Only a graph
    that a search has captured is replayed: captured here, with the group thawed, it would lack STEP_CHAIN_VALID and stay
    cached for the searches that follow.  A frozen-chain group reads chains that only exist between freeze() and thaw(): it is
    frozen for the replays."""
    out = {}
    for f, eng in sorted(acq._device_searches.items()):
        assert per in eng._graphs, "replay_us: run a search with iters_per_graph = %d first" % per
        graph = eng._graphs[per]
        with eng.group.frozen():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n // per):
                graph.replay()
            torch.cuda.synchronize()
            out[f] = round(1e6 * (time.perf_counter() - t0) / (n // per * per), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--cond-iters", type=int, default=200)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--unroll", default="1,4,8")
    ap.add_argument("--sizes", default="64,20")
    ap.add_argument("--force-split", action="store_true")
    a = ap.parse_args()
    if a.force_split:
        from mobocmf_amd.util import panel_predict
        panel_predict.PanelPredictGroup.why_not = classmethod(lambda cls, *args, **kw: "switched off by --force-split")
    unroll = [int(u) for u in a.unroll.split(",")]
    for size in [int(s) for s in a.sizes.split(",")]:
        n_low, n_high = SPLIT[size]
        _, acq, _, _ = B.run(epochs=a.epochs, cond_iters=a.cond_iters, acq_iters=1, n_low=n_low, n_high=n_high, verbose=False)
        first = {e: timed(acq, e, a.iters)[0] for e in ("host", "device")}      # warm-up: groups, descriptors, graph capture
        res = {"size": size, "iters": a.iters, "repeats": a.repeats, "first_call_s": {k: round(v, 4) for k, v in first.items()},
               "engines": dict(acq.last_search_engine),
               "groups": sorted({type(g).__name__ for g in acq.__dict__.get("_panel_groups", {}).values() if g is not None})}
        times = {"host": [], "device": []}
        for _ in range(a.repeats):
            for e in ("host", "device"):
                t, cand, fidelity = timed(acq, e, a.iters)
                times[e].append(t)
                res[e] = {"candidate": [round(float(c), 6) for c in cand], "fidelity": fidelity}
        for e in times:
            res[e]["median_s"] = round(statistics.median(times[e]), 4)
            res[e]["min_s"] = round(min(times[e]), 4)
            res[e]["spread_s"] = round(max(times[e]) - min(times[e]), 4)
        res["candidate_distance"] = float((torch.tensor(res["host"]["candidate"]) - torch.tensor(res["device"]["candidate"])).norm())
        res["unroll"] = {}
        for per in unroll:
            for eng in acq._device_searches.values():
                eng.iters_per_graph = per
            timed(acq, "device", a.iters)      # captures the graph of ``per`` iterates
            ts = [timed(acq, "device", a.iters)[0] for _ in range(a.repeats)]
            res["unroll"][per] = {"median_s": round(statistics.median(ts), 4), "replay_us_per_iterate": replay_us(acq, per)}
        for eng in acq._device_searches.values():
            eng.iters_per_graph = type(eng).iters_per_graph
        acq.search = "host"
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
