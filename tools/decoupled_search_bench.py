#!/usr/bin/env python3
"""What the decoupled search costs (JESMOC_MFDGP.get_nextpoint_decoupled, DecoupledDeviceAcqSearch, mobocmf_jes_mc_box_forward)
at N = M = 64 (44 low + 20 high fidelity) with three black-boxes (two objectives + one constraint), K in {1, 4}:

  launch   microseconds of the per-box JES launch alone in selected-box mode with seeds and tracking (200 launches captured as
           one graph chain, replayed: device time) at T = 15 (the replayed iterate: three boxes x five restarts) and T = 200,
           and of the all-box mode at T = 200 (the raw candidates); beside each the coupled launch on the same inputs
  k<K>     seconds per get_nextpoint_decoupled on the host engine and on the device engine (median of three calls after one
           that builds groups, descriptors and graphs), and microseconds per replayed decoupled iterate (T = 15) beside the
           coupled iterate (T = 5) of the same models, per fidelity

Every step runs in a fresh child process under its own time limit; the first step that fails or runs out of time ends the run
(nothing more is started on the device after a failure).  One JSON line per step.

usage: python tools/decoupled_search_bench.py [--steps launch,k1,k4] [--epochs 300] [--cond-iters 200] [--iters 50]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LIMIT_S = {"launch": 120, "k1": 300, "k4": 420}      # per step, in its own process


def _replay_us(engines, rounds=7, n=1000):
    """Microseconds per replayed iterate of each engine's captured one-iterate graph, per fidelity: median and spread of
    ``rounds`` windows of ``n`` replays (the group frozen, as in a search)."""
    import torch
    out = {}
    for f, eng in sorted(engines.items()):
        graph, ts = eng._graphs[1], []
        with eng.group.frozen():
            for r in range(rounds + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    graph.replay()
                torch.cuda.synchronize()
                if r:      # (round 0 warms up)
                    ts.append(1e6 * (time.perf_counter() - t0) / n)
        out[f] = {"median": round(statistics.median(ts), 2), "spread": round(max(ts) - min(ts), 2), "T": eng.T}
    return out


def step_k(a, K):
    import torch
    from jes_mc_bench import _add_boxes, _unconditioned
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP
    fitter = _unconditioned(a, 44, 20)
    acq = _add_boxes(JESMOC_MFDGP(model=fitter, num_fidelities=2, search="device", num_pareto_samples=K, pareto_seed=1,
                                  standard_bounds=torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device="cuda")))
    out = {"step": "k%d" % K, "K": K, "N": 64, "boxes": 3, "search_iters": a.iters, "seconds_per_call": {}, "engines": {}, "choice": {}}
    for engine in ("host", "device"):
        acq.search = engine
        ts = []
        for r in range(4):      # (call 0 builds groups, descriptors and graphs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, fidelity, name, _ = acq.get_nextpoint_decoupled(maxiter=a.iters, generator=torch.Generator(device="cuda").manual_seed(0))
            torch.cuda.synchronize()
            if r:
                ts.append(time.perf_counter() - t0)
        out["seconds_per_call"][engine] = {"median": round(statistics.median(ts), 4), "spread": round(max(ts) - min(ts), 4)}
        out["engines"][engine] = dict(acq.last_search_engine)
        out["choice"][engine] = [int(fidelity), name, [round(float(v), 6) for v in x]]
    acq.search = "device"
    acq.get_nextpoint_coupled(maxiter=a.iters, generator=torch.Generator(device="cuda").manual_seed(0))
    torch.cuda.synchronize()
    out["models_per_group"] = len(acq._decoupled_searches[1].group.models)
    out["replay_us_per_iterate"] = {"decoupled": _replay_us(acq._decoupled_searches), "coupled": _replay_us(acq._device_searches)}
    return out


def step_launch(a):
    import torch
    from mobocmf_amd import functional as F
    out = {"step": "launch", "n_boxes": 3, "S": 5, "launches_per_window": 20000, "windows": 7, "us_per_launch": {}}
    g = torch.Generator().manual_seed(0)

    def graph_of(fn, n=200):
        fn()
        torch.cuda.synchronize()
        graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            for _ in range(n):
                fn(stream)
        return graph, n

    def us(graphs, replays=100, rounds=7):
        times = {name: [] for name in graphs}
        for r in range(rounds + 1):
            for name, (graph, n) in graphs.items():      # the graphs alternate inside every round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(replays):
                    graph.replay()
                e1.record()
                torch.cuda.synchronize()
                if r:      # (round 0 warms up)
                    times[name].append(1e3 * e0.elapsed_time(e1) / (replays * n))
        return {name: {"median": round(statistics.median(t), 3), "spread": round(max(t) - min(t), 3)} for name, t in times.items()}

    for T in (15, 200):
        for K in (1, 4):
            B, S, d = 3, 5, 2
            n = B * (1 + K)
            mom = torch.empty(n, 2, T * S, dtype=torch.float64)
            mom[:, 0] = torch.randn(n, T * S, dtype=torch.float64, generator=g)
            mom[:, 1] = 0.05 + 1.95 * torch.rand(n, T * S, dtype=torch.float64, generator=g)
            mom, noise = mom.cuda(), (1e-3 + 0.099 * torch.rand(n, dtype=torch.float64, generator=g)).cuda()
            acq, seeds, rows = torch.zeros(T, dtype=torch.float64, device="cuda"), torch.zeros_like(mom), torch.zeros(B, T, dtype=torch.float64, device="cuda")
            x, best_x = torch.rand(T, d, dtype=torch.float64, device="cuda"), torch.zeros(T, d, dtype=torch.float64, device="cuda")
            best_v = torch.full((T,), float("-inf"), dtype=torch.float64, device="cuda")
            words = (torch.arange(T, device="cuda") // (T // B)).clamp(max=B - 1).to(torch.int32)
            kw = dict(seeds=seeds, x=x, best_v=best_v, best_x=best_x)
            key = "T%d_K%d" % (T, K)
            graphs = {key + "_box_selected": graph_of(lambda st=None, a=(mom, noise, K, T, S, acq), kw=kw:
                                                      F.jes_mc_box_forward(*a, box_of_point=words, stream=st, **kw)),
                      key + "_coupled": graph_of(lambda st=None, a=(mom, noise, K, T, S, acq), kw=kw:
                                                 F.jes_mc_group_forward(*a, stream=st, **kw))}
            if T == 200:
                graphs[key + "_box_all"] = graph_of(lambda st=None, a=(mom, noise, K, T, S, rows): F.jes_mc_box_forward(*a, stream=st))
            out["us_per_launch"].update(us(graphs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="launch,k1,k4")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--cond-iters", type=int, default=200)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if a.step is not None:
        res = step_launch(a) if a.step == "launch" else step_k(a, int(a.step[1:]))
        print(json.dumps(res), flush=True)
        return 0
    for step in a.steps.split(","):
        if step not in LIMIT_S:
            ap.error("unknown step %r" % step)
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--epochs", str(a.epochs), "--cond-iters",
               str(a.cond_iters), "--iters", str(a.iters)]
        try:
            rc = subprocess.run(cmd, timeout=LIMIT_S[step]).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": step, "error": "time limit of %d s" % LIMIT_S[step]}), flush=True)
            return 124
        if rc != 0:      # nothing more is started after a failed step
            print(json.dumps({"step": step, "error": "exit status %d" % rc}), flush=True)
            return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
