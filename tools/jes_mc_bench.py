#!/usr/bin/env python3
"""What averaging the JES acquisition over K sampled Pareto sets costs and buys (JESMOC_MFDGP(num_pareto_samples=K),
mobocmf_jes_mc_group_forward), K in {1, 2, 4, 8}:

  launch   microseconds of the JES launch alone (200 launches captured as one graph chain, replayed: device time, no Python call
           per launch) at the shapes of the replayed iterate (three black-boxes, T = 5, S = 5) and of the raw-candidate scoring
           (T = 200): mobocmf_jes_mc_group_forward at every K and, alternating with it at K = 1, mobocmf_jes_group_forward
           ("_pair_entry": the same kernel behind the pair entry point, which must cost nothing more)
  k<K>     N = M = 64 (44 low + 20 high fidelity), two objectives + one constraint: seconds for the K conditioned fits (the
           time inside train_conditioned_mfdgps, synchronised; the Pareto sampling is reported apart) and microseconds per
           replayed iterate of the device search, per fidelity
  spread   the toy problem (14 + 6 points): from ONE unconditioned fit, the candidate the device search chooses and its coupled
           acquisition value for 8 Pareto seeds, K = 1 against K = 8 -- how much the choice depends on the seed

Every step runs in a fresh child process under its own time limit; the first step that fails or runs out of time ends the run
(nothing more is started on the device after a failure).  One JSON line per step.

usage: python tools/jes_mc_bench.py [--steps launch,k1,k2,k4,k8,spread] [--epochs 300] [--cond-iters 200] [--iters 50]
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

LIMIT_S = {"launch": 120, "k1": 240, "k2": 240, "k4": 300, "k8": 420, "spread": 480}      # per step, in its own process
BOXES = (("obj1", False), ("obj2", False), ("con1", True))


def _add_boxes(acq):
    for f in range(2):
        for name, is_con in BOXES:
            acq.add_blackbox(f, name, cost_evaluation=1.0 if f == 0 else 10.0, is_constraint=is_con)
    return acq


def _unconditioned(a, n_low, n_high):
    """The fitter of bo_iteration_toy2d.run after the unconditioned fit (no Pareto solution yet), cond_iters set."""
    import numpy as np
    import torch
    import bo_iteration_toy2d as B
    from mobocmf_amd.models.mfdgp import TL
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    np.random.seed(0)
    x = rng.uniform(size=(n_low + n_high, 2))
    fid = np.concatenate([np.zeros(n_low), np.ones(n_high)])
    fitter = BlackBoxMFDGPFitter(2, x.shape[0], num_epochs_1=a.epochs, num_epochs_2=a.epochs, pareto_set_size=10,
                                 opt_grid_size=100, type_lengthscale=TL.MEDIAN, device="cuda")
    fitter.verbose = False
    for name, (lo, hi, is_con) in B.blackboxes().items():
        y = np.where(fid == 0, lo(x), hi(x))
        fitter.initialize_mfdgp(torch.from_numpy(x), torch.from_numpy(y)[:, None], torch.from_numpy(fid)[:, None], name,
                                is_constraint=is_con)
    fitter.train_mfdgps()
    fitter.num_epochs_2 = a.cond_iters
    return fitter


def _timed_fits():
    """Accumulates the synchronised time inside BlackBoxMFDGPFitter.train_conditioned_mfdgps; returns the accumulator."""
    import torch
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    acc = {"s": 0.0, "n": 0}
    original = BlackBoxMFDGPFitter.train_conditioned_mfdgps

    def timed(self, *args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = original(self, *args, **kw)
        torch.cuda.synchronize()
        acc["s"] += time.perf_counter() - t0
        acc["n"] += 1
        return out

    BlackBoxMFDGPFitter.train_conditioned_mfdgps = timed
    return acc


def _search(acq, iters, seed=0):
    import torch
    acq.search = "device"
    cand, fidelity = acq.get_nextpoint_coupled(maxiter=iters, generator=torch.Generator(device="cuda").manual_seed(seed))
    torch.cuda.synchronize()
    return cand, fidelity


def _replays(acq, rounds=7, n=1000):
    """Microseconds per replayed iterate, per fidelity: median and spread of ``rounds`` windows of ``n`` replays."""
    from acq_search_bench import replay_us
    runs = [replay_us(acq, 1, n=n) for _ in range(rounds)]
    return {f: {"median": round(statistics.median(r[f] for r in runs), 2),
                "spread": round(max(r[f] for r in runs) - min(r[f] for r in runs), 2)} for f in runs[0]}


def step_k(a, K):
    import torch
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP
    fitter = _unconditioned(a, 44, 20)
    acc = _timed_fits()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    acq = _add_boxes(JESMOC_MFDGP(model=fitter, num_fidelities=2, search="device", num_pareto_samples=K, pareto_seed=1,
                                  standard_bounds=torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device="cuda")))
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    _search(acq, a.iters)      # groups, descriptors, graph capture
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _search(acq, a.iters)
        ts.append(time.perf_counter() - t0)
    return {"step": "k%d" % K, "K": K, "N": 64, "cond_iters": a.cond_iters, "conditioned_fits": acc["n"],
            "conditioned_fits_s": round(acc["s"], 4), "pareto_sampling_and_copies_s": round(total - acc["s"], 4),
            "engines": dict(acq.last_search_engine), "models_per_group": len(acq._device_searches[1].group.models),
            "search_s_median": round(statistics.median(ts), 4), "search_iters": a.iters,
            "replay_us_per_iterate": _replays(acq)}


def step_launch(a):
    import torch
    from mobocmf_amd import functional as F
    out = {"step": "launch", "n_boxes": 3, "S": 5, "launches_per_window": 20000, "windows": 7, "us_per_launch": {}}
    g = torch.Generator().manual_seed(0)

    def graph_of(fn, n=200):
        """``n`` launches captured as one chain: a replay times the device, not the Python call around each launch."""
        fn()
        torch.cuda.synchronize()
        graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            for _ in range(n):
                fn(stream)
        return graph, n

    def us(graphs, replays=100, rounds=7):
        """Per named graph the median and the spread (largest minus smallest) of ``rounds`` windows of ``replays`` replays,
        the graphs alternating inside every round."""
        times = {name: [] for name in graphs}
        for r in range(rounds + 1):
            for name, (graph, n) in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(replays):
                    graph.replay()
                e1.record()
                torch.cuda.synchronize()
                if r:      # (round 0 warms up)
                    times[name].append(1e3 * e0.elapsed_time(e1) / (replays * n))
        return {name: {"median": round(statistics.median(t), 3), "spread": round(max(t) - min(t), 3)} for name, t in times.items()}

    for T in (5, 200):
        for K in (1, 2, 4, 8):
            n, S, d = 3 * (1 + K), 5, 2
            mom = torch.empty(n, 2, T * S, dtype=torch.float64)
            mom[:, 0] = torch.randn(n, T * S, dtype=torch.float64, generator=g)
            mom[:, 1] = 0.05 + 1.95 * torch.rand(n, T * S, dtype=torch.float64, generator=g)
            mom, noise = mom.cuda(), (1e-3 + 0.099 * torch.rand(n, dtype=torch.float64, generator=g)).cuda()
            acq, seeds = torch.zeros(T, dtype=torch.float64, device="cuda"), torch.zeros_like(mom)
            x, best_x = torch.rand(T, d, dtype=torch.float64, device="cuda"), torch.zeros(T, d, dtype=torch.float64, device="cuda")
            best_v = torch.full((T,), float("-inf"), dtype=torch.float64, device="cuda")
            kw = dict(seeds=seeds, x=x, best_v=best_v, best_x=best_x)
            key = "T%d_K%d" % (T, K)
            graphs = {key: graph_of(lambda st=None, a=(mom, noise, K, T, S, acq), kw=kw:
                                    F.jes_mc_group_forward(*a, stream=st, **kw))}
            if K == 1:
                graphs[key + "_pair_entry"] = graph_of(lambda st=None, a=(mom, noise, T, S, acq), kw=kw:
                                                       F.jes_group_forward(*a, stream=st, **kw))
            out["us_per_launch"].update(us(graphs))
    return out


def step_spread(a):
    import torch
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP
    base = _unconditioned(a, 14, 6)
    bounds = torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device="cuda")
    out = {"step": "spread", "N": 20, "pareto_seeds": 8, "cond_iters": a.cond_iters, "search_iters": a.iters}
    for K in (1, 8):
        cands, vals, fids = [], [], []
        for seed in range(8):
            fitter = base.copy_uncond()
            torch.manual_seed(100 + seed)
            acq = _add_boxes(JESMOC_MFDGP(model=fitter, num_fidelities=2, search="device", num_pareto_samples=K,
                                          pareto_seed=1000 + seed, standard_bounds=bounds))
            cand, fidelity = _search(acq, a.iters)
            cands.append(cand.detach().cpu())
            fids.append(int(fidelity))
            vals.append(float(acq.last_search_values[fidelity]))
        c = torch.stack(cands)
        out["K%d" % K] = {"values": [round(v, 6) for v in vals], "fidelities": fids,
                          "value_mean": round(statistics.mean(vals), 6), "value_std": round(statistics.pstdev(vals), 6),
                          "value_std_over_mean": round(statistics.pstdev(vals) / max(statistics.mean(vals), 1e-300), 4),
                          "candidate_std": [round(float(s), 4) for s in c.std(0, unbiased=False)],
                          "engines": dict(acq.last_search_engine)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="launch,k1,k2,k4,k8,spread")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--cond-iters", type=int, default=200)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if a.step is not None:
        res = step_launch(a) if a.step == "launch" else step_spread(a) if a.step == "spread" else step_k(a, int(a.step[1:]))
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
