#!/usr/bin/env python3
"""Cost of the joint Pareto sampling step at the reference's sizes (d = 8, F = 500, grid 1000 d^2 + N rows), K black-boxes:

  draw_ms        K chain samples (layers.rff.sample_chain_from_posterior, host float64)
  exchange_ms    parallel.all_gather_samples of the K packed samples inside a one-rank RCCL group, and its payload bytes
  grid_batched_ms / grid_per_callable_ms
                 all K samples on the grid: ONE mobocmf_rff_eval_chains launch (grid uploaded once, values stay on the GPU)
                 against the per-callable path (per sample: grid upload, one mobocmf_rff_eval per layer, values back)
  moop_batched_ms / moop_per_callable_ms
                 the whole MOOP.compute_pareto_solution_from_samples (SLSQP refinements included) on both paths
  refine_slsqp_ms / refine_device_ms
                 the refinement stage alone, every objective's constrained optimum from the same grid values: the host SLSQP
                 runs (MOOP.optimize_obj_globally) against ONE mobocmf_rff_refine launch (16 starts per objective, start
                 selection and read-back included).  For these and the next two fields every constraint's threshold is the 0.4
                 quantile of its sample on the grid, so that constraints are active (the -10 of the fields above leaves every
                 constraint inactive); refine_device_minus_slsqp: per objective, device optimum - SLSQP optimum (the grid's
                 best where a refinement returns nothing)
  moop_slsqp_refine_ms / moop_device_refine_ms
                 the whole MOOP at those thresholds with refine="slsqp" / refine="device"

One JSON line per run on stdout.  Times are medians of --reps runs after one warm-up, each ending in a device synchronise.

    python tools/pareto_sample_bench.py [--reps 5] [--K 3 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def bench_K(K, d, F, N, reps):
    from mobocmf_amd import functional as Fn
    from mobocmf_amd import parallel
    from mobocmf_amd.layers import rff
    from mobocmf_amd.util import synthetic
    from mobocmf_amd.util.moop import MOOP
    models = [synthetic.model_from_problem(synthetic.make_problem(d=d, L=2, M=40, N=N, S=1, output=k, seed=k),
                                           device="cuda") for k in range(K)]
    gen = lambda k: torch.Generator().manual_seed(1000 + k)
    draw = lambda: [rff.sample_chain_from_posterior(m, nFeatures=F, generator=gen(k)) for k, m in enumerate(models)]
    rec = {"K": K, "draw_ms": _timed(draw, reps)}
    chains = draw()
    calls = [m.sample_function_from_each_layer(nFeatures=F, generator=gen(k))[-1] for k, m in enumerate(models)]
    bufs = [c.pack() for c in chains]
    rec["exchange_ms"] = _timed(lambda: parallel.all_gather_samples(bufs, list(range(K))), reps)
    rec["payload_bytes"] = int(sum(8 * b.numel() for b in bufs))
    inputs = np.random.default_rng(0).random((N, d))
    grid = np.concatenate([np.random.default_rng(1).random((1000 * d * d, d)), inputs])
    rec["grid_rows"] = int(grid.shape[0])
    params, layers, base = [], [], 0
    for c, b in zip(chains, bufs):
        layers.append(c.layer_offsets(base))
        base += b.numel()
    params = torch.cat(bufs).cuda()

    def batched_grid():
        return Fn.rff_eval_chains(torch.from_numpy(grid).cuda(), params, layers)[: K].cpu().numpy()

    def per_callable_grid():
        return np.stack([f(grid) for f in calls])

    rec["grid_batched_ms"] = _timed(batched_grid, reps)
    rec["grid_per_callable_ms"] = _timed(per_callable_grid, reps)
    diff = np.abs(batched_grid() - per_callable_grid()).max()
    rec["grid_max_abs_diff"] = float(diff)
    n_obj = max(1, K // 2)
    thr = np.full(K - n_obj, -10.0)

    def moop(samples):
        m = MOOP(samples[:n_obj], samples[n_obj:], input_dim=d, grid_size=1000 * d, pareto_set_size=50,
                 feasible_values=thr, rng=np.random.default_rng(2))
        return m.compute_pareto_solution_from_samples(inputs)

    rec["moop_batched_ms"] = _timed(lambda: moop(chains), max(1, reps // 2))
    rec["moop_per_callable_ms"] = _timed(lambda: moop(calls), max(1, reps // 2))
    a, b = moop(chains), moop(calls)
    rec["moop_same_set"] = bool(np.array_equal(a[0].numpy(), b[0].numpy()))
    rec["moop_front_max_rel_diff"] = float(np.abs(a[1].numpy() - b[1].numpy()).max() / max(1.0, np.abs(b[1].numpy()).max()))

    # the refinement stage, constraints active
    vals = Fn.rff_eval_chains(torch.from_numpy(grid).cuda(), params, layers).cpu().numpy()
    thr_q = np.array([np.quantile(vals[n_obj + i], 0.4) for i in range(K - n_obj)])

    def moop_q(refine):
        return MOOP(chains[:n_obj], chains[n_obj:], input_dim=d, grid_size=1000 * d, pareto_set_size=50,
                    feasible_values=thr_q, rng=np.random.default_rng(2), refine=refine)

    m = moop_q("device")
    fgrid, evals = m._feasible_grid_batched(grid, torch.device("cuda", 0), False)
    slsqp = lambda: [m.optimize_obj_globally(chains[j], chains[n_obj:], evals[:, j], fgrid) for j in range(n_obj)]
    rec["refine_slsqp_ms"] = _timed(slsqp, max(1, reps // 2))
    rec["refine_device_ms"] = _timed(lambda: m._refine_device(evals, fgrid), reps)
    best = lambda opts: [float(evals[:, j].min()) if o is None else float(chains[j](o)[0]) for j, o in enumerate(opts)]
    f_slsqp = best(slsqp())
    out = Fn.rff_refine(torch.stack([torch.from_numpy(fgrid[np.argsort(evals[:, j], kind="stable")[:m.refine_starts]]).cuda()
                                     for j in range(n_obj)]), params, layers, obj=list(range(n_obj)),
                        cons=[list(range(n_obj, K))] * n_obj, thr=[thr_q] * n_obj)
    f_dev = [min(float(f), float(evals[:, j].min())) if np.isfinite(f) else float(evals[:, j].min())
             for j, f in enumerate(out["f_best"].cpu().numpy())]
    rec["refine_device_minus_slsqp"] = [a - b for a, b in zip(f_dev, f_slsqp)]
    rec["moop_slsqp_refine_ms"] = _timed(lambda: moop_q("slsqp").compute_pareto_solution_from_samples(inputs), max(1, reps // 2))
    rec["moop_device_refine_ms"] = _timed(lambda: moop_q("device").compute_pareto_solution_from_samples(inputs), reps)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--F", type=int, default=500)
    ap.add_argument("--N", type=int, default=100)
    a = ap.parse_args()
    out = {"tool": "pareto_sample_bench", "d": a.d, "F": a.F, "N": a.N}
    if not torch.cuda.is_available():
        out["results"] = "not measured (no GPU)"
        print(json.dumps(out))
        return
    import torch.distributed as dist
    from mobocmf_amd import parallel
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(parallel._free_port()))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        out["device"] = torch.cuda.get_device_name(0)
        out["results"] = [bench_K(K, a.d, a.F, a.N, a.reps) for K in a.K]
    finally:
        dist.destroy_process_group()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
