#!/usr/bin/env python3
"""Cost of functional.select_inducing (greedy conditional-variance selection of inducing points) in both forms, against the
numpy statement of the same rules on the host:

    (N, M, d) = (512, 128, 2), (2048, 256, 8), (8192, 512, 8), (65536, 1024, 32)      uniform rows, lengthscale sqrt(d) / 2

  form1_ms / form2_ms   median of --reps calls after one warm-up, each call ending in a device synchronise (the wrapper
                        reads ``count`` back).  Form 1 (one workgroup) is skipped above --form1-max-n rows.
  host_ms               the numpy oracle, one call (skipped above --host-max-n rows); picks_equal_host compares the picks
                        (they may differ once the residuals reach rounding level: max_resid_left says whether they did)
  model_*               what form 2 has to move: N M^2 / 2 doubles of factor reads, and its launch count
  crossover             the sizes where each form wins, from --sweep row counts at M = N / 4, d = 8: three alternated
                        rounds per form, the median of the rounds' medians and their spread (max - min)

One JSON line on stdout.  ``--only N`` restricts the run to one size (for a kernel trace of that size alone).

    python tools/inducing_select_bench.py [--reps 10] [--sweep] [--only 8192]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(512, 128, 2), (2048, 256, 8), (8192, 512, 8), (65536, 1024, 32)]
SWEEP = [256, 384, 512, 768, 1024, 2048, 4096]


def _timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", type=int, default=0, help="time this N of the size table only")
    ap.add_argument("--form1-max-n", type=int, default=8192)
    ap.add_argument("--host-max-n", type=int, default=8192)
    ap.add_argument("--sweep", action="store_true", help="also locate the crossover between the forms")
    a = ap.parse_args()
    from mobocmf_amd import functional as F
    from tests.test_inducing_select_cpu import greedy_oracle
    out = {"device": torch.cuda.get_device_name(0), "sizes": []}
    for N, M, d in SIZES:
        if a.only and N != a.only:
            continue
        x_np = np.random.default_rng(0).random((N, d))
        ls = np.sqrt(d) / 2
        x = torch.from_numpy(x_np).cuda()
        hyp = torch.tensor([1.0] + [ls] * d, dtype=torch.float64, device="cuda")
        row = {"N": N, "M": M, "d": d, "model_read_gb": N * M * M / 2 * 8 / 1e9, "model_launches": M + 3}
        reps = a.reps if N < 65536 else max(3, a.reps // 3)
        got = {}
        for form in (1, 2):
            if form == 1 and N > a.form1_max_n:
                continue
            row["form%d_ms" % form] = _timed(lambda: F.select_inducing(x, hyp, M, form=form), reps)
            got[form] = F.select_inducing(x, hyp, M, form=form)
        row["default_ms"] = _timed(lambda: F.select_inducing(x, hyp, M), reps)
        if 1 in got:
            row["forms_bitwise_equal"] = bool(torch.equal(got[1][0], got[2][0]) and torch.equal(got[1][1], got[2][1]) and
                                              torch.equal(got[1][2], got[2][2]))
        row["form2_read_gbps"] = row["model_read_gb"] / (row["form2_ms"] * 1e-3)
        row["form2_us_per_launch"] = 1e3 * row["form2_ms"] / (M + 3)
        if N <= a.host_max_n:
            t0 = time.perf_counter()
            o_idx, o_resid, _, _ = greedy_oracle(x_np, np.full(d, ls), 1.0, M)
            row["host_ms"] = 1e3 * (time.perf_counter() - t0)
            row["picks_equal_host"] = bool(np.array_equal(o_idx, got[2][0].cpu().numpy()))
            row["max_resid_left"] = float(got[2][2].max())
        out["sizes"].append(row)
    if a.sweep:
        sweep = []
        for N in SWEEP:
            x = torch.from_numpy(np.random.default_rng(0).random((N, 8))).cuda()
            hyp = torch.tensor([1.0] + [np.sqrt(8.0) / 2] * 8, dtype=torch.float64, device="cuda")
            reps = a.reps * (5 if N <= 1024 else 1)       # sub-millisecond calls: more of them, and the forms alternated
            t1, t2 = [], []
            for _ in range(3):
                t1.append(_timed(lambda: F.select_inducing(x, hyp, N // 4, form=1), reps, warmup=3))
                t2.append(_timed(lambda: F.select_inducing(x, hyp, N // 4, form=2), reps, warmup=3))
            sweep.append({"N": N, "M": N // 4, "form1_ms": float(np.median(t1)), "form2_ms": float(np.median(t2)),
                          "form1_spread_ms": max(t1) - min(t1), "form2_spread_ms": max(t2) - min(t2)})
        out["sweep"] = sweep
        wins1 = [s["N"] for s in sweep if s["form1_ms"] <= s["form2_ms"]]
        out["crossover"] = {"largest_N_where_form1_wins": max(wins1) if wins1 else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
