#!/usr/bin/env python3
"""Cost of the recommendation and its score on the GPU, against the host MOOP.compute_pareto_front for the masks:

  mask_uniform_ms    functional.pareto_mask on 200 000 x 3 uniform rows
  mask_simplex_ms    functional.pareto_mask on 20 000 x 3 near-simplex rows (nearly every row on the front)
  hv3_ms             functional.hypervolume, k = 3, P = 2 000 points of a front
  hv4_ms             functional.hypervolume, k = 4, P = 500 points of a front

Each GPU time is the median of --reps calls after one warm-up, each call ending in a device synchronise (the hypervolume
synchronises itself).  ``--host`` adds the host MOOP times of the two mask cases (one call each) and checks that the masks
agree.  One JSON line on stdout.

    python tools/pareto_hv_bench.py [--reps 20] [--host]
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


def simplex(rng, n, k, jitter=1e-3):
    x = np.abs(rng.normal(size=(n, k)))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x + jitter * rng.uniform(size=(n, k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host", action="store_true", help="also time the host MOOP on the two mask cases")
    a = ap.parse_args()
    from mobocmf_amd import functional as F
    from mobocmf_amd.util.moop import MOOP
    rng = np.random.default_rng(0)
    uni = rng.uniform(size=(200_000, 3))
    smp = simplex(rng, 20_000, 3)
    out = {"device": torch.cuda.get_device_name(0)}
    for name, pts in (("uniform", uni), ("simplex", smp)):
        t = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()
        out["mask_%s_ms" % name] = _timed(lambda: F.pareto_mask(t), a.reps)
        m, c = F.pareto_mask(t)
        out["front_%s" % name] = int(c[1])
        if a.host:
            t0 = time.perf_counter()
            ref = MOOP.compute_pareto_front(pts)
            out["host_mask_%s_ms" % name] = 1e3 * (time.perf_counter() - t0)
            out["mask_%s_equal" % name] = bool(np.array_equal(ref, m.cpu().numpy()))
    for k, P in ((3, 2000), (4, 500)):
        f = torch.from_numpy(np.ascontiguousarray(simplex(rng, P, k, 0.0))).cuda()
        ref = [1.1] * k
        out["hv%d_ms" % k] = _timed(lambda: F.hypervolume(f, ref), a.reps)
        out["hv%d" % k] = F.hypervolume(f, ref)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
