#!/usr/bin/env python3
"""How many epochs a warm-started refit (``warm_start="posterior"``) saves when one observation is appended.

Problems: the toy 2-D problem of examples/bo_iteration_toy2d.py (two objectives, one constraint, N = M from 20 up) and a
synthetic three-surrogate problem (``synthetic.target``, d = 8) at N = M = 64; Adam and ``variational_optimizer="natgrad"``
(one-launch steps, ``natgrad_one_launch=True``); seeds 0-2.  Per setting:

  1. the predecessor: a fit from scratch on the N rows (phase 1 + phase 2, the schedule of ``--epochs1 / --epochs2``);
  2. from scratch on the N + 1 rows, same schedule: seconds (construction included, device synchronised) and the final -ELBO;
  3. warm start from 1. on the N + 1 rows, phase 2 only (``--warm-epochs``, default: epochs2): -ELBO every 50 epochs, seconds
     (construction included; the time of the -ELBO evaluations taken out, the verification every 50 epochs left in);
  4. the first recorded epoch at which the warm run is at or below the from-scratch final value, or "never".

-ELBO here is the sum over the three black-boxes of the negative ELBO on all N + 1 rows, averaged over 16 fixed draws of the
hidden-layer eps (the same draws for every run of a setting), evaluated outside the training step.

    python tools/warm_start_bench.py [--epochs1 300] [--epochs2 300] [--warm-epochs E] [--sizes 20,32,48] [--seeds 0,1,2]
                                     [--out warm_start_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from bo_iteration_toy2d import blackboxes  # noqa: E402
from mobocmf_amd.models.mfdgp import TL  # noqa: E402
from mobocmf_amd.util import blackbox_mfdgp_fitter as BF  # noqa: E402
from mobocmf_amd.util import synthetic  # noqa: E402

EVERY, DRAWS, DEV = 50, 16, "cuda"


def toy_problem(n, seed):
    """n + 1 rows of the toy problem (0.7 n low-fidelity rows first, as the example), the last one the appended observation."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n + 1, 2))
    n_low = int(round(0.7 * n))
    fid = np.concatenate([np.zeros(n_low), np.ones(n - n_low), [float(seed % 2)]])
    ys = {name: (np.where(fid == 0, lo(x), hi(x)), is_con) for name, (lo, hi, is_con) in blackboxes().items()}
    return x, fid, ys


def synthetic_problem(n, seed):
    """n + 1 rows in [0, 1]^8, a quarter at the top fidelity first; three surrogates (outputs 0-2 of ``synthetic.target``)."""
    rng = np.random.default_rng(seed)
    x = rng.random((n + 1, 8))
    fid = np.concatenate([np.ones(n // 4), np.zeros(n - n // 4), [float(seed % 2)]])
    ys = {}
    for o, name in enumerate(("obj1", "obj2", "con1")):
        lo, hi = synthetic.target(x, o)
        ys[name] = (np.where(fid == 0, lo, hi), name == "con1")
    return x, fid, ys


def build(x, fid, ys, epochs1, epochs2, optimizer, previous=None):
    kw = dict(variational_optimizer="natgrad", natgrad_one_launch=True) if optimizer == "natgrad" else {}
    fitter = BF.BlackBoxMFDGPFitter(2, x.shape[0], num_epochs_1=epochs1, num_epochs_2=epochs2, type_lengthscale=TL.MEDIAN,
                                    device=DEV, **kw)
    fitter.verbose = False
    for name, (y, is_con) in ys.items():
        start = {} if previous is None else dict(previously_trained_model=previous.get_model(name, is_constraint=is_con),
                                                 warm_start="posterior")
        fitter.initialize_mfdgp(torch.from_numpy(x), torch.from_numpy(y)[:, None], torch.from_numpy(fid)[:, None], name,
                                is_constraint=is_con, **start)
    return fitter


def neg_elbo(fitter, eps):
    """Sum over the black-boxes of -ELBO on their rows (rolled by one, so that layer 0 takes the general branch as in training),
    averaged over the fixed draws ``eps`` (DRAWS, N)."""
    total = 0.0
    with torch.no_grad():
        for _, _, h in fitter._handlers():
            x, y, f = (t.roll(1, 0) for t in h.train_dataset.tensors)
            for e in eps:
                total += -float(h.elbo(h.mfdgp(x, eps=[None, e.roll(1, 0)]), y.T, f)[0]) / len(eps)
    torch.cuda.synchronize()
    return total


def timed_fit(make):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fitter = make()
    fitter.train_mfdgps()
    torch.cuda.synchronize()
    return fitter, time.perf_counter() - t0


def one_setting(problem, n, seed, optimizer, epochs1, epochs2, warm_epochs):
    x, fid, ys = problem(n, seed)
    old = {k: (y[:n], c) for k, (y, c) in ys.items()}
    eps = torch.randn(DRAWS, n + 1, dtype=torch.float64, generator=torch.Generator().manual_seed(1000 + seed)).to(DEV)
    torch.manual_seed(seed)
    previous, _ = timed_fit(lambda: build(x[:n], fid[:n], old, epochs1, epochs2, optimizer))
    scratch, t_scratch = timed_fit(lambda: build(x, fid, ys, epochs1, epochs2, optimizer))
    target = neg_elbo(scratch, eps)
    # the warm run: the trainer verifies (and here reports) every EVERY epochs; the reports evaluate -ELBO, their time is taken out
    curve, t_eval = [], [0.0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    warm = build(x, fid, ys, 0, warm_epochs, optimizer, previous=previous)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0

    def evaluate(epoch):
        torch.cuda.synchronize()
        t = time.perf_counter()
        curve.append((epoch, neg_elbo(warm, eps)))
        t_eval[0] += time.perf_counter() - t

    evaluate(0)
    last = len(warm._handlers()) - 1
    warm.verbose = True
    # (one report per black-box and verification; the last one of a verification records the state after epoch i)
    warm._print_epoch = lambda tag, k, i, num, loss, kl: evaluate(i + 1) if (tag, k) == warm._handlers()[last][:2] else None
    keep = BF.ITER_PRINT
    BF.ITER_PRINT = EVERY
    try:
        warm.train_mfdgps()
    finally:
        BF.ITER_PRINT = keep
    torch.cuda.synchronize()
    t_warm = time.perf_counter() - t0 - t_eval[0]
    reached = next((e for e, v in curve if v <= target), None)
    return dict(n=n, seed=seed, optimizer=optimizer, scratch_final=target, scratch_seconds=t_scratch, warm_start_value=curve[0][1],
                warm_final=curve[-1][1], warm_seconds=t_warm, warm_build_seconds=t_build, reached_at=reached,
                warm_epochs=warm_epochs, curve=curve)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs1", type=int, default=300)
    ap.add_argument("--epochs2", type=int, default=300)
    ap.add_argument("--warm-epochs", type=int, default=None)
    ap.add_argument("--sizes", default="20,32,48", help="N = M of the toy problem before the row is appended")
    ap.add_argument("--seeds", default="0,1,2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    warm_epochs = a.epochs2 if a.warm_epochs is None else a.warm_epochs
    settings = [("toy2d", toy_problem, int(n)) for n in a.sizes.split(",")] + [("synthetic3", synthetic_problem, 64)]
    rows = []
    print("problem      N  optimizer seed | scratch: -ELBO      s | warm: -ELBO at 0   final      s (build) | reached at epoch")
    for name, problem, n in settings:
        for optimizer in ("adam", "natgrad"):
            for seed in (int(s) for s in a.seeds.split(",")):
                r = one_setting(problem, n, seed, optimizer, a.epochs1, a.epochs2, warm_epochs)
                r["problem"] = name
                rows.append(r)
                print("%-10s %3d  %-8s %4d | %14.4f %6.2f | %14.4f %10.4f %6.2f (%.2f) | %s" %
                      (name, n, optimizer, seed, r["scratch_final"], r["scratch_seconds"], r["warm_start_value"], r["warm_final"],
                       r["warm_seconds"], r["warm_build_seconds"],
                       r["reached_at"] if r["reached_at"] is not None else "never within %d epochs" % warm_epochs))
                sys.stdout.flush()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(epochs1=a.epochs1, epochs2=a.epochs2, warm_epochs=warm_epochs, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
